"""The small stage operators swept over their kernel forms, tails and launch caps (tests/stage_ops_cases.py): k_sum_partial /
k_sum_final / k_adjust_apply / k_norm_apply, k_make_isotropic<VEC>, k_weight_image, k_weights<...>, k_downsample2x, the bead
normalisation's k_minmax / k_norm_apply, and the decision point of k_pack_u16.

The CPU tests hold the restated caps and predicates to the launchers' source, decide the coverage from them, and show on the
sweep's own inputs that a plain NumPy restatement of every operator matches the oracle while each deliberate mistake does not.
The GPU tests hold the kernels to the oracle: bit for bit where the arithmetic is fixed (makeIsotropic, the weights, downSample2x,
the bead normalisation, adjustImage's two roundings), and to a bound counted from the reduction's structure where it is a sum."""
import math
import os
import re
import zlib

import numpy as np
import pytest

from . import stage_ops_cases as S
from .conftest import ROOT

F32 = np.float32
SEED = 464232194
RAMP_TOL = 6e-8          # one float32 ulp below 1: device cos against libm (test_make_isotropic_and_weight_image's)
ADJ_REL = 1.2e-7         # per voxel against the oracle (test_adjust_and_norm_match_oracle's limits)
ADJ_FRAC = 1e-4
MIN_VALUE = float(F32(0.0001))


def _ids(cs):
    return dict(argvalues=cs, ids=[c.id for c in cs])


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ NumPy restatements
def np_make_isotropic(v, inc, zdiv="float", mirror="single", acc="float"):
    nz = v.shape[0]
    z = np.arange((nz - 1) * inc + 1)
    pz = (z.astype(F32) / F32(inc)).astype(np.float64) if zdiv == "float" else z / float(inc)
    fz = np.floor(pz)
    w2 = (pz - fz)[:, None, None]
    w2n = 1.0 - w2

    def mir(i):
        if nz == 1:
            return np.zeros_like(i)
        p = 2 * nz - 2 if mirror == "single" else 2 * nz
        i = np.mod(i, p)
        return np.where(i < nz, i, (p if mirror == "single" else p - 1) - i)
    a = v[mir(fz.astype(np.int64))].astype(np.float64) * w2n
    b = v[mir(fz.astype(np.int64) + 1)].astype(np.float64) * w2
    if acc == "double":
        return (a + b).astype(F32)
    return a.astype(F32) + b.astype(F32)


def np_weight_image(shape, inclusive=False, half_up=False, reverse=True):
    nz, ny, nx = shape
    y = np.arange(ny)
    l = ny - y - 1 if reverse else y
    half = (ny + 1) // 2 if half_up else ny // 2
    pos = ((l - half).astype(np.float64) / float(S.COSINE_SPAN)) * 3.141592653589793
    ramp = ((np.cos(pos) + 1.0) / 2.0).astype(F32)
    one = l <= half if inclusive else l < half
    zero = l >= half + S.COSINE_SPAN if inclusive else l > half + S.COSINE_SPAN
    row = np.where(one, F32(1), np.where(zero, F32(0), ramp)).astype(F32)
    return np.broadcast_to(row[None, :, None], shape).copy()


def weight_plateaus(ny):
    """(rows that must be exactly 1, rows that must be exactly 0), by the reference's two tests."""
    l = ny - np.arange(ny) - 1
    return l < ny // 2, l > ny // 2 + S.COSINE_SPAN


def np_adjust(x, min_value, target, roundings=2, sub="float", sum_="exact"):
    if sum_ == "exact":
        s = math.fsum(x.tolist())
    else:
        s = float(np.cumsum(x, dtype=F32)[-1])            # sequential float accumulation
    with np.errstate(divide="ignore", invalid="ignore"):
        avg = np.float64(s) / np.float64(x.size)
        num = np.float64(F32(target) - F32(min_value)) if sub == "float" else np.float64(F32(target)) - np.float64(F32(min_value))
        corr = num / avg
        t = x.astype(np.float64) * corr
        if roundings == 1:
            return (t + np.float64(F32(min_value))).astype(F32), float(corr)
        return t.astype(F32) + F32(min_value), float(corr)


def np_normalize_weights(ws, osem, sum_="float", order="forward", clamp=True, early_zero=False):
    dt = F32 if sum_ == "float" else np.float64
    seq = ws if order == "forward" else ws[::-1]
    tot = np.zeros(ws[0].shape, dt)
    for w in seq:
        tot = tot + w.astype(dt)
    tot = tot.astype(F32)
    zero = tot == 0
    if early_zero:
        zero = zero | (ws[0] == 0)                         # the test taken after the first view
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for w in ws:
            r = F32(osem) * (w / tot)
            if clamp:
                r = np.where(r < 1, r, F32(1))
            out.append(np.where(zero, F32(0), r).astype(F32))
    return out


def np_view_sum(ws):
    tot = np.zeros(ws[0].shape, F32)
    for w in ws:
        tot = tot + w
    return tot


def np_downsample2x(v, order="gray", scale="taps"):
    oz, oy, ox = (s // 2 - 1 for s in v.shape)
    taps = {"gray": ((0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1), (1, 0, 0)),        # (dz, dy, dx)
            "plain": ((0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1))}[order]
    acc = None
    for dz, dy, dx in taps:
        t = v[dz:dz + 2 * oz:2, dy:dy + 2 * oy:2, dx:dx + 2 * ox:2]
        if scale == "taps":
            t = (t.astype(np.float64) * 0.125).astype(F32)
        acc = t.copy() if acc is None else acc + t
    return acc if scale == "taps" else (acc.astype(np.float64) * 0.125).astype(F32)


def np_beads_normalize(x, body_only=False):
    src = x[:x.size & ~3] if body_only else x
    mn = src.min() if src.size else F32(np.finfo(F32).max)
    mx = src.max() if src.size else F32(-np.finfo(F32).max)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return ((x - mn) / (mx - mn)).astype(F32)


# ------------------------------------------------------------------------------------------------ CPU: table, source, coverage
def test_case_list_is_deterministic_with_unique_ids():
    a, b = S.cases(), S.cases()
    assert a == b and len({c.id for c in a}) == len(a)
    for c in a:
        if c.op == "weight":                                     # no input: the interval alone
            continue
        x, y = S.inputs(c), S.inputs(c)
        xs, ys = (x, y) if isinstance(x, list) else ([x], [y])
        assert len(xs) == len(ys) and all(_same_bits(p, q) for p, q in zip(xs, ys)), c.id
        assert all(p.dtype == F32 and p.flags.c_contiguous for p in xs), c.id
        assert xs[0] is not ys[0]


def _source(name):
    return open(os.path.join(ROOT, "multiview-simulation_amd", "csrc", name)).read()


def _body(text, signature):
    """The text of the function whose definition starts with `signature`, up to its closing brace in column 0."""
    m = re.search(re.escape(signature) + r".*?\n\}\n", text, re.S)
    assert m, signature
    return m.group(0)


def _int(pattern, text):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1))


def test_restated_caps_and_predicates_are_the_launchers():
    """A cap or a predicate changed in the source must fail here, not quietly stop being crossed by the cases."""
    k, common = _source("kernels.hip"), _source("common.h")
    iso = _body(k, "int launch_make_isotropic(")
    assert _int(r"want > (\d+) \? \1 : want", iso) == S.ISO_BX_CAP
    assert _int(r"if \(onz > (\d+)\)", iso) == S.ISO_MAX_PLANES
    assert "const bool vec = plane % 4 == 0 && ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;" in iso
    assert "const long long per = vec ? plane / 4 : plane;" in iso and "(per + 255) / 256" in iso
    assert _int(r"want > (\d+) \? \1 : want", _body(k, "int launch_weight_image(")) == S.WEIGHT_IMAGE_CAP
    assert _int(r"want > (\d+) \? \1 : want", _body(k, "int launch_weights(")) == S.WEIGHTS_CAP
    assert _int(r"constexpr int SUM_BLOCKS = (\d+);", common) == S.SUM_BLOCKS
    lsum = _body(k, "int launch_sum(")
    assert "(n / 4 + 255) / 256" in lsum and "if (blocks > SUM_BLOCKS) blocks = SUM_BLOCKS;" in lsum
    adj = _body(k, "int launch_adjust_apply(")
    assert "(n / 4 + 255) / 256" in adj and _int(r"if \(blocks > (\d+)\) blocks = \1;", adj) == S.ADJUST_CAP
    nrm = _body(k, "int launch_norm_apply(")
    assert "(n + 255) / 256" in nrm and _int(r"if \(blocks > (\d+)\) blocks = \1;", nrm) == S.NORM_CAP
    # the 16-byte body of the sum and of the apply: n >> 2 float4s behind an aligned pointer, none otherwise
    for sig, ptr in (("void k_sum_partial(", "in"), ("void k_adjust_apply(", "img")):
        assert f"const long long n4 = ((reinterpret_cast<uintptr_t>({ptr}) & 15) == 0) ? (n >> 2) : 0;" in _body(k, sig), sig
    # the reduction the depth R is counted from
    assert "for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);" in _body(k, "double wave_sum(")
    assert "r = ((sh[0] + sh[1]) + (sh[2] + sh[3]));" in _body(k, "double block_sum_256(")
    assert "acc += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);" in _body(k, "void k_sum_partial(")
    assert "for (int i = threadIdx.x; i < count; i += 256) acc += partial[i];" in _body(k, "void k_sum_final(")
    assert _int(r"want > (\d+) \? \1 : want", _body(_source("phantom.hip"), "int launch_downsample2x(")) == S.DOWNSAMPLE_CAP
    b = _source("beads.hip")
    assert _int(r"constexpr int NORM_BLOCKS = (\d+);", b) == S.BEADS_MINMAX_CAP
    bn = _body(b, "int beads_normalize_dev(")
    assert "std::min<int64_t>(NORM_BLOCKS, (n + 255) / 256)" in bn
    assert _int(r"k_norm_apply, dim3\(std::min<int64_t>\((\d+), \(n \+ 255\) / 256\)\)", bn) == S.BEADS_APPLY_CAP
    header = open(os.path.join(ROOT, "include", "mvsim.h")).read()
    assert _int(r"#define MVSIM_MAX_VIEWS (\d+)", header) == S.MAX_VIEWS
    assert _int(r"cosine_span = (\d+);", open(os.path.join(ROOT, "oracle", "mvsim_oracle.c")).read()) == S.COSINE_SPAN
    assert f"l > ny / 2 + {S.COSINE_SPAN}" in _body(k, "void k_weight_image(")
    pack = _body(k, "void k_pack_u16(")
    assert "fminf(fmaxf(v, 0.f), 65535.f)" in pack


def test_sum_depths_are_the_written_ones():
    """R, written next to every sum case, is what the kernels' structure gives, and stays below 64 at every size."""
    for c in S.cases("adjust") + S.cases("norm"):
        assert c.R == S.sum_depth(c.n, c.aligned), (c.id, c.R, S.sum_depth(c.n, c.aligned))
        assert 0 < c.R < 64, c.id
    assert S.sum_depth(4, True) == 2 + 1 + 8 + 1 + 8           # one float4: 2 + one `acc +=`, 6 + 2, one partial, 6 + 2


def _coverage_key(c):
    """(operator, form, above its cap?, tail?) of a case, from the restated predicates."""
    if c.op == "iso":
        items = S.iso_items(c.plane, c.aligned)
        return ("iso", "vec" if S.iso_vec(c.plane, c.aligned) else "scalar", S.iso_above(c.plane, c.aligned), items % 256 != 0)
    if c.op == "weight":
        total = int(np.prod(c.shape))
        return ("weight", "scalar", S._want(total) > S.WEIGHT_IMAGE_CAP, total % 256 != 0)
    if c.op == "adjust":
        return ("adjust", "vec" if S.sum_vec(c.aligned) else "scalar", (S.sum_above(c.n), S.adjust_above(c.n)), c.n % 4 != 0)
    if c.op == "norm":
        return ("norm", "vec-sum", S.norm_above(c.n), c.n % 4 != 0)
    if c.op == "weights":
        return ("weights", "all", S._want(c.n) > S.WEIGHTS_CAP, c.n % 256 != 0)
    if c.op == "down":
        total = int(np.prod([s // 2 - 1 for s in c.shape]))
        return ("down", "scalar", S._want(total) > S.DOWNSAMPLE_CAP, total % 256 != 0)
    if c.op == "beads":
        return ("beads", "scalar", (S._want(c.n) > S.BEADS_MINMAX_CAP, S._want(c.n) > S.BEADS_APPLY_CAP), c.n % 4 != 0)
    raise AssertionError(c.op)


def _largest_array(c):
    if c.op == "iso":
        return c.plane * ((c.shape[0] - 1) * c.inc + 1)
    return max(c.n, int(np.prod(c.shape)) if c.shape else 0)


def test_sweep_covers_every_form_cap_and_tail():
    keys = {_coverage_key(c) for c in S.cases() if not c.refused}
    tf = (False, True)
    want = {("iso", f, a, t) for f in ("vec", "scalar") for a in tf for t in tf}
    want |= {("weight", "scalar", a, t) for a in tf for t in tf}
    # adjust: below both caps, past the sum's only, past both -- in the 16-byte form with and without a tail
    want |= {("adjust", "vec", a, t) for a in ((False, False), (True, False), (True, True)) for t in tf}
    want |= {("adjust", "scalar", a, t) for a, t in (((False, False), True), ((False, False), False), ((True, False), True))}
    want |= {("norm", "vec-sum", a, t) for a in tf for t in tf}
    want |= {("weights", "all", a, t) for a in tf for t in tf}
    want |= {("down", "scalar", False, t) for t in tf}          # its cap is crossed by test_simulate_phantom_full_size
    want |= {("beads", "scalar", a, t) for a in ((False, False), (True, False)) for t in tf} | {("beads", "scalar", (True, True), True)}
    assert want <= keys, sorted(want - keys, key=str)
    # the sizes the issue names as edges
    iso = S.cases("iso")
    assert {c.shape[0] for c in iso} >= {1, 2} and any(c.kind == "mixed" for c in iso)
    planes = {(c.shape[0] - 1) * c.inc + 1: c.refused for c in iso if c.shape == (2, 1, 1)}
    assert planes == {S.ISO_MAX_PLANES: False, S.ISO_MAX_PLANES + 1: True}
    assert any(c.offset and c.plane % 4 == 0 for c in iso)
    assert {c.shape[1] for c in S.cases("weight")} >= {1, 2, 39, 40, 41, 80, 81, 82, 100, 101}
    assert any(c.offset for c in S.cases("weight")) and any(c.offset for c in S.cases("adjust"))
    # 4 194 304 + 3 voxels are exactly 4096 blocks of k_adjust_apply: the cap is first exceeded four voxels later
    assert not S.adjust_above(4194304 + 3) and S.adjust_above(4194304 + 7)
    assert {c.kind for c in S.cases("adjust")} == {"uniform", "desc", "zeros"}
    w = S.cases("weights")
    assert {c.views for c in w} >= {1, 2, 7, S.MAX_VIEWS} and {c.n for c in w} >= {1, 255, 1920, 2097152 + 513}
    assert {p for c in w for p in S.weight_plants(c)} == set(S.WEIGHT_PATTERNS)
    assert {c.kind for c in S.cases("beads")} == set(S.BEADS_PLANTS) | {"none"}
    for c in S.cases():                                             # the largest buffer: about 17 MB per array
        assert _largest_array(c) * 4 <= 17.5e6 and (c.views < S.MAX_VIEWS or c.n < 2000), c.id


def test_planted_weight_patterns_do_what_they_are_for():
    c = next(c for c in S.cases("weights") if c.views == 7 and c.n == 1920)
    ws, at = S.inputs(c), S.weight_plants(c)
    col = lambda name: np.array([w[at[name]] for w in ws])
    fwd = np_view_sum(ws)
    assert fwd[at["all_zero"]] == 0 and not col("all_zero").any()
    assert fwd[at["plus_minus"]] == 0 and col("plus_minus")[0] > 0 and not np.signbit(fwd[at["plus_minus"]])
    assert np.signbit(col("neg_zero")).all()
    assert fwd[at["cancel4"]] == 1 and np_view_sum(ws[::-1])[at["cancel4"]] == 0 and col("cancel4").astype(np.float64).sum() == 2
    assert S.OSEM * col("dominant").max() / fwd[at["dominant"]] > 1


# ------------------------------------------------------------------------------------------------ CPU: sensitivity
def _oracle(orc, c):
    x = None if c.op == "weight" else S.inputs(c)
    if c.op == "iso":
        return orc.make_isotropic(x, c.inc)
    if c.op == "weight":
        return orc.compute_weight_image(c.shape)
    if c.op == "adjust":
        orc.adjust_image(x, MIN_VALUE, 1.0)
        return x
    if c.op == "weights":
        orc.normalize_weights(x, S.OSEM)
        return np.stack(x)
    if c.op == "down":
        return orc.downsample2x(x)
    if c.op == "beads":
        return np_beads_normalize(x)             # the reference is three lines of float arithmetic; there is no C restatement of it
    raise AssertionError(c.op)


def _restated(c, **mistake):
    x = None if c.op == "weight" else S.inputs(c)
    if c.op == "iso":
        return np_make_isotropic(x, c.inc, **mistake)
    if c.op == "weight":
        return np_weight_image(c.shape, **mistake)
    if c.op == "adjust":
        return np_adjust(x, MIN_VALUE, 1.0, **mistake)[0]
    if c.op == "weights":
        return np.stack(np_normalize_weights(x, S.OSEM, **mistake))
    if c.op == "down":
        return np_downsample2x(x, **mistake)
    if c.op == "beads":
        return np_beads_normalize(x, **mistake)
    raise AssertionError(c.op)


def _within(op, got, want):
    """The operator's tolerance, as its GPU test applies it."""
    if op == "weight":
        ny = want.shape[1]
        one, zero = weight_plateaus(ny)
        return bool((got[:, one] == 1).all() and (got[:, zero] == 0).all() and np.max(np.abs(got.astype(np.float64) - want)) <= RAMP_TOL)
    if op == "adjust":
        return _adjust_close(got, want)
    if op == "iso":
        return _same_bits(got, want)
    return np.array_equal(got, want, equal_nan=True)


def _rel_excess(got, want):
    """max(|got - want| - ADJ_REL |want|): <= 0 when every voxel is within the relative limit (a zero must then be a zero)."""
    want = want.astype(np.float64)
    return float(np.max(np.abs(got.astype(np.float64) - want) - ADJ_REL * np.abs(want)))


def _adjust_close(got, want):
    if np.isnan(want).any():
        return np.array_equal(got, want, equal_nan=True)
    return bool(np.mean(got != want) < ADJ_FRAC and _rel_excess(got, want) <= 0)


MISTAKES = {
    "iso": {"z / inc divided in double": dict(zdiv="double"), "mirror off by one (2n - 1 - i)": dict(mirror="double"),
            "the two taps accumulated in double": dict(acc="double")},
    "weight": {"ny / 2 rounded up": dict(half_up=True), "row index not reversed": dict(reverse=False)},
    "adjust": {"one rounding instead of two": dict(roundings=1), "target - min subtracted in double": dict(sub="double"),
               "a float sum": dict(sum_="float")},
    "weights": {"sum in double": dict(sum_="double"), "sum in reverse view order": dict(order="reverse"), "no clamp": dict(clamp=False),
                "sum == 0 tested before all views are summed": dict(early_zero=True)},
    "down": {"plain tap order instead of Gray-code order": dict(order="plain")},
    "beads": {"min and max over the vector body only": dict(body_only=True)},
}
# Two of the mistakes the sweep was asked to expose change no value on any finite input, so no input can expose them; the test
# below asserts exactly that, on every case, so that a change which makes them matter shows up here.
#   `<=` for `<` at both plateau tests: the ramp is exactly 1.0 at l == ny / 2 (cos 0) and exactly 0.0 at l == ny / 2 + 40
#       (cos of the double nearest pi rounds to -1.0), the values the plateaus give those two rows.
#   0.125 applied after the sum: a multiplication by a power of two commutes with every float rounding (no underflow at these inputs).
NOT_MISTAKES = {
    "weight": {"<= for < at both plateau tests": dict(inclusive=True)},
    "down": {"weight 0.125 applied after the sum": dict(scale="sum")},
}


def _sensitivity_cases(op):
    # the large cases add nothing a mistake could hide behind, except for the sums, whose depth they are about
    limit = {"adjust": 2200000}.get(op, 300000)
    return [c for c in S.cases(op) if not c.refused and _largest_array(c) <= limit]


@pytest.mark.parametrize("op", sorted(MISTAKES))
def test_sweep_inputs_expose_stage_operator_mistakes(orc, op):
    cs = _sensitivity_cases(op)
    want = {c.id: _oracle(orc, c) for c in cs}
    for c in cs:
        assert _within(op, _restated(c), want[c.id]), c.id                     # the restatement is the oracle's arithmetic
    for name, kw in MISTAKES[op].items():
        caught = [c.id for c in cs if not _within(op, _restated(c, **kw), want[c.id])]
        print(f"{op}: {name}: caught by {len(caught)} of {len(cs)} cases")
        assert caught, name
    for name, kw in NOT_MISTAKES.get(op, {}).items():
        assert all(_same_bits(_restated(c, **kw), _restated(c)) for c in cs), name


def test_inclusive_plateau_tests_change_no_row_at_any_height():
    for ny in range(1, 260):
        assert _same_bits(np_weight_image((1, ny, 1), inclusive=True), np_weight_image((1, ny, 1))), ny


# ------------------------------------------------------------------------------------------------ GPU
class _Dev:
    """Device buffers of one test, freed on exit; `off` floats of slack in front make a pointer that is only 4-byte aligned."""

    def __init__(self, ctx):
        self.ctx, self.bases = ctx, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.bases:
            self.ctx.dev_free(p)

    def alloc(self, nfloats, off=0):
        p = self.ctx.dev_alloc((nfloats + off) * 4)
        assert p % 16 == 0
        self.bases.append(p)
        return p + 4 * off

    def put(self, arr, off=0):
        p = self.alloc(arr.size, off)
        self.ctx.upload(p, arr)
        return p


@pytest.mark.gpu
@pytest.mark.parametrize("case", **_ids(S.cases("iso")))
def test_make_isotropic_sweep(ctx, orc, case):
    v = S.inputs(case)
    nz, ny, nx = case.shape
    if case.refused:
        with pytest.raises(ValueError):
            ctx.make_isotropic(v, case.inc)
        return
    want = orc.make_isotropic(v, case.inc)
    if case.offset:
        with _Dev(ctx) as d:
            src, dst = d.put(v, off=1), d.alloc(want.size, off=1)
            assert src % 16 == 4 and dst % 16 == 4
            ctx.make_isotropic_dev(src, (nx, ny, nz), case.inc, dst)
            got = ctx.download(dst, want.shape)
    else:
        got = ctx.make_isotropic(v, case.inc)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert _same_bits(got, want)                              # ... the signs of the zeros included


@pytest.mark.gpu
@pytest.mark.parametrize("case", **_ids(S.cases("weight")))
def test_weight_image_sweep(ctx, orc, case):
    nz, ny, nx = case.shape
    if case.offset:
        with _Dev(ctx) as d:
            dst = d.alloc(nz * ny * nx, off=1)
            ctx.compute_weight_image_dev((nx, ny, nz), dst)
            got = ctx.download(dst, case.shape)
    else:
        got = ctx.compute_weight_image(case.shape)
    want = orc.compute_weight_image(case.shape)
    one, zero = weight_plateaus(ny)
    assert (got[:, one, :] == 1.0).all() and (got[:, zero, :] == 0.0).all()
    err = float(np.max(np.abs(got.astype(np.float64) - want)))
    print(case.id, "plateau rows", int(one.sum()), int(zero.sum()), "max ramp error", err)
    assert err <= RAMP_TOL


def _gpu_adjust(ctx, case, x, min_value, target):
    """adjustImage on the GPU, in place on a copy: (adjusted, corr)."""
    a = x.copy()
    if not case.offset:
        return a, ctx.adjust_image(a, min_value, target)
    with _Dev(ctx) as d:
        p = d.put(a, off=1)
        assert p % 16 == 4
        corr = ctx.adjust_image_dev(p, a.size, min_value, target)
        return ctx.download(p, a.shape), corr


@pytest.mark.gpu
@pytest.mark.parametrize("case", **_ids(S.cases("adjust")))
def test_adjust_image_sweep(ctx, orc, case):
    """The sum is held to math.fsum within (R + 4) 2^-53 sum|x|: R additions on the reduction's longest path (written next to the
    case, counted from k_sum_partial and k_sum_final), one rounding each in sum / n, 1 / avg and n / corr here, one for the
    second-order terms.  k_adjust_apply is held bit for bit to the two-rounding rule with the GPU's own corr."""
    x = S.inputs(case)
    n = x.size
    exact = math.fsum(x.tolist())
    with np.errstate(divide="ignore", invalid="ignore"):
        for min_value, target in ((0.0, 1.0), (MIN_VALUE, 1.0)):
            got, corr = _gpu_adjust(ctx, case, x, min_value, target)
            if min_value == 0.0:
                gpu_sum = float(np.float64(n) / np.float64(corr))
                bound = (case.R + 4) * 2.0 ** -53 * math.fsum(np.abs(x).tolist())
                print(case.id, "R", case.R, "sum error", abs(gpu_sum - exact), "bound", bound)
                assert abs(gpu_sum - exact) <= bound
            rule = (x.astype(np.float64) * np.float64(corr)).astype(F32) + F32(min_value)
            assert np.array_equal(_bits(got), _bits(rule)) or (case.kind == "zeros" and np.array_equal(got, rule, equal_nan=True))
            want = x.copy()
            corr_o = orc.adjust_image(want, min_value, target)
            if case.kind == "zeros":
                assert corr == corr_o == math.inf and np.array_equal(got, want, equal_nan=True) and np.isnan(got).all()
                continue
            print(case.id, "corr", corr, corr_o, "voxels differing", float(np.mean(got != want)), "excess over the relative limit", _rel_excess(got, want))
            assert np.mean(got != want) < ADJ_FRAC and _rel_excess(got, want) <= 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", **_ids(S.cases("norm")))
def test_norm_image_sweep(ctx, orc, case):
    x = S.inputs(case)
    got, want = x.copy(), x.copy()
    ctx.norm_image(got)
    orc.norm_image(want)
    total = math.fsum(got.tolist())
    print(case.id, "voxels differing", float(np.mean(got != want)), "excess over the relative limit", _rel_excess(got, want), "sum", total)
    assert np.mean(got != want) < ADJ_FRAC and _rel_excess(got, want) <= 0
    assert abs(total - 1.0) <= 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("case", **_ids(S.cases("weights")))
def test_normalize_weights_sweep(ctx, orc, case):
    """k_weights in its three forms at every case: the host entry point (own sum), sum_views_dev (sum only), and
    normalize_weights_dev with the sum supplied -- there with a true -0.0 where every view holds -0.0."""
    ws = S.inputs(case)
    n, at = case.n, S.weight_plants(case)
    want = [w.copy() for w in ws]
    orc.normalize_weights(want, S.OSEM)
    got = [w.copy() for w in ws]
    ctx.normalize_weights(got, S.OSEM)
    for v in range(case.views):
        assert np.array_equal(got[v], want[v]), v
    if "dominant" in at:
        assert want[case.views - 1][at["dominant"]] == 1.0
    for name in ("all_zero", "plus_minus", "neg_zero"):
        if name in at:
            assert all(_bits(w)[at[name]] == 0 for w in got), name
    tot = np_view_sum(ws)
    with _Dev(ctx) as d:
        ptrs = [d.put(w) for w in ws]
        d_sum = d.alloc(n)
        ctx.sum_views_dev(ptrs, n, d_sum)
        assert np.array_equal(ctx.download(d_sum, (n,)), tot)
        if "neg_zero" in at:
            tot[at["neg_zero"]] = F32(-0.0)
            ctx.upload(d_sum, tot)
        ctx.normalize_weights_dev(ptrs, n, S.OSEM, sum_dptr=d_sum)
        for v in range(case.views):
            assert np.array_equal(ctx.download(ptrs[v], (n,)), want[v]), v


@pytest.mark.gpu
@pytest.mark.parametrize("case", **_ids(S.cases("down")))
def test_downsample2x_sweep(ctx, orc, case):
    v = S.inputs(case)
    got = ctx.downsample2x(v)
    assert got.shape == tuple(s // 2 - 1 for s in case.shape)
    assert np.array_equal(got, orc.downsample2x(v))


@pytest.mark.gpu
@pytest.mark.parametrize("case", **_ids(S.cases("beads")))
def test_beads_normalize_sweep(ctx, case):
    x = S.inputs(case)
    want = np_beads_normalize(x)
    got = x.copy()
    ctx.beads_normalize(got)
    assert np.array_equal(got, want, equal_nan=True)
    with _Dev(ctx) as d:
        p = d.put(x)
        ctx.beads_normalize_dev(p, x.size)
        assert np.array_equal(ctx.download(p, x.shape), want, equal_nan=True)
    if case.n == 1:
        assert np.isnan(got).all()                            # (v - v) / (max - min) = 0 / 0, as in the reference
    else:
        assert got.min() == 0.0 and got.max() == 1.0
        at = -1 if case.kind.endswith("last") else 0
        assert got[at] == (0.0 if case.kind.startswith("min") else 1.0)


@pytest.mark.gpu
def test_more_views_than_the_kernel_holds_are_refused(ctx):
    """MVSIM_MAX_VIEWS views pass, one more is refused by all three entry points before anything is launched.  (The plane count
    of makeIsotropic -- 65 535 accepted, 65 536 refused -- is in its sweep.)"""
    one = [np.ones(4, F32) for _ in range(S.MAX_VIEWS + 1)]
    with pytest.raises(ValueError):
        ctx.normalize_weights(one, S.OSEM)
    with _Dev(ctx) as d:
        p, q = d.put(one[0]), d.alloc(4)
        with pytest.raises(ValueError):
            ctx.normalize_weights_dev([p] * (S.MAX_VIEWS + 1), 4, S.OSEM)
        with pytest.raises(ValueError):
            ctx.sum_views_dev([p] * (S.MAX_VIEWS + 1), 4, q)
        assert np.array_equal(ctx.download(p, (4,)), one[0])
    ctx.normalize_weights(one[:S.MAX_VIEWS], S.OSEM)
    assert all(np.array_equal(w, np.full(4, S.OSEM / S.MAX_VIEWS, F32)) for w in one[:S.MAX_VIEWS])


# ------------------------------------------------------------------------------------------------ the uint16 boundary
U16_N = (1 << 20) + 5
U16_CANDIDATES = 20000
U16_STREAM = 3
U16_SEED = SEED


def u16_boundary_volumes(orc, seed=U16_SEED):
    """(lambdas whose largest count is exactly 65 535, the same with one count >= 65 536 kept, the kept counts, that count).
    The sampler is counter-based -- a voxel's count depends on its lambda and its index alone -- so the oracle gives the count of
    every candidate (lambda 65 535) in place, and the candidates that would exceed 65 535 go back to lambda 5."""
    rng = np.random.default_rng(zlib.crc32(b"u16-boundary"))
    lam = (4.0 + 2.0 * rng.random(U16_N)).astype(F32)
    where = np.sort(rng.choice(U16_N, U16_CANDIDATES, replace=False))
    where[-1] = U16_N - 1                                     # one candidate in the packer's scalar tail
    cand = np.full(U16_N, 5.0, F32)
    cand[where] = 65535.0
    counts = orc.poisson_counter_array(cand, 1.0, seed, U16_STREAM, 0)[where]
    keep = counts <= 65535
    below = lam.copy()
    below[where[keep]] = 65535.0
    over = int(where[~keep][0])
    above = below.copy()
    above[over] = 65535.0
    return below, above, counts[keep], float(counts[~keep][0])


def test_uint16_boundary_volume_holds_an_exact_65535(orc, mvs):
    """CPU: with this seed the kept candidates hold counts of exactly 65 535 (30 of them) and none above; the extra one is >= 65 536."""
    assert mvs._lib.load().mvsim_poisson_mul(float(np.sqrt(5.0))) == 1.0         # the values ARE the lambdas
    below, above, kept, over = u16_boundary_volumes(orc)
    hits = int((kept == 65535).sum())
    print("kept candidates", kept.size, "exact 65535", hits, "largest", float(kept.max()), "the one above", over)
    assert kept.size > U16_CANDIDATES // 3 and kept.max() == 65535 and hits == 30 and over >= 65536
    assert int((below != above).sum()) == 1


@pytest.mark.gpu
def test_counts_of_exactly_65535_cross_pcie_as_uint16(mvs, orc):
    """k_pack_u16's decision point: 2^20 + 5 lambdas (SNR sqrt 5: the values are the lambdas), about 5 everywhere except some 10 000
    voxels at lambda 65 535 whose counts the oracle says are <= 65 535 -- 30 of them exactly 65 535 with the seed above.  The volume
    must travel as uint16 (transfer statistics move by (1, 0)) and equal the float32 transfer bit for bit; with one more voxel kept
    whose count is >= 65 536 the transfer must fall back (1, 1) and be equal again."""
    snr = float(np.sqrt(5.0))
    below, above, kept, over = u16_boundary_volumes(orc)
    assert kept.max() == 65535 and (kept == 65535).sum() >= 1 and over >= 65536
    with mvs.Context(0) as c:
        def sample(x, transfer):
            c.set_option("acq_transfer", transfer)
            y = x.copy()
            c.poisson_process(y, snr, U16_SEED, stream=U16_STREAM)
            return y

        for name, x, moved, top in (("largest count 65535", below, (1, 0), 65535.0), ("one count above", above, (1, 1), over)):
            want = sample(x, "f32")
            before = c.transfer_stats()
            got = sample(x, "auto")
            after = c.transfer_stats()
            print(name, "stats", before, after, "max count", float(want.max()))
            assert np.array_equal(_bits(got), _bits(want)), name
            assert (after[0] - before[0], after[1] - before[1]) == moved, (name, before, after)
            assert want.max() == top, name
        assert np.array_equal(want, orc.poisson_counter_array(above, 1.0, U16_SEED, U16_STREAM, 0))
