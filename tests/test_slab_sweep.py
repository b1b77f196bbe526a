"""The z-slab tiling of one view swept over its own arithmetic (tests/slab_sweep_cases.py): the halo folded back at the global faces,
the direct z pass over a window of planes, the slab's share of adjustImage's sum, the compact and the non-compact extraction, the
global Poisson counters.  Every slab is held to the UNTILED view bit for bit: both sides are given the same total, so everything
behind the convolution is exact by construction and a wrong row, plane or counter cannot hide in a percentage.

Reference (parts that other sweeps hold to their own references): the oracle's rotate + attenuate, the untiled hand-written convolution
of the result (`raw`), adjustImage restated in numpy with the total T the slabs returned, the oracle's extractSlices with counter RNG.

Tiers.  Bit-exact: every case with zconv_strided=0 and fft_zpass=direct, early_sum 1 and 0, SNR -1 / 8 / 25; the fused-x-eligible
cases with fused_fftx 0 and 1.  Default options + exp=2: the cases with inc 2..4; their compact slabs may take the strided z pass
(another summation order: test_strided_z_pass_of_compact_views' limits), their non-compact slabs stay bit-exact.

Measured on an MI355X (30 cases, 110 slabs): every class of the bit-exact tier IS bit-exact -- "same per-plane transforms, same z taps
in the same order" holds for folds, deep halos, even depths, compact and non-compact extraction alike; no class needed the tolerance
tier.  Default options: the 41 non-compact slabs bit-exact; the 53 compact slabs within 3.6e-7 of the maximum (limit 3e-6), 4 of
285 760 counts differ (limit 2e-3).

Slab sums against the fp64 host sum of raw[z0:z1], relative to the sum of the whole raw: early_sum=1 3e-7 (the limit of
test_early_sum_from_the_spectrum_matches_pass_e; measured 4.7e-8 at most); early_sum=0 EARLY0_SUM_LIMIT = 1e-15, one decade above the
largest difference measured on these cases (9.6e-17, see there).  A slab whose own sum is 0 (all of its input planes are exact
zeros) is not run through the ONE-CALL check with noise: adjustImage's factor would be a division by zero and the sampler would be
handed NaN rates; it runs noise-free.

Found while writing it: for Kz >= Nz the halo was every plane of the view, not the smallest interval the taps reach (slab [0, 1) of
four planes under four taps reads the planes 0 .. 2): harmless to the result, but planes rotated and transformed for nothing.  The
general fold already yields the smallest interval there; the special case is gone from mvsim_view_slab_convolve_dev and halo_planes.

The CPU tests prove the class coverage, hold tiling.acquired_planes to enumeration and tiling.halo_planes to the oracle's convolution,
and show that a numpy restatement of the slab pipeline equals the untiled oracle pipeline and loses that equality with each classic
mistake planted."""
import importlib
import math
import types
import zlib

import numpy as np
import pytest

from . import slab_sweep_cases as S

CASES = S.cases()
STREAM = 5
SENTINEL = np.float32(-12345.0)
EARLY1_SUM_LIMIT = 3e-7
# early_sum=0: pass E reduces in fp64 the very floats the test sums.  Largest |slab sum - fp64 host sum| / sum(raw) measured over the
# 110 slabs of this module on an MI355X (case compact3): MEASURED_EARLY0 -- the order of an fp64 sum; the limit is one decade above it.
MEASURED_EARLY0 = 9.619e-17
EARLY0_SUM_LIMIT = 1e-15
STRIDED_SUM_LIMIT = 1e-6         # k_zconv_strided's sum from the tile's input rows (test_strided_z_pass_of_compact_views: the factor to 1e-6)
STRIDED_PLANE_LIMIT = 3e-6       # ... its planes, relative to the maximum
STRIDED_COUNT_LIMIT = 2e-3       # ... and the share of counts a moved rounding may change


def _tiling():
    return importlib.import_module("multiview-simulation_amd.tiling")


_ATT = {}


def _attenuated(orc, case):
    """The oracle's rotate + attenuate of the case's ground truth; computed once, read-only."""
    if case.id not in _ATT:
        a = orc.attenuate3d(orc.rotate_around_axis(S.ground_truth(case), 0, case.degrees), S.DELTA)
        a.flags.writeable = False
        _ATT[case.id] = a
    return _ATT[case.id]


def _zero_slabs(orc, case):
    """Slabs all of whose input planes, halo included, are exact zeros while the view is not."""
    att = _attenuated(orc, case)
    if not att.any():
        return []
    halo = _tiling().halo_planes
    return [(z0, z1) for z0, z1 in case.slabs if not att[slice(*halo(case.nz, case.kz, z0, z1))].any()]


# ------------------------------------------------------------------------------------------------ CPU: the case list
def test_case_list_is_deterministic_and_small():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids) and ids == [c.id for c in S.cases()]
    for c in CASES:
        nx, ny, nz = c.dim
        assert ny >= nx and 2 <= nz <= 80 and 1 <= c.kz <= 64, c.id
        if c.fused_eligible:
            assert nx >= 64 and S.CS.pick_x(nx + c.kdim[0] - 1) >= 72 and nz <= 12, c.id
        else:
            assert 12 <= nx <= 40 and 12 <= ny <= 40, c.id
        assert c.cuts[0] == 0 and c.cuts[-1] == nz and list(c.cuts) == sorted(set(c.cuts)), c.id
        if c.nslabs:
            assert c.slabs == [S.slab_range(nz, c.nslabs, r) for r in range(c.nslabs)], c.id
    assert 3 * sum(c.dim[1] > c.dim[0] for c in CASES) >= len(CASES)


def _tier3(case):
    """The default-options tier: spacings the strided z pass is instantiated for."""
    return case.inc in S.STRIDED_INCS


def test_cases_cover_every_class(orc):
    seen = set()
    for c in CASES:
        seen |= S.classes_of(c)
        if _zero_slabs(orc, c):
            seen.add("zero_slab")
    missing = (S.required_classes() | {"zero_slab"}) - seen
    assert not missing, sorted(missing)
    # the bit-exact tier runs every case; the fused-x cases run with fused_fftx 0 and 1 and hold a non-compact slab as well
    fused = [c for c in CASES if c.fused_eligible]
    assert fused and all(c.inc > 1 and any(not S.is_compact(z0, c.inc) for z0, _ in c.slabs) for c in fused)
    # the default-options tier: its compact slabs (tolerance) and its non-compact ones (bit-exact) still see every class that applies
    compact, plain = set(), set()
    for c in filter(_tier3, CASES):
        zero = _zero_slabs(orc, c)
        for z0, z1 in c.slabs:
            into = compact if S.is_compact(z0, c.inc) else plain
            into |= S.slab_classes(c, z0, z1) | {k for k in S.case_classes(c) if k.startswith("kz")}
            if (z0, z1) in zero:
                into.add("zero_slab")
    shared = {"kz_even", "kz_odd", "kz64", "kz_ge_nz", "halo_deeper_than_slab", "fold_low_only", "fold_high_only", "fold_both", "no_fold",
              "depth1", "first_acquired_is_last", "zero_slab"}
    want_compact = shared | {"kz1"} | {f"inc{i}_compact" for i in S.STRIDED_INCS}
    want_plain = shared | {"nzo0"} | {f"inc{i}_noncompact" for i in S.STRIDED_INCS}
    assert not want_compact - compact, sorted(want_compact - compact)
    assert not want_plain - plain, sorted(want_plain - plain)


# ------------------------------------------------------------------------------------------------ CPU: the restatements tiling rests on
def test_acquired_planes_against_enumeration():
    acq = _tiling().acquired_planes
    for inc in range(1, 9):
        for z0 in range(0, 40):
            for z1 in range(z0 + 1, 41):
                k0, k1 = acq(z0, z1, inc)
                assert list(range(k0, k1)) == [k for k in range(0, 41) if z0 <= k * inc < z1], (z0, z1, inc)
    # any tiling of [0, nz): the slabs' planes are range(extract_nz(nz, inc)), each once
    rng = np.random.default_rng(S.SEED)
    tilings = [c.cuts for c in CASES if c.nz <= 40]
    for nz in range(1, 41):
        tilings += [S.range_cuts(nz, n) for n in range(1, nz + 1)]
        tilings += [tuple([0] + sorted(rng.choice(np.arange(1, nz), size=min(nz - 1, int(rng.integers(1, 7))), replace=False).tolist()) + [nz])
                    for _ in range(8 if nz > 1 else 0)]
    for cuts in tilings:
        for inc in range(1, 9):
            got = [k for z0, z1 in zip(cuts, cuts[1:]) for k in range(*acq(z0, z1, inc))]
            assert got == list(range(S.extract_nz(cuts[-1], inc))), (cuts, inc)


def _reach(orc, nz, kz):
    """reach[i, o]: input plane i of a 1 x 1 x nz column changes output plane o of the ORACLE's convolution."""
    rng = np.random.default_rng(100 * nz + kz)
    base = rng.random((nz, 1, 1), dtype=np.float32) + 0.5
    psf = rng.random((kz, 1, 1), dtype=np.float32) + 0.5
    ref = orc.convolve_direct(base, psf.copy())
    reach = np.zeros((nz, nz), bool)
    for i in range(nz):
        v = base.copy()
        v[i] += 1.0
        reach[i] = (orc.convolve_direct(v, psf.copy()) != ref)[:, 0, 0]
    return reach


HALO_NZ_MAX = 9        # with every Kz in 1 .. 64: up to seven reflections of the taps' reach


def test_halo_planes_against_the_oracle_convolution(orc):
    """[za, zb) is the smallest interval that holds every input plane reaching an output of the slab -- read off the oracle's own
    convolution, so the tap orientation for even Kz (centre Kz / 2, no flip) is the oracle's and not a restatement's."""
    halo = _tiling().halo_planes
    n = 0
    for nz in range(1, HALO_NZ_MAX + 1):
        for kz in range(1, 65):
            reach = _reach(orc, nz, kz)
            assert reach.any(axis=0).all()
            # ... and the plain mirror rule enumerates the same planes (it carries the check to the sizes of the case list, below)
            for o in range(nz):
                assert np.flatnonzero(reach[:, o]).tolist() == S.reached_planes(nz, kz, o, o + 1), (nz, kz, o)
            for z0 in range(nz):
                for z1 in range(z0 + 1, nz + 1):
                    need = np.flatnonzero(reach[:, z0:z1].any(axis=1))
                    assert halo(nz, kz, z0, z1) == (int(need[0]), int(need[-1]) + 1), (nz, kz, z0, z1)
                    n += 1
    assert n > 10000


def test_halo_planes_against_the_mirror_rule_at_the_sweeps_sizes():
    halo = _tiling().halo_planes
    todo = {(c.nz, c.kz, z0, z1) for c in CASES for z0, z1 in c.slabs}
    for nz in (10, 17, 33, 64, 80):
        for kz in (1, 2, 3, 8, 31, 32, 63, 64):
            todo |= {(nz, kz, z0, z1) for z0 in range(0, nz, 3) for z1 in range(z0 + 1, nz + 1, 2)}
    for nz, kz, z0, z1 in sorted(todo):
        need = S.reached_planes(nz, kz, z0, z1)
        assert halo(nz, kz, z0, z1) == (need[0], need[-1] + 1), (nz, kz, z0, z1)


# ------------------------------------------------------------------------------------------------ CPU: sensitivity
MISTAKES = ("halo_short_low", "halo_short_high", "edge_repeating_mirror", "hl_c_swapped", "in_offset_off_by_one", "rng_offset_from_z0",
            "sum_over_halo")


def _dyadic_inputs(case, i):
    """An attenuated volume and z taps whose every product and sum is exact in float32 and in double, in any order: the restatement and
    the oracle then agree bit for bit or not at all.  Nx = Ny = 4 .. 6; dense and positive, the taps all different from their mirror
    images."""
    n = 4 + i % 3
    rng = np.random.default_rng(zlib.crc32(case.id.encode()) + 1)
    att = (rng.integers(1, 64, size=(case.nz, n, n)) / 8.0).astype(np.float32)
    a = np.array([1 + (t * 5) % 7 for t in range(case.kz)], dtype=np.int64)
    total = 1 << int(math.ceil(math.log2(a.sum()))) if a.sum() > 1 else 1
    a[0] += total - a.sum()
    taps = (a / float(total)).astype(np.float32)
    assert float(taps.astype(np.float64).sum()) == 1.0
    return att, taps


def _mirror(i, n, edge_repeating=False):
    if edge_repeating:                      # ... -1 -> 0, n -> n - 1: the edge plane twice
        p = 2 * n
        i %= p
        return i if i < n else p - 1 - i
    return S.mirror(i, n)


def _restated_convolve(att, taps, z0, z1, inc, mistake=None):
    """The slab's first call: cut the halo window, convolve its planes along z with the fold at the GLOBAL faces; returns the buffer the
    second call reads (the planes z0 + k * inc alone when the slab is compact), whether it is compact, and the slab's sum."""
    nz, kz = att.shape[0], len(taps)
    za, zb = _tiling().halo_planes(nz, kz, z0, z1)
    if mistake == "halo_short_low":
        za += 1
    if mistake == "halo_short_high":
        zb -= 1
    window = att[za:zb]
    c = kz // 2
    if mistake == "hl_c_swapped":
        c = kz - 1 - c
    zeros = np.zeros(att.shape[1:], np.float64)

    def plane(g):                           # a plane outside the window was never computed: whatever the buffer holds (here: zeros)
        g = _mirror(g, nz, mistake == "edge_repeating_mirror")
        return window[g - za].astype(np.float64) if za <= g < zb else zeros

    def conv(z):
        acc = zeros.copy()
        for t in range(kz):
            acc += np.float64(taps[t]) * plane(z + c - t)
        return acc.astype(np.float32)

    out = [conv(z) for z in range(z0, z1)]
    summed = range(za, zb) if mistake == "sum_over_halo" else range(z0, z1)
    total = float(sum(np.sum(conv(z), dtype=np.float64) for z in summed))
    compact = S.is_compact(z0, inc)
    return (out[::inc] if compact else out), compact, total


def _adjust(v, total, n):
    """Tools.adjustImage with a given sum, as k_adjust_corr and adjust_one state it."""
    corr = float(np.float64(np.float32(S.TARGET) - np.float32(S.MIN_VALUE)) / (np.float64(total) / np.float64(n)))
    return (np.asarray(v, np.float32).astype(np.float64) * corr).astype(np.float32) + np.float32(S.MIN_VALUE)


def _restated_finish(orc, buf, compact, shape, z0, z1, inc, snr, total, mistake=None):
    """The slab's second call: adjust with the view's total, extract (ExtractGeom::slab), counter Poisson on the GLOBAL voxel index."""
    nz, ny, nx = shape
    plane = ny * nx
    k0, k1 = _tiling().acquired_planes(z0, z1, inc)
    first = k0 * inc
    in_plane = 0 if compact else first - z0
    if mistake == "in_offset_off_by_one" and not compact:
        in_plane += 1
    stride = 1 if compact else inc
    index0 = (z0 if mistake == "rng_offset_from_z0" else first) * plane
    out = []
    for k in range(max(0, k1 - k0)):
        j = in_plane + k * stride
        v = _adjust(buf[j] if j < len(buf) else np.zeros((ny, nx), np.float32), total, nz * plane)
        out.append(v if snr < 0 else orc.poisson_counter_array(v, orc.poisson_mul(snr), S.SEED, STREAM, index0 + k * inc * plane))
    return out


def _restated_tiled_view(orc, case, att, taps, snr, mistake=None):
    first = [_restated_convolve(att, taps, z0, z1, case.inc, mistake) for z0, z1 in case.slabs]
    total = float(np.sum(np.array([f[2] for f in first], np.float64)))
    planes = []
    for (buf, compact, _), (z0, z1) in zip(first, case.slabs):
        planes += _restated_finish(orc, buf, compact, att.shape, z0, z1, case.inc, snr, total, mistake)
    return np.stack(planes) if planes else np.zeros((0,) + att.shape[1:], np.float32)


def _untiled_oracle_view(orc, att, taps, inc, snr):
    raw = orc.convolve_direct(att, np.ascontiguousarray(taps.reshape(-1, 1, 1)).copy())
    orc.adjust_image(raw, S.MIN_VALUE, S.TARGET)
    return raw[::inc].copy() if snr < 0 else orc.extract_slices_counter(raw, inc, snr, S.SEED, STREAM)


def _mistake_applies(mistake, case):
    """The class of cases a planted mistake belongs to: where the code it breaks does anything."""
    halo = _tiling().halo_planes
    slabs = case.slabs
    if mistake in ("halo_short_low", "halo_short_high"):
        return True
    if mistake == "edge_repeating_mirror":
        return any(any(S.folds(case.nz, case.kz, z0, z1)) for z0, z1 in slabs)
    if mistake == "hl_c_swapped":
        return case.kz % 2 == 0
    if mistake in ("in_offset_off_by_one", "rng_offset_from_z0"):
        return any(not S.is_compact(z0, case.inc) and z0 % case.inc != 0 and S.nzo(z0, z1, case.inc) > 0 for z0, z1 in slabs)
    if mistake == "sum_over_halo":
        return any(halo(case.nz, case.kz, z0, z1) != (z0, z1) for z0, z1 in slabs)
    raise AssertionError(mistake)


def test_restated_slab_pipeline_equals_the_untiled_oracle_and_exposes_planted_mistakes(orc):
    caught = {m: [] for m in MISTAKES}
    applies = {m: [] for m in MISTAKES}
    for i, case in enumerate(CASES):
        att, taps = _dyadic_inputs(case, i)
        want = {snr: _untiled_oracle_view(orc, att, taps, case.inc, snr) for snr in (-1.0, 25.0)}
        for snr in (-1.0, 25.0):
            got = _restated_tiled_view(orc, case, att, taps, snr)
            assert got.shape == want[snr].shape and np.array_equal(got.view(np.uint32), want[snr].view(np.uint32)), (case.id, snr)
        for m in MISTAKES:
            if not _mistake_applies(m, case):
                continue
            applies[m].append(case.id)
            snr = 25.0 if m == "rng_offset_from_z0" else -1.0         # (the counters only matter to the sampler)
            if not np.array_equal(_restated_tiled_view(orc, case, att, taps, snr, m), want[snr]):
                caught[m].append(case.id)
    for m in MISTAKES:
        print(f"{m}: caught on {len(caught[m])} of the {len(applies[m])} cases of its class")
        assert applies[m] and caught[m], m
        # dense positive inputs and taps: every case of the class shows it, not just one
        assert caught[m] == applies[m], (m, sorted(set(applies[m]) - set(caught[m])))


# ------------------------------------------------------------------------------------------------ CPU: the misuse guard
class _FakeContext:
    """What TiledView asks of a context, recording the launches; `comm_size` only where given (the gloo worker's context has none)."""

    def __init__(self, **attrs):
        self.launches = []
        for k, v in attrs.items():
            setattr(self, k, v)

    def slab_range(self, nz, nranks, rank):
        return S.slab_range(nz, nranks, rank)

    def _planes(self, params, z0, z1):
        return S.nzo(z0, z1, params.inc)

    def view_slab_dev(self, gt, dim, psf, params, z0, z1, acq, comm_ctx=None):
        self.launches.append(("view_slab_dev", z0, z1, comm_ctx))
        return self._planes(params, z0, z1)

    def view_slab_convolve_dev(self, gt, dim, psf, params, z0, z1):
        self.launches.append(("convolve", z0, z1))
        return 1.5

    def view_slab_finish_dev(self, dim, params, z0, z1, total, acq):
        self.launches.append(("finish", z0, z1, total))
        return self._planes(params, z0, z1)

    def comm_allreduce_sum_f64(self, v):
        return 2 * v


def test_run_on_device_refuses_ranks_without_their_communicator():
    TiledView = _tiling().TiledView
    args = (0, (12, 12, 10), np.ones((3, 3, 3), np.float32), types.SimpleNamespace(inc=2), 0)
    for comm_size in (None, 1, 3):
        c = _FakeContext(comm_size=comm_size)
        with pytest.raises(RuntimeError, match="comm_size"):
            TiledView(c, 1, 2).run_on_device(*args)
        assert c.launches == []                                   # ... before any launch
    bare = _FakeContext()                                         # no comm_size attribute at all: no communicator
    with pytest.raises(RuntimeError, match="comm_size"):
        TiledView(bare, 0, 2).run_on_device(*args)
    assert bare.launches == []
    # the communicator may live in another context (bench.py: comm_ctx=...)
    compute, comm = _FakeContext(), _FakeContext(comm_size=2)
    assert TiledView(compute, 1, 2, comm_ctx=comm).run_on_device(*args)["k1"] == 5
    assert compute.launches == [("view_slab_dev", 5, 10, comm)] and comm.launches == []
    with pytest.raises(RuntimeError, match="comm_size"):
        TiledView(comm, 1, 2, comm_ctx=compute).run_on_device(*args)
    # comm_init(n, r, uid) and then TiledView(c, r, n): the two-process RCCL worker's order
    c = _FakeContext(comm_size=2)
    assert TiledView(c, 0, 2).run_on_device(*args)["planes_owned"] == 5 and c.launches == [("view_slab_dev", 0, 5, None)]
    # one rank reduces nothing and needs no communicator
    c = _FakeContext()
    assert TiledView(c, 0, 1).run_on_device(*args)["k1"] == 5 and c.launches == [("view_slab_dev", 0, 10, None)]
    # run() brings its own reduction or the context's: duck-typed contexts pass as before
    c = _FakeContext()
    info = TiledView(c, 1, 2, allreduce_f64=lambda v: v + 1).run(*args)
    assert info["total"] == 2.5 and c.launches == [("convolve", 5, 10), ("finish", 5, 10, 2.5)]
    c = _FakeContext()
    assert TiledView(c, 0, 2).run(*args)["total"] == 3.0


# ------------------------------------------------------------------------------------------------ GPU
_DEFAULTS = (("fft_zpass", "auto"), ("zconv_strided", 1), ("early_sum", 1), ("exp", 0), ("fused_fftx", "auto"))
_PINNED = {"fft_zpass": "direct", "zconv_strided": 0, "exp": 0, "fused_fftx": "auto"}      # the bit-exact tier (early_sum: the caller's)
CAP = max(c.dim[0] * c.dim[1] * c.dim[2] for c in CASES)


class _Rank:
    """One slab's context ("a GPU per rank", all on device 0) with its copy of the ground truth and two acquisition buffers."""

    def __init__(self, c):
        self.c = c
        c.set_option("fused_rotate", 1)
        self.d_gt, self.d_a, self.d_b = (c.dev_alloc(CAP * 4) for _ in range(3))

    def run(self, n, plane, call, d=None):
        """`call(buffer)` on a buffer filled with the sentinel: (planes it returned, those planes); nothing behind them is touched."""
        d = self.d_a if d is None else d
        self.c.upload(d, np.full(n, SENTINEL, np.float32))
        k = call(d)
        buf = self.c.download(d, (n,))
        assert 0 <= k * plane <= n and np.all(buf[k * plane:] == SENTINEL), k
        return k, buf[:k * plane].reshape(k, plane)

    def close(self):
        for d in (self.d_gt, self.d_a, self.d_b):
            self.c.dev_free(d)
        self.c.close()


@pytest.fixture(scope="module")
def pool(mvs):
    ranks = [_Rank(mvs.Context(0)) for _ in range(max(len(c.slabs) for c in CASES))]
    yield ranks
    for r in ranks:
        r.close()


@pytest.fixture
def options(ctx, pool):
    """Run-time switches of the session context and of every slab context; the defaults are restored afterwards."""
    everyone = [ctx] + [r.c for r in pool]

    def set_(**kw):
        for c in everyone:
            for k, v in kw.items():
                c.set_option(k, v)
    yield set_
    set_(**dict(_DEFAULTS))


_RAW = {}


def _raw(ctx, orc, case):
    """The untiled hand-written convolution of the attenuated view, direct z pass; computed once, read-only."""
    if case.id not in _RAW:
        for k, v in _PINNED.items():
            ctx.set_option(k, v)
        raw = ctx.convolve(_attenuated(orc, case), S.psf_of(case), method=1)
        assert float(raw.max()) > 0 and float(raw.min()) > -1e-6 * float(raw.max())      # non-negative inputs: nothing cancels in a sum
        raw.flags.writeable = False
        _RAW[case.id] = raw
    return _RAW[case.id]


def _params(c, case, snr, inc=None):
    return c.view_params(degrees=case.degrees, delta=S.DELTA, min_value=S.MIN_VALUE, target_average=S.TARGET,
                         inc=case.inc if inc is None else inc, snr=snr, seed=S.SEED, stream=STREAM, conv_method=1)


def _want(orc, raw, total, inc, snr):
    adj = _adjust(raw, total, raw.size)
    return np.ascontiguousarray(adj[::inc]) if snr < 0 else orc.extract_slices_counter(adj, inc, snr, S.SEED, STREAM)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _convolve_slabs(pool, case, gt, fused=None):
    """Every slab through mvsim_view_slab_convolve_dev in a context of its own: the slab sums."""
    sums = []
    for rk, (z0, z1) in zip(pool, case.slabs):
        rk.c.upload(rk.d_gt, gt)
        if fused is not None:
            rk.c.enable_timing(True)
        sums.append(rk.c.view_slab_convolve_dev(rk.d_gt, case.dim, S.psf_of(case), _params(rk.c, case, 25.0), z0, z1))
        if fused is not None:
            # the fused rotate + attenuate + x transform really ran (or did not): it does pass A's work itself
            t = rk.c.timings()
            rk.c.enable_timing(False)
            assert t["rotate_ms"] > 0 and (t["pass_a_ms"] == 0) == (fused == 1), (fused, t)
    return sums


def _check_sums(orc, case, raw, sums, limit_of):
    """Each slab sum against the fp64 host sum of the untiled planes; returns the largest difference relative to the whole sum."""
    whole = float(np.sum(raw, dtype=np.float64))
    zero = _zero_slabs(orc, case)
    worst = 0.0
    for (z0, z1), s in zip(case.slabs, sums):
        ref = float(np.sum(raw[z0:z1], dtype=np.float64))
        diff = abs(s - ref) / whole
        worst = max(worst, diff)
        print(f"slab sum {case.id} [{z0},{z1}): {s!r} against {ref!r}, {diff:.3e} of the view's")
        if (z0, z1) in zero:
            assert s == 0.0 and ref == 0.0, (z0, z1, s, ref)
        assert diff <= limit_of(z0), (z0, z1, s, ref, diff)
    return worst


def _sweep_bit_exact(ctx, orc, pool, case, early, fused):
    gt, psf, raw = S.ground_truth(case), S.psf_of(case), _raw(ctx, orc, case)
    nz, ny, nx = case.shape
    plane, n = ny * nx, nz * ny * nx
    slabs = case.slabs
    sums = _convolve_slabs(pool, case, gt, fused)
    worst = _check_sums(orc, case, raw, sums, lambda z0: EARLY1_SUM_LIMIT if early else EARLY0_SUM_LIMIT)
    total = float(np.sum(np.array(sums, dtype=np.float64)))             # what the all-reduce delivers
    spans = [(len(a), a[0] if a else None) for a in (S.acquired(z0, z1, case.inc) for z0, z1 in slabs)]
    assert sum(k for k, _ in spans) == S.extract_nz(nz, case.inc)
    out = {}
    for snr in S.SNRS:
        want = _want(orc, raw, total, case.inc, snr).reshape(-1, plane)
        assert want.shape[0] == S.extract_nz(nz, case.inc) and (snr < 0 or np.all(want == np.round(want)))
        parts = []
        for rk, (z0, z1), own, (count, k0) in zip(pool, slabs, sums, spans):
            p = _params(rk.c, case, snr)
            k, got = rk.run(n, plane, lambda d: rk.c.view_slab_finish_dev(case.dim, p, z0, z1, total, d))
            assert k == count, (z0, z1, k, count)                        # (0 planes: nothing written, see _Rank.run)
            if count:
                assert _same_bits(got, want[k0:k0 + count]), (snr, z0, z1, float(np.max(np.abs(got - want[k0:k0 + count]))))
            parts.append(got)
            # the same slab in ONE call, on a context without a communicator: the three-step form with the slab's own sum as the total
            if own == 0.0 and snr >= 0:
                continue                                                  # (0 / 0: see the module's docstring)
            ka, three = rk.run(n, plane, lambda d: rk.c.view_slab_finish_dev(case.dim, p, z0, z1, own, d))
            kb, one = rk.run(n, plane, lambda d: rk.c.view_slab_dev(rk.d_gt, case.dim, psf.copy(), p, z0, z1, d), rk.d_b)
            assert ka == kb == count and _same_bits(one, three), (snr, z0, z1)
        out[snr] = np.concatenate(parts, axis=0)
        assert _same_bits(out[snr], want)
    # a slab without an acquired plane leaves its context usable: the case's first slab on it
    p = _params(ctx, case, 25.0)
    want = _want(orc, raw, total, case.inc, 25.0).reshape(-1, plane)
    for rk, (count, _) in zip(pool, spans):
        if count == 0:
            z0, z1 = slabs[0]
            assert rk.c.view_slab_convolve_dev(rk.d_gt, case.dim, psf.copy(), p, z0, z1) == sums[0]
            k, got = rk.run(n, plane, lambda d: rk.c.view_slab_finish_dev(case.dim, p, z0, z1, total, d))
            assert k == spans[0][0] and _same_bits(got, want[:k])
    return out, worst


@pytest.mark.gpu
@pytest.mark.parametrize("early", (1, 0), ids=("early_sum1", "early_sum0"))
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_every_slab_equals_the_untiled_view_bit_for_bit(ctx, orc, pool, options, case, early):
    _raw(ctx, orc, case)
    res = {}
    for fused in ((0, 1) if case.fused_eligible else (None,)):
        options(early_sum=early, **dict(_PINNED, fused_fftx="auto" if fused is None else fused))
        res[fused], worst = _sweep_bit_exact(ctx, orc, pool, case, early, fused)
        print(f"largest slab sum difference {case.id} early_sum={early}: {worst:.3e}")
    if case.fused_eligible:
        for snr in S.SNRS:
            assert _same_bits(res[0][snr], res[1][snr]), snr


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if _tier3(c)], ids=lambda c: c.id)
def test_slabs_under_default_options(ctx, orc, pool, options, case):
    """Default options plus exp=2 (the strided z pass wherever its geometry allows, as test_strided_z_pass_of_compact_views forces it):
    compact slabs to that test's limits, non-compact slabs -- they never take a z stride -- bit for bit."""
    gt, raw = S.ground_truth(case), _raw(ctx, orc, case)
    options(**dict(_DEFAULTS, exp=2))
    nz, ny, nx = case.shape
    plane, n = ny * nx, nz * ny * nx
    sums = _convolve_slabs(pool, case, gt)
    _check_sums(orc, case, raw, sums, lambda z0: STRIDED_SUM_LIMIT if S.is_compact(z0, case.inc) else EARLY1_SUM_LIMIT)
    total = float(np.sum(np.array(sums, dtype=np.float64)))
    for snr in S.SNRS:
        want = _want(orc, raw, total, case.inc, snr).reshape(-1, plane)
        differ = counts = 0
        for rk, (z0, z1) in zip(pool, case.slabs):
            a = S.acquired(z0, z1, case.inc)
            p = _params(rk.c, case, snr)
            k, got = rk.run(n, plane, lambda d: rk.c.view_slab_finish_dev(case.dim, p, z0, z1, total, d))
            assert k == len(a)
            if not a:
                continue
            ref = want[a[0]:a[0] + k]
            if not S.is_compact(z0, case.inc):
                assert _same_bits(got, ref), (snr, z0, z1)
            elif snr < 0:
                err = float(np.max(np.abs(got - ref)))
                print(f"compact slab {case.id} [{z0},{z1}): max |got - want| = {err:.3e}, {err / float(want.max()):.3e} of the maximum")
                assert err <= STRIDED_PLANE_LIMIT * float(want.max()), (z0, z1, err)
            else:
                assert np.all(got == np.round(got))
                differ += int((got != ref).sum())
                counts += got.size
        if counts:
            print(f"compact slabs {case.id} snr {snr}: {differ} of {counts} counts differ")
            assert differ < STRIDED_COUNT_LIMIT * counts, (snr, differ, counts)


# one small view for the error paths and the guard: slab [4, 9) of ten planes, compact at inc 2
GOOD = S.Case("good", (12, 14, 10), (3, 3, 3), 2, (0, 4, 9, 10))
ERRORS = ("finish_without_convolve", "finish_other_range", "finish_other_inc", "z1_past_nz", "z0_negative", "kz65", "nx_gt_ny", "fft_zpass_partial")


def _good_slab_runs(ctx, orc, d_gt, d_acq, z0=4, z1=9):
    """Slab [z0, z1) of GOOD on `ctx`, finished with the untiled sum as the total: the planes of the untiled view, bit for bit."""
    raw = _raw(ctx, orc, GOOD)
    total = float(np.sum(raw, dtype=np.float64))
    p = _params(ctx, GOOD, 25.0)
    ctx.view_slab_convolve_dev(d_gt, GOOD.dim, S.psf_of(GOOD), p, z0, z1)
    a = S.acquired(z0, z1, GOOD.inc)
    assert ctx.view_slab_finish_dev(GOOD.dim, p, z0, z1, total, d_acq) == len(a)
    got = ctx.download(d_acq, (len(a),) + GOOD.shape[1:])
    assert _same_bits(got, _want(orc, raw, total, GOOD.inc, 25.0)[a[0]:a[0] + len(a)])


@pytest.fixture
def good(ctx, orc, options):
    _raw(ctx, orc, GOOD)
    options(early_sum=1, **_PINNED)
    d_gt, d_acq = ctx.dev_alloc(CAP * 4), ctx.dev_alloc(CAP * 4)
    ctx.upload(d_gt, S.ground_truth(GOOD))
    ctx.upload(d_acq, np.full(CAP, SENTINEL, np.float32))
    yield types.SimpleNamespace(d_gt=d_gt, d_acq=d_acq)
    ctx.dev_free(d_gt)
    ctx.dev_free(d_acq)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ERRORS)
def test_slab_entry_points_reject_and_recover(mvs, ctx, orc, options, good, what):
    dim, psf, p = GOOD.dim, S.psf_of(GOOD), _params(ctx, GOOD, 25.0)
    d_gt, d_acq = good.d_gt, good.d_acq
    total = float(np.sum(_raw(ctx, orc, GOOD), dtype=np.float64))
    with pytest.raises(ValueError):
        if what == "finish_without_convolve":
            with mvs.Context(0) as fresh:
                fresh.view_slab_finish_dev(dim, p, 4, 9, total, d_acq)
        elif what == "finish_other_range":
            ctx.view_slab_convolve_dev(d_gt, dim, psf, p, 4, 9)
            ctx.view_slab_finish_dev(dim, p, 4, 8, total, d_acq)
        elif what == "finish_other_inc":
            ctx.view_slab_convolve_dev(d_gt, dim, psf, p, 4, 9)              # compact: the planes 4, 6, 8 alone
            ctx.view_slab_finish_dev(dim, _params(ctx, GOOD, 25.0, inc=3), 4, 9, total, d_acq)
        elif what == "z1_past_nz":
            ctx.view_slab_convolve_dev(d_gt, dim, psf, p, 4, 11)
        elif what == "z0_negative":
            ctx.view_slab_convolve_dev(d_gt, dim, psf, p, -1, 9)
        elif what == "kz65":
            ctx.view_slab_convolve_dev(d_gt, dim, np.ones((65, 3, 3), np.float32), p, 4, 9)
        elif what == "nx_gt_ny":
            ctx.view_slab_convolve_dev(d_gt, (14, 12, 10), psf, p, 4, 9)
        elif what == "fft_zpass_partial":
            options(fft_zpass="fft")
            ctx.view_slab_convolve_dev(d_gt, dim, psf, p, 4, 9)
    assert np.all(ctx.download(d_acq, (CAP,)) == SENTINEL)                   # nothing was written
    if what in ("z1_past_nz", "z0_negative"):
        with pytest.raises(ValueError):                                      # the second call checks its range as well
            ctx.view_slab_finish_dev(dim, p, *((4, 11) if what == "z1_past_nz" else (-1, 9)), total, d_acq)
    options(fft_zpass="direct")
    _good_slab_runs(ctx, orc, d_gt, d_acq)


@pytest.mark.gpu
def test_run_on_device_guard_on_a_real_context(ctx, orc, options, good):
    TiledView = _tiling().TiledView
    assert ctx.comm_size is None
    p = _params(ctx, GOOD, 25.0)
    with pytest.raises(RuntimeError, match="comm_size"):
        TiledView(ctx, 0, 2).run_on_device(good.d_gt, GOOD.dim, S.psf_of(GOOD), p, good.d_acq)
    assert np.all(ctx.download(good.d_acq, (CAP,)) == SENTINEL)
    # one rank: the whole view as its slab, adjusted with its own sum
    info = TiledView(ctx, 0, 1).run_on_device(good.d_gt, GOOD.dim, S.psf_of(GOOD), p, good.d_acq)
    assert (info["z0"], info["z1"], info["k1"]) == (0, GOOD.nz, S.extract_nz(GOOD.nz, GOOD.inc))
    got = ctx.download(good.d_acq, (info["k1"],) + GOOD.shape[1:])
    own = ctx.view_slab_convolve_dev(good.d_gt, GOOD.dim, S.psf_of(GOOD), p, 0, GOOD.nz)
    assert _same_bits(got, _want(orc, _raw(ctx, orc, GOOD), own, GOOD.inc, 25.0))
