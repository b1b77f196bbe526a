"""Extract + Poisson swept over its sampler forms (tests/poisson_sweep_cases.py): the four kernels of launch_extract (extract.hip) with and
without the fused adjust, the queue kernels with full segments and with segments that refuse (refused walks 1 and 2), the fused tail, the
stacked-view table forms; queue shares 16, 1, auto and off; planes of 4 .. 4096 voxels, spacings 1, 2, 3, 7; counters that cross
2^32, 2^33, 2^34 and 2^63 inside one wave; Philox keys with a non-zero high word and streams up to 2^32 - 1.

Every GPU case first asserts, through mvsim_extract_path (or mvsim_fused_tail_geometry), that it lands on the form it claims, then
that its counts EQUAL the oracle's counter sampler on the lambda the sampler read: the input itself for poisson_process and
extractSlices, the noise-free twin of the same call (snr < 0) for views and slabs.  The CPU tests hold the case list to the library's
path decision and the plan header (csrc/extract_plan.h, in a program of its own) to both, check that the list covers every form and
counter range, and that its lambda mix would expose the classic counter mistakes."""
import ctypes as C
import importlib
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from . import poisson_sweep_cases as S

SEED = S.SEED
REF_DELTA = float(np.float32(0.01))


def _i64(vals):
    return (C.c_int64 * len(vals))(*vals)


def _path(mvs, dim, inc, index_inc, offset, aligned16, share):
    """mvsim_extract_path: (kernel, segments can refuse, blocks, items per segment)."""
    p = _i64([0] * 4)
    rc = mvs._lib.load().mvsim_extract_path(_i64(dim), inc, index_inc, offset, aligned16, share, p)
    assert rc == 0, (dim, inc, index_inc, offset, share)
    return tuple(p)


def _mix_of(case):
    """The case's lambda mix (poisson / extract cases): values v, lambda = (double) v * mul."""
    n = int(np.prod(case.shape))
    return S.lambda_mix(n, S.mul_of(case), zlib.crc32(case.id.encode()), exact_ten=case.entry == "poisson").reshape(case.shape)


def _oracle_planes(orc, lam_planes, mul, seed, stream, counters):
    """The oracle's counts of every plane, plane k's voxel i on counter counters[k] + i."""
    return np.stack([orc.poisson_counter_array(p, mul, seed, stream, c) for p, c in zip(lam_planes, counters)])


def _assert_counts(got, lam_planes, want, mul, counters, what):
    if np.array_equal(got, want, equal_nan=True):
        return
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))).reshape(-1))
    k, i = (int(t) for t in np.unravel_index(bad[0], (want.shape[0], int(np.prod(want.shape[1:])))))
    v = float(lam_planes.reshape(want.shape[0], -1)[k, i])
    raise AssertionError(f"{what}: {bad.size} of {want.size} counts differ; first at plane {k} voxel {i}: lambda {v * mul!r}, "
                         f"counter {counters[k] + i} ({(counters[k] + i) % 2 ** 64:#x}), got {got.reshape(want.shape[0], -1)[k, i]!r}, "
                         f"oracle {want.reshape(want.shape[0], -1)[k, i]!r}")


# ------------------------------------------------------------------------------------------------ CPU: path, coverage, yardstick
def test_case_ids_are_unique_and_the_list_deterministic():
    ids = [c.id for c in S.CASES]
    assert len(ids) == len(set(ids))
    assert [c.id for c in importlib.reload(S).CASES] == ids
    for c in S.CASES:
        assert S.acquired(c.shape[0], c.inc) >= 3 or c.entry == "poisson", c.id
        assert int(np.prod(c.shape)) <= 1 << 20, c.id


def test_path_query_agrees_with_the_case_list(mvs):
    for c in S.CASES:
        if c.claim == S.FUSED:
            continue
        args = S.launch_args(c)
        k, r, blocks, items = _path(mvs, *args)
        assert (k, bool(r)) == S.expect_path(*args) == (c.claim, c.refuses), c.id
        assert blocks >= 1 and (items > 0) == (k in (S.K_NOISE2, S.K_NOISE2_ANY)), c.id


def test_path_query_at_the_size_guards(mvs):
    # N' >= 2^32: work items carry the output position in 32 bits -> the queue-less kernel
    assert _path(mvs, (2048, 2048, 1024), 1, 0, 0, 1, 16)[0] == S.K_VEC
    assert _path(mvs, (2048, 2048, 1023), 1, 0, 0, 1, 16)[0] == S.K_NOISE2
    assert _path(mvs, (2048, 2048, 2047), 2, 0, 0, 1, 16)[0] == S.K_VEC          # N' = 1024 planes
    # (index_inc - 1) * plane >= 2^31: a compact 2048 x 2048 x 520 view at inc 516 (two acquired planes)
    assert _path(mvs, (2048, 2048, 2), 1, 516, 0, 1, 16)[0] == S.K_VEC
    assert _path(mvs, (2048, 2048, 2), 1, 512, 0, 1, 16)[0] == S.K_NOISE2
    assert _path(mvs, (2048, 2048, 520), 516, 0, 0, 0, 16)[0] == S.K_SCALAR
    # a vector slot of 256 outputs crosses up to ceil(255 / plane) plane boundaries: at plane 4 and index_inc 2^27, 64 jumps of
    # ~2^29 counters -- one jump alone would pass a single-boundary guard
    assert (2 ** 27 - 1) * 4 < 2 ** 31
    assert _path(mvs, (4, 1, 1000), 1, 2 ** 27, 0, 1, 16)[0] == S.K_VEC
    assert _path(mvs, (4, 1, 1000), 1, 2 ** 22, 0, 1, 16)[0] == S.K_NOISE2
    # jumps of 2^30 counters: two per slot at planes of 128 voxels, one at 256
    assert _path(mvs, (128, 1, 1000), 1, 2 ** 23 + 1, 0, 1, 16)[0] == S.K_VEC
    assert _path(mvs, (256, 1, 1000), 1, 2 ** 22 + 1, 0, 1, 16)[0] == S.K_NOISE2
    # the production volumes keep the queue kernels: the bench's 512^3 at inc 1, configs[4] at inc 3 (compact)
    assert _path(mvs, (512, 512, 512), 1, 0, 0, 1, 16)[:2] == (S.K_NOISE2, 0)
    assert _path(mvs, (512, 512, 512), 1, 0, 0, 1, 5)[:2] == (S.K_NOISE2, 1)
    assert _path(mvs, (2048, 2048, 171), 1, 3, 0, 1, 5)[:2] == (S.K_NOISE2, 1)
    assert _path(mvs, (2048, 2048, 512), 3, 0, 0, 1, 16)[:2] == (S.K_NOISE2, 0)
    for args in (((2048, 2048, 2), 1, 516, 0, 1, 16), ((4, 1, 1000), 1, 2 ** 27, 0, 1, 16), ((2048, 2048, 1024), 1, 0, 0, 1, 16)):
        assert _path(mvs, *args)[0] == S.expect_path(*args)[0]


def _geom_of(args):
    """launch_args' (dim, inc, index_inc, offset, ..) as ExtractGeom states it: (plane, acquired planes, inc, index_inc, index_offset)."""
    dim, inc, index_inc, offset = args[:4]
    return dim[0] * dim[1], S.acquired(dim[2], inc), inc, index_inc or inc, offset


def _plan_request(c):
    """The ExtractGeom constructor the case's entry point calls (api.cpp, api_host.cpp, api_view.cpp), as a request of extract_plan_main."""
    nz, ny, nx = c.shape
    _, _, _, offset, aligned16, share = S.launch_args(c)
    kind, a, b, k = "strided", 0, 0, 0
    if c.entry == "poisson":
        kind, (nx, ny, nz), b = "path", (c.shape[2], 1, 1), offset
    elif c.entry in ("view", "views") and c.inc > 1 and c.queue != "off":
        kind = "compact"
    elif c.entry in ("slab3", "slab_dev"):
        kind, (a, b), k = "slab", c.slab, int(S.slab_planes(c)[2])
    return f"{kind} {nx} {ny} {nz} {c.inc} {a} {b} {k} {aligned16} 1 {share}"


# test_path_query_at_the_size_guards' inputs and the kernels it expects of them
_GUARD_INPUTS = (
    (((2048, 2048, 1024), 1, 0, 0, 1, 16), S.K_VEC), (((2048, 2048, 1023), 1, 0, 0, 1, 16), S.K_NOISE2),
    (((2048, 2048, 2047), 2, 0, 0, 1, 16), S.K_VEC), (((2048, 2048, 2), 1, 516, 0, 1, 16), S.K_VEC),
    (((2048, 2048, 2), 1, 512, 0, 1, 16), S.K_NOISE2), (((2048, 2048, 520), 516, 0, 0, 0, 16), S.K_SCALAR),
    (((4, 1, 1000), 1, 2 ** 27, 0, 1, 16), S.K_VEC), (((4, 1, 1000), 1, 2 ** 22, 0, 1, 16), S.K_NOISE2),
    (((128, 1, 1000), 1, 2 ** 23 + 1, 0, 1, 16), S.K_VEC), (((256, 1, 1000), 1, 2 ** 22 + 1, 0, 1, 16), S.K_NOISE2),
    (((512, 512, 512), 1, 0, 0, 1, 16), (S.K_NOISE2, 0)), (((512, 512, 512), 1, 0, 0, 1, 5), (S.K_NOISE2, 1)),
    (((2048, 2048, 171), 1, 3, 0, 1, 5), (S.K_NOISE2, 1)), (((2048, 2048, 512), 3, 0, 0, 1, 16), (S.K_NOISE2, 0)),
)


def test_plan_header_agrees_with_the_case_list_and_the_library(mvs, tmp_path):
    """tests/c_abi/extract_plan_main.cpp: csrc/extract_plan.h compiled by plain g++ under ASan + UBSan (no HIP, no libmvsim.so; a child
    process, nothing preloaded).  (a) every non-fused case through the constructor its entry point calls: the geometry is launch_args',
    the kernel and the refusing flag expect_path's, blocks and items per segment mvsim_extract_path's; (b) the size guards; (c)
    ExtractGeom::slab over planes of 4, 60 and 257 voxels, nz 1..24, inc 1, 2, 3, 7, every 0 <= z0 < z1 <= nz, strided and -- where z0
    is a multiple of inc -- compact: slab_planes' and launch_args' geometry, empty slabs included.  No mismatch, no sanitizer report."""
    exe = str(tmp_path / "extract_plan_main")
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
           "-Wextra", "-Werror", "-I" + os.path.join(os.path.dirname(os.path.abspath(mvs.__file__)), "csrc"),
           os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_abi", "extract_plan_main.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    cases = [c for c in S.CASES if c.claim != S.FUSED]
    slabs = []
    for ny, nx in ((1, 4), (6, 10), (1, 257)):
        for nz in range(1, 25):
            for inc in S.INCS:
                for z0 in range(nz):
                    for z1 in range(z0 + 1, nz + 1):
                        for compact in (0, 1) if z0 % inc == 0 else (0,):
                            slabs.append((S.Case("grid", "slab3", (nz, ny, nx), inc=inc, slab=(z0, z1)), compact))
    requests = [_plan_request(c) for c in cases]
    requests += [f"path {d[0]} {d[1]} {d[2]} {inc} {iinc} {off} 0 {al} 1 {share}" for (d, inc, iinc, off, al, share), _ in _GUARD_INPUTS]
    requests += [f"slab {c.shape[2]} {c.shape[1]} {c.shape[0]} {c.inc} {c.slab[0]} {c.slab[1]} {k} 1 1 16" for c, k in slabs]
    r = subprocess.run([exe], input="\n".join(requests) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and f"extract plan run ok: {len(requests)} requests" in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]
    rows = [tuple(int(t) for t in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == len(requests)
    mismatches = []
    for c, row in zip(cases, rows):
        args = S.launch_args(c)
        ok = row[:5] == _geom_of(args) and (row[6], bool(row[7])) == S.expect_path(*args) == (c.claim, c.refuses)
        ok = ok and row[8:10] == _path(mvs, *args)[2:4] and row[12] == args[5]
        if c.entry in ("slab3", "slab_dev"):
            first, _, compact = S.slab_planes(c)
            ok = ok and row[5] == (0 if compact else c.plane * (first - c.slab[0])) and (row[5] % 4 == 0) == bool(args[4])
        else:
            ok = ok and row[5] == 0
        if not ok:
            mismatches.append((c.id, row))
    rows = rows[len(cases):]
    for (args, want), row in zip(_GUARD_INPUTS, rows):
        got = (row[6], row[7], row[8], row[9])
        if got != _path(mvs, *args) or (got[:2] != want if isinstance(want, tuple) else got[0] != want) or row[:5] != _geom_of(args):
            mismatches.append((args, row))
    rows = rows[len(_GUARD_INPUTS):]
    n_empty = 0
    for (c, k), row in zip(slabs, rows):
        (z0, z1), plane = c.slab, c.plane
        first, n_acq, compact = S.slab_planes(c)
        ok = n_acq == sum(1 for j in range(c.shape[0] + 1) if z0 <= j * c.inc < z1) and first % c.inc == 0 and (n_acq == 0 or z0 <= first < z1)
        ok = ok and row[:6] == (plane, n_acq, 1 if k else c.inc, c.inc, first * plane, 0 if k else plane * (first - z0))
        if bool(k) == compact:
            ok = ok and row[:5] == _geom_of(S.launch_args(c))
        n_empty += n_acq == 0
        if not ok:
            mismatches.append((c.shape, c.inc, c.slab, k, row))
    assert n_empty > 0 and not mismatches, (len(mismatches), mismatches[:5])


def test_sweep_covers_every_form_and_counter_range():
    inst = {(c.claim, c.adjust, c.refuses, c.entry == "views") for c in S.CASES}
    for k in (S.K_SCALAR, S.K_VEC):
        for adj in (False, True):
            assert (k, adj, False, False) in inst, (k, adj)
    for k in (S.K_NOISE2, S.K_NOISE2_ANY):
        for adj in (False, True):
            for ref in (False, True):
                assert (k, adj, ref, False) in inst, (k, adj, ref)        # refused walks 1 (vector) and 2 (group by group)
        assert (k, True, False, True) in inst and (k, True, True, True) in inst, k      # the stacked table forms
    assert any(c.claim == S.FUSED for c in S.CASES)
    assert {c.entry for c in S.CASES} == set(S.ENTRIES)
    for e in ("slab3", "slab_dev"):
        assert {S.slab_planes(c)[2] for c in S.CASES if c.entry == e} == {True, False}, e     # z0 % inc == 0 and != 0
    assert {c.queue for c in S.CASES} == set(S.QUEUES)
    assert {c.queue for c in S.CASES if c.entry in S.VIEW_ENTRIES} == set(S.QUEUES)
    assert {c.seed for c in S.CASES} == set(S.KEYS)
    assert {c.stream for c in S.CASES} == set(S.STREAMS)
    assert {c.plane for c in S.CASES if c.entry != "poisson"} >= {ny * nx for ny, nx in S.PLANES}
    assert {c.inc for c in S.CASES} >= set(S.INCS)
    assert {c.offset % 4 for c in S.CASES if c.entry == "poisson"} == {0, 1, 2, 3}
    assert any(c.offset == 0 for c in S.CASES if c.entry == "poisson")
    # every boundary inside one wave slot (256 counters from the slot's first) in the vector and the group-by-group form, queue on and off
    for b in S.BOUNDARIES:
        seen = set()
        for c in S.CASES:
            if c.entry == "poisson" and c.offset < b < c.offset + min(256, c.shape[2]):
                seen.add((c.claim in (S.K_VEC, S.K_NOISE2), c.queue != "off"))
        assert seen == {(True, True), (True, False), (False, True), (False, False)}, (b, seen)


def _mistakes(c):
    """(name, plane counters) under each mistake the yardstick applies, or None where the mistake is the identity."""
    plane = c.plane if c.entry != "poisson" else c.shape[2]
    base = [c.offset] if c.entry == "poisson" else S.counters_of(c)
    out = [("counter+1", [b + 1 for b in base], c.seed, c.stream), ("counter-1", [b - 1 for b in base], c.seed, c.stream),
           ("counter+4", [b + 4 for b in base], c.seed, c.stream), ("one plane", [b + plane for b in base], c.seed, c.stream),
           ("stream+1", base, c.seed, (c.stream + 1) & 0xFFFFFFFF)]
    if c.inc > 1 and len(base) > 1:
        out.append(("k(inc-1) planes", [b - k * (c.inc - 1) * plane for k, b in enumerate(base)], c.seed, c.stream))
    if c.seed >> 32:
        out.append(("key high word", base, c.seed & 0xFFFFFFFF, c.stream))
    return base, out


def test_lambda_mix_exposes_counter_mistakes(orc):
    n_inc = n_key = 0
    for c in S.CASES:
        if c.entry not in ("poisson", "extract", "extract_dev"):
            continue
        v = _mix_of(c)
        mul = S.mul_of(c)
        planes = v.reshape(1, -1) if c.entry == "poisson" else v[::c.inc][:S.acquired(c.shape[0], c.inc)]
        base, mistakes = _mistakes(c)
        want = _oracle_planes(orc, planes, mul, c.seed, c.stream, base)
        for name, counters, seed, stream in mistakes:
            alt = _oracle_planes(orc, planes, mul, seed, stream, counters)
            diff = int((alt != want).sum())
            assert diff >= 100 and diff >= 0.01 * want.size, (c.id, name, diff, want.size)
            n_inc += name == "k(inc-1) planes"
            n_key += name == "key high word"
        lam = planes.astype(np.float64) * mul
        assert np.nanmax(lam) > 1e9 and (lam[np.isfinite(lam)] < 10).mean() > 0.3, c.id   # both regimes, and the unsqueezed run
    assert n_inc >= 5 and n_key >= 10


def test_oracle_array_is_the_scalar_counter(orc):
    v = S.lambda_mix(4096, 1.0, 3, exact_ten=True)
    for seed, stream, off in ((SEED, 0, 0), (S.SEED_BOTH, 5, 2 ** 33 - 7), (S.SEED_MAX, 2 ** 32 - 1, 2 ** 64 - 100)):
        got = orc.poisson_counter_array(v, 1.0, seed, stream, off)
        idx = np.arange(0, 4096, 37)
        want = [orc.poisson_counter(float(v[i]), seed, stream, (off + int(i)) % 2 ** 64) for i in idx]
        assert got[idx].tolist() == [float(np.float32(w)) for w in want]


# ------------------------------------------------------------------------------------------------ GPU
_CTX = {}


def _ctx(mvs, queue, fuse=False):
    key = (queue, fuse)
    if key not in _CTX:
        c = mvs.Context(0)
        c.set_option("fused_rotate", 1)
        c.set_option("poisson_queue", 0 if queue == "off" else 1)
        if queue != "off":
            c.set_option("poisson_queue_share", queue)
        c.set_option("fuse_tail", 1 if fuse else 0)
        _CTX[key] = c
    return _CTX[key]


@pytest.fixture(scope="module")
def contexts():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def _phantom(shape, seed):
    """Dark background with bright blobs: after adjustImage both regimes of the sampler are populated."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    v = np.full(shape, 0.02, np.float32)
    for _ in range(10):
        cz, cy, cx = rng.uniform(0, nz), rng.uniform(0, ny), rng.uniform(0, nx)
        r = rng.uniform(3, 8)
        v += (rng.uniform(1, 6) * np.exp(-((z - cz) ** 2 + (y - cy) ** 2 + (x - cx) ** 2) / (2 * r * r))).astype(np.float32)
    return v


_KDIM = (5, 5, 7)     # x, y, z taps of the views' PSF


def _psf(synth):
    return synth.gaussian_psf(*_KDIM, sigma=(1.1, 1.3, 1.8))


def _check_path(mvs, c):
    if c.claim == S.FUSED:
        return
    got = _path(mvs, *S.launch_args(c))
    assert (got[0], bool(got[1])) == (c.claim, c.refuses), (c.id, got)


def _recorded(mvs, ctx):
    """mvsim_get_extract_path: the form of the context's last extract (kernel, can refuse, blocks, items per segment, views)."""
    p = _i64([0] * 5)
    assert mvs._lib.load().mvsim_get_extract_path(ctx._h, p) == 0
    return tuple(p)


def _took(mvs, ctx, c):
    """The noisy call just made took the form the case claims (as the library recorded it), and its refusing segments refused."""
    got = _recorded(mvs, ctx)
    assert (got[0], bool(got[1])) == (c.claim, c.refuses), (c.id, got)
    assert got[4] == (c.views if c.entry == "views" else 1), (c.id, got)       # views > 1: the stacked ExtractView tables ran
    if c.claim == S.FUSED:
        # the convolution's last pass sampled (the view was not handed to launch_extract), with the geometry the library reports
        nz, ny, nx = c.shape
        g = _i64([0, 0])
        assert mvs._lib.load().mvsim_fused_tail_geometry(ctx._h, _i64((nx, ny, nz)), _i64(_KDIM), c.inc, 0, g) == 0, c.id
        assert got[2:4] == (g[0], g[1]) and g[0] >= 1 and g[1] >= nx, (c.id, got)
    else:
        assert got[2:4] == _path(mvs, *S.launch_args(c))[2:4], (c.id, got)
    if c.refuses:
        assert ctx.queue_stats()["refused"] > 0, c.id


def _view_params(ctx, c, snr, v=0):
    seed = c.seed if v == 0 else (c.seed ^ (0x1234567800000001 * v)) & 0xFFFFFFFFFFFFFFFF
    stream = c.stream if v == 0 else (c.stream + 7 * v) & 0xFFFFFFFF
    return ctx.view_params(degrees=30 + 25 * v, delta=REF_DELTA, inc=c.inc, snr=snr, seed=seed, stream=stream, conv_method=1), seed, stream


def _run_view(mvs, synth, c):
    """(list of (counts, lambda planes, seed, stream, plane counters)) of a view / slab case: counts of the noisy call, lambda of its
    noise-free twin."""
    ctx = _ctx(mvs, c.queue, fuse=c.entry == "view_fused")
    nz, ny, nx = c.shape
    gt = _phantom(c.shape, zlib.crc32(c.id.encode()))
    psf = _psf(synth)
    out = []
    if c.entry in ("view", "view_con", "view_fused"):
        want = ("con", "acq") if c.entry == "view_con" else ("acq",)
        p, seed, stream = _view_params(ctx, c, S.SNR)
        pn, _, _ = _view_params(ctx, c, -1.0)
        counts = ctx.simulate_view(gt, psf.copy(), p, want=want)["acq"]
        _took(mvs, ctx, c)
        lam = ctx.simulate_view(gt, psf.copy(), pn, want=want)["acq"]
        if c.entry == "view" and c.queue == "off" and c.inc > 1:
            # the noisy call convolves every plane (no queue: no compact planes), its noise-free twin only the acquired ones
            full = ctx.simulate_view(gt, psf.copy(), pn, want=("con", "acq"))
            assert np.array_equal(full["con"][::c.inc], lam) and np.array_equal(full["acq"], lam), c.id
        out.append((counts, lam, seed, stream, S.counters_of(c)))
    elif c.entry == "views":
        ps = [_view_params(ctx, c, S.SNR, v) for v in range(c.views)]
        pn = [_view_params(ctx, c, -1.0, v)[0] for v in range(c.views)]
        counts = ctx.simulate_views(gt, [psf.copy() for _ in ps], [p for p, _, _ in ps])
        _took(mvs, ctx, c)
        lams = ctx.simulate_views(gt, [psf.copy() for _ in ps], pn)
        for (p, seed, stream), a, lam in zip(ps, counts, lams):
            out.append((a, lam, seed, stream, S.counters_of(c)))
    else:
        dims = (nx, ny, nz)
        z0, z1 = c.slab
        _, n_acq, _ = S.slab_planes(c)
        d_gt = ctx.dev_alloc(gt.nbytes)
        d_acq = ctx.dev_alloc(max(1, n_acq) * ny * nx * 4)
        try:
            ctx.upload(d_gt, gt)
            res = []
            for snr in (S.SNR, -1.0):
                p, seed, stream = _view_params(ctx, c, snr)
                if c.entry == "slab3":
                    own = ctx.view_slab_convolve_dev(d_gt, dims, psf.copy(), p, z0, z1)
                    k = ctx.view_slab_finish_dev(dims, p, z0, z1, own, d_acq)
                else:
                    k = ctx.view_slab_dev(d_gt, dims, psf.copy(), p, z0, z1, d_acq)
                ctx.synchronize()
                assert k == n_acq
                if snr > 0:
                    _took(mvs, ctx, c)
                res.append(ctx.download(d_acq, (k, ny, nx)))
            out.append((res[0], res[1], seed, stream, S.counters_of(c)))
        finally:
            ctx.dev_free(d_gt)
            ctx.dev_free(d_acq)
    for _, lam, _, _, _ in out:
        lam64 = lam.astype(np.float64) * S.mul_of(c)
        assert lam64.max() > 50 and lam64.min() < 10, c.id                               # both regimes of the sampler
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", S.CASES, ids=[c.id for c in S.CASES])
def test_counts_equal_the_oracle(mvs, synth, orc, contexts, case):
    c = case
    _check_path(mvs, c)
    mul = S.mul_of(c)
    if c.entry == "poisson":
        ctx = _ctx(mvs, c.queue)
        v = _mix_of(c).reshape(-1)
        img = v.copy()
        ctx.poisson_process(img, S.SNR_UNIT, c.seed, c.stream, c.offset)
        _took(mvs, ctx, c)
        want = orc.poisson_counter_array(v, mul, c.seed, c.stream, c.offset)
        _assert_counts(img.reshape(1, -1), v.reshape(1, -1), want.reshape(1, -1), mul, [c.offset], c.id)
        return
    if c.entry in ("extract", "extract_dev"):
        ctx = _ctx(mvs, c.queue)
        vol = _mix_of(c)
        nz, ny, nx = c.shape
        nzo = S.acquired(nz, c.inc)
        if c.entry == "extract":
            got = ctx.extract_slices(vol, c.inc, S.SNR, c.seed, c.stream)
        else:
            # both device pointers 4 bytes past a 16-byte boundary: the forms without 16-byte accesses
            d_in, d_out = ctx.dev_alloc(vol.nbytes + 16), ctx.dev_alloc(nzo * ny * nx * 4 + 16)
            try:
                ctx.upload(d_in + 4, vol)
                ctx.extract_slices_dev(d_in + 4, (nx, ny, nz), c.inc, S.SNR, c.seed, c.stream, d_out + 4)
                ctx.synchronize()
                got = ctx.download(d_out + 4, (nzo, ny, nx))
            finally:
                ctx.dev_free(d_in)
                ctx.dev_free(d_out)
        _took(mvs, ctx, c)
        lam = vol[::c.inc][:nzo]
        counters = S.counters_of(c)
        _assert_counts(got, lam, _oracle_planes(orc, lam, mul, c.seed, c.stream, counters), mul, counters, c.id)
        return
    for counts, lam, seed, stream, counters in _run_view(mvs, synth, c):
        _assert_counts(counts, lam, _oracle_planes(orc, lam, mul, seed, stream, counters), mul, counters, c.id)


# ------------------------------------------------------------------------------------------------ regressions
@pytest.mark.gpu
def test_regression_slab_queue_off_compact_counters(mvs, synth, orc):
    """Slab tiling with the work queue off: a slab that starts at a multiple of the spacing is convolved compact (its acquired
    planes only), and the queue-less vector kernel must count the RNG in SOURCE planes -- plane k of the slab on counter
    (z0 + k * inc) * plane + i, not (z0 + k) * plane + i.  64^3, inc 3, two slabs, three-step and one-call."""
    n, inc = 64, 3
    gt = _phantom((n, n, n), 5)
    psf = _psf(synth)
    dims = (n, n, n)
    plane = n * n
    mul = S.mul_of(S.Case("r", "view", (n, n, n)))
    with mvs.Context(0) as c:
        c.set_option("fused_rotate", 1)
        c.set_option("poisson_queue", 0)
        d_gt, d_acq = c.dev_alloc(gt.nbytes), c.dev_alloc(gt.nbytes)
        try:
            c.upload(d_gt, gt)
            for z0, z1 in ((0, 32), (32, 64)):
                k0 = (z0 + inc - 1) // inc
                n_acq = (z1 + inc - 1) // inc - k0
                counters = [(k0 + k) * inc * plane for k in range(n_acq)]
                for one_call in (False, True):
                    res = []
                    for snr in (S.SNR, -1.0):
                        p = c.view_params(degrees=40, delta=REF_DELTA, inc=inc, snr=snr, seed=S.SEED_BOTH, stream=5, conv_method=1)
                        if one_call:
                            k = c.view_slab_dev(d_gt, dims, psf.copy(), p, z0, z1, d_acq)
                        else:
                            own = c.view_slab_convolve_dev(d_gt, dims, psf.copy(), p, z0, z1)
                            k = c.view_slab_finish_dev(dims, p, z0, z1, own, d_acq)
                        c.synchronize()
                        assert k == n_acq
                        if snr > 0:
                            assert _recorded(mvs, c)[:2] == (S.K_VEC, 0), (z0, one_call)         # the queue-less vector kernel
                        res.append(c.download(d_acq, (k, n, n)))
                    want = _oracle_planes(orc, res[1], mul, S.SEED_BOTH, 5, counters)
                    _assert_counts(res[0], res[1], want, mul, counters, f"slab [{z0}, {z1}) one_call={one_call}")
        finally:
            c.dev_free(d_gt)
            c.dev_free(d_acq)


@pytest.mark.gpu
def test_regression_untiled_2048x2048x520_inc516_plane1(mvs, orc):
    """An untiled compact view whose two acquired planes lie (inc - 1) * plane >= 2^31 counters apart fails the queue's straddle
    guard and goes to the queue-less vector kernel (default options): plane 1, on counters 516 * 2^22 + i ~ 2^31, must be drawn
    on its SOURCE plane's counters."""
    nx = ny = 2048
    nz, inc = 520, 516
    plane = nx * ny
    assert _path(mvs, (nx, ny, 2), 1, inc, 0, 1, 16)[0] == S.K_VEC
    gt = np.full((nz, ny, nx), 0.05, np.float32)
    rng = np.random.default_rng(9)
    blob = rng.random((6, ny, nx), dtype=np.float32) ** 6 * 8
    gt[:6] += blob
    gt[nz - 6:] += blob
    del blob
    psf = np.zeros((3, 3, 3), np.float32)
    psf[1, 1, 1] = 1.0
    psf[0, 1, 1] = psf[2, 1, 1] = psf[1, 0, 1] = psf[1, 1, 0] = 0.25
    mul = S.mul_of(S.Case("r", "view", (1, 1, 1)))
    with mvs.Context(0) as c:
        d_gt, d_acq, d_lam = c.dev_alloc(gt.nbytes), c.dev_alloc(2 * plane * 4), c.dev_alloc(2 * plane * 4)
        try:
            c.upload(d_gt, gt)
            del gt
            p = c.view_params(degrees=0, delta=REF_DELTA, inc=inc, snr=S.SNR, seed=S.SEED_BOTH, stream=3, conv_method=1)
            c.simulate_view_dev(d_gt, (nx, ny, nz), psf.copy(), p, d_acq)
            assert _recorded(mvs, c)[:2] == (S.K_VEC, 0)
            pn = c.view_params(degrees=0, delta=REF_DELTA, inc=inc, snr=-1.0, seed=S.SEED_BOTH, stream=3, conv_method=1)
            c.simulate_view_dev(d_gt, (nx, ny, nz), psf.copy(), pn, d_lam)
            c.synchronize()
            counts, lam = c.download(d_acq, (2, ny, nx)), c.download(d_lam, (2, ny, nx))
        finally:
            for d in (d_gt, d_acq, d_lam):
                c.dev_free(d)
    assert float(lam[1].max()) * mul > 50
    counters = [0, inc * plane]
    assert counters[1] > 2 ** 31
    _assert_counts(counts, lam, _oracle_planes(orc, lam, mul, S.SEED_BOTH, 3, counters), mul, counters, "2048x2048x520 inc 516")


@pytest.mark.gpu
@pytest.mark.parametrize("queue", ["16", "1"])
def test_huge_lambda_on_the_queue_path(mvs, orc, contexts, queue):
    """lambda from 1e9 to 1e15 everywhere (PTRS without the squeeze): the resolver's fp32 screen of the exact test must leave these to the
    fp64 test, whose own rounding grows with lambda -- on the resolver (share 16) and where refused voxels are sampled in place (share 1)."""
    n = 16384
    v = np.exp(np.random.default_rng(17).uniform(np.log(1.1e9), np.log(1e15), n)).astype(np.float32)
    img = v.copy()
    ctx = _ctx(mvs, queue)
    ctx.poisson_process(img, S.SNR_UNIT, S.SEED_BOTH, 5, 0)
    assert _recorded(mvs, ctx)[0] == S.K_NOISE2
    _assert_counts(img.reshape(1, -1), v.reshape(1, -1), orc.poisson_counter_array(v, 1.0, S.SEED_BOTH, 5, 0).reshape(1, -1), 1.0, [0],
                   f"huge lambda, share {queue}")
