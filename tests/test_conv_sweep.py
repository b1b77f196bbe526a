"""The convolution swept over its compiled instances (tests/conv_sweep_cases.py): every length of the hand-written FFT's size
table as y lines, FFT z pass and x half length, with zero and with the largest padding slack; the split y lines taken and
declined; the sizes just past the table (rocFFT); the direct z pass for Kz = 1 .. 64; every (NG, NEAR) instance of the direct
stencil and its chunk boundaries; and every half length of the fused rotate + attenuate + x transform, both block shapes.

Convolution cases are held to the oracle's exact fp64 direct sum on every voxel (mirror-single boundary, centre K/2, no flip);
the fused kernel bit for bit to the separate kernels.  The CPU tests check that the sweep's table is the library's, that the
cases cover every instance, and that the inputs would expose the classic convolution mistakes."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import zlib
from collections import defaultdict

import numpy as np
import pytest

from . import conv_sweep_cases as S
from .conftest import ROOT, rel_to_max

CONV_TOL = 1e-5          # range-normalised, as in test_gpu_parity
SPLIT_AGREE = 2e-6       # the split y lines against the one-block transform
SEED = 464232194


def _inputs(case):
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    v = rng.random(case.shape, dtype=np.float32)
    psf = rng.random(case.kshape, dtype=np.float32) + 0.05      # not symmetric: a flip or a wrong centre is a large error
    return v, psf


def _i64(vals):
    return (C.c_int64 * len(vals))(*vals)


def _fft_geometry(mvs, dim, kdim):
    """mvsim_fft_geometry: {Px, Py, Pz or Nz, Hxp, direct z pass?}, or None when no hand-written size fits."""
    g = _i64([0] * 5)
    rc = mvs._lib.load().mvsim_fft_geometry(_i64(dim), _i64(kdim), g)
    return list(g) if rc == 0 else None


def _stencil_geometry(mvs, kdim):
    g = _i64([0] * 5)
    assert mvs._lib.load().mvsim_stencil_geometry(_i64(kdim), g) == 0
    return list(g)


# ------------------------------------------------------------------------------------------------ CPU: table, coverage, yardstick
def _table_of_fft_dev_h():
    text = open(os.path.join(ROOT, "multiview-simulation_amd", "csrc", "fft_dev.h")).read()
    m = re.search(r"#ifdef MVSIM_DEV_SIZES\n.*?\n#else\n(.*?)\n#endif", text, re.S)
    assert m, "MVSIM_FFT_SIZES: product branch not found"
    return [tuple(int(t) for t in x.split(",")) for x in re.findall(r"X\(\s*(\d+(?:\s*,\s*\d+)*)\s*\)", m.group(1))]


def test_sweep_table_is_the_product_size_table():
    table = _table_of_fft_dev_h()
    assert len(table) == 48
    assert [(e[0], tuple(e[1:])) for e in table] == S.FFT_SIZES
    for L, rad in S.FFT_SIZES:
        assert int(np.prod(rad)) == L, (L, rad)
    assert S.LENGTHS == sorted(set(S.LENGTHS))


def test_stencil_geometry_restatement_matches_the_library(mvs):
    """The sweep picks its stencil PSFs through a restatement of pair_geometry: it must be the library's (host-only call)."""
    kdims = {c.kdim for c in S.cases() if c.role == "stencil"} | {(k, 5, 9) for k in range(1, 65, 3)} | {(9, k, k) for k in (1, 17, 40, 64)}
    for kd in sorted(kdims):
        g = _stencil_geometry(mvs, kd)
        assert tuple(g[:3]) == S.stencil_geometry(kd), kd


GEOMETRY_EDGES = (1, 2, 15, 16, 17, 63, 64, 512, 513, 576, 577, 1024, 1121, 2048, 2240, 2241, 4481)
GEOMETRY_PSF_XY = (1, 31, 100)
GEOMETRY_PSF_Z = (1, 47, 48, 64, 65, 100)          # around the inline z pass's first depth and the direct z pass's last


def _geometry_sweep(mvs, zfft):
    """(cases, cases without a hand-written size, mismatches) of mvsim_fft_geometry against the restatement of
    conv_sweep_cases (pick, pick_x, hxp, lines_per_tile, NLZ): the cross product of the edge sizes and 20 000 seeded shapes."""
    fn = mvs._lib.load().mvsim_fft_geometry
    pick = {need: S.pick(need) for need in range(1, 4600)}
    rng = np.random.default_rng(SEED)
    rnd = np.concatenate([rng.integers(1, 2300, (20000, 3)), rng.integers(1, 101, (20000, 3))], axis=1).tolist()
    edges = [(x, y, z, kx, ky, kz) for x in GEOMETRY_EDGES for y in GEOMETRY_EDGES for z in GEOMETRY_EDGES
             for kx in GEOMETRY_PSF_XY for ky in GEOMETRY_PSF_XY for kz in GEOMETRY_PSF_Z]
    dim, kdim, g = _i64([0] * 3), _i64([0] * 3), _i64([0] * 5)
    none, bad = 0, []
    for c in edges + rnd:
        dim[:], kdim[:] = c[:3], c[3:]
        got = list(g) if fn(dim, kdim, g) == 0 else None
        m, py, pz = (pick[(c[0] + c[3]) // 2], pick[c[1] + c[4] - 1], pick[c[2] + c[5] - 1])      # pick_x: ceil((n + k - 1) / 2)
        want = None
        if m and py and pz:
            zdirect = not zfft and c[5] <= 64
            want = [2 * m, py, c[2] if zdirect else pz, S.hxp(2 * m, py, pz, zdirect), int(zdirect)]
        none += want is None
        if got != want and len(bad) < 10:
            bad.append((c, got, want))
    return len(edges) + len(rnd), none, bad


def test_fft_geometry_matches_the_restatement(mvs):
    """The plan of the hand-written convolution (conv_plan, read through mvsim_fft_geometry) against the sweep's restatement, with
    the default options here and with MVSIM_FFT_ZPASS=fft in a child process (the environment is read once per process)."""
    code = ("import importlib, json; from tests import test_conv_sweep as T; "
            "print(json.dumps(T._geometry_sweep(importlib.import_module('multiview-simulation_amd'), True)))")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MVSIM_")}
    child = subprocess.Popen([sys.executable, "-c", code], cwd=ROOT, env=dict(env, MVSIM_FFT_ZPASS="fft"), stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True)
    results = {"default": _geometry_sweep(mvs, os.environ.get("MVSIM_FFT_ZPASS") == "fft")}
    out, err = child.communicate(timeout=120)
    assert child.returncode == 0, err[-2000:]
    results["fft_zpass=fft"] = json.loads(out.splitlines()[-1])
    for name, (n, none, bad) in results.items():
        print(f"{name}: {n} cases, {none} without a hand-written size, {len(bad)} mismatches")
        assert not bad, (name, bad)
        assert n > 200000 and 2 * none < n, (name, n, none)       # ... and not by comparing None with None


def _fused_reachable():
    """(M, G) pairs rotate_attenuate_fftx can take: Nx in [64, 1024], Kx <= Nx, M in the fused range."""
    out = set()
    for nx in range(64, 1025):
        g = 2 if (nx + 63) // 64 > 8 else 1
        for need in range(nx, 2 * nx):
            m = S.pick_x(need)
            if m is not None and S.FUSED_RANGE[0] <= m <= S.FUSED_RANGE[1]:
                out.add((m, g))
    return out


def _key(c):
    """The one instance a case stands for (its landing computed from its own shape, not from what it claims)."""
    dim, kdim = c.dim, c.kdim
    need = [dim[d] + kdim[d] - 1 for d in range(3)]
    if c.role == "ylines":
        L = S.pick(need[1])
        assert c.target["L"] == L
        return ("ylines", L, {L: "zero", S.prev_len(L) + 1: "max"}.get(need[1]))
    if c.role == "xpass":
        M = S.pick_x(need[0])
        assert c.target["M"] == M and dim[0] % 2 == 0
        return ("xpass", M, {2 * M: "zero", 2 * S.prev_len(M) + 1: "max"}.get(need[0]))
    if c.role == "zfft":
        assert c.opts == {"fft_zpass": "fft"} and kdim[2] <= 64
        return ("zfft", S.pick(need[2]), need[2] == S.pick(need[2]))
    if c.role == "zfft_deep":
        assert not c.opts and kdim[2] > 64
        return ("zfft_deep", S.pick(need[2]))
    if c.role == "split":
        return ("split", S.pick(need[1]), S.split_taken(dim, kdim, c.opts.get("fft_zpass", "auto")))
    if c.role == "fallback":
        assert c.padded() is None
        return ("fallback", "y" if need[1] == S.LENGTHS[-1] + 1 else "x" if need[0] == 2 * S.LENGTHS[-1] + 1 else None)
    if c.role == "zdirect":
        assert not c.opts and c.method == 1 and S.pick(need[2]) is not None
        return ("zdirect", kdim[2])
    if c.role == "stencil":
        assert c.method == 2
        kxp, kyc, kzc = S.stencil_geometry(kdim)
        near = S.stencil_near(dim, kdim)
        if c.tag:
            edge = {"y": (kdim[1], kyc), "z": (kdim[2], kzc)}[c.tag[0]]
            assert edge[1] < edge[0] and edge[0] % edge[1] == (0 if c.tag.endswith("full") else 1), c.id
            return ("stencil_edge", c.tag, near)
        return ("stencil", kxp // 4, near, kdim[0] - kxp)
    if c.role == "fused":
        assert S.fused_geometry_ok(dim, kdim) and c.opts == {"fused_fftx": 1}
        return ("fused", S.pick_x(need[0]), S.fused_g(c))
    raise AssertionError(c.role)


def _required_keys():
    req = set()
    for L in S.LENGTHS:
        req |= {("ylines", L, "zero"), ("ylines", L, "max"), ("xpass", L, "zero"), ("xpass", L, "max"), ("zfft", L, True)}
        if L >= 128:
            req.add(("zfft_deep", L))
    for L in S.SPLIT_LENGTHS:
        req |= {("split", L, True), ("split", L, False)}
    req |= {("fallback", "y"), ("fallback", "x")}
    req |= {("zdirect", k) for k in range(1, 65)}
    req |= {("stencil", ng, near, d) for ng in range(1, 17) for near in (True, False) for d in (0, -3)}
    req |= {("stencil_edge", e, near) for e in ("y_full", "y_plus1", "z_full", "z_plus1") for near in (True, False)}
    req |= {("fused", m, g) for m, g in _fused_reachable()}
    return req


def test_sweep_covers_every_instance():
    cases = S.cases()
    keys = [_key(c) for c in cases]
    # one case per instance: dropping any case leaves its instance unswept
    dup = {k for k in keys if keys.count(k) > 1}
    assert not dup, sorted(dup, key=str)
    assert set(keys) == _required_keys(), (sorted(set(keys) ^ _required_keys(), key=str))
    by = defaultdict(list)
    for c in cases:
        by[c.role].append(c)
    # odd and even taps along the swept axis; Nz that fill the last 16-plane z tile and that do not, and thinner than the PSF
    assert {c.kdim[1] % 2 for c in by["ylines"]} == {0, 1} and {c.kdim[0] % 2 for c in by["xpass"]} == {0, 1}
    assert {c.kdim[2] % 2 for c in by["zfft"]} == {0, 1}
    for L in S.LENGTHS[1:]:
        assert len({c.kdim[1] % 2 for c in by["ylines"] if c.target["L"] == L}) == 2, L
    zd = by["zdirect"]
    assert any(c.dim[2] % 16 == 0 for c in zd) and any(c.dim[2] % 16 for c in zd) and any(c.dim[2] < c.kdim[2] for c in zd)
    # the fused cases: rows that are not a multiple of 64, Ny > Nx, and both sides of the x = 512 block boundary
    fu = by["fused"]
    assert all(c.dim[0] % 64 for c in fu) and any(c.dim[1] > c.dim[0] for c in fu) and any(c.dim[1] == c.dim[0] for c in fu)
    # the fp64 reference stays cheap
    for c in S.conv_cases():
        assert c.macs <= S.MAX_MACS, (c.id, c.macs)


# plain numpy fp64 convolutions, right and with each classic mistake
def _index_map(n, k, c, boundary, period=None):
    """idx[a, x]: the source index tap a reads for output x (-1: zero)."""
    i = np.arange(n)[None, :] - (np.arange(k)[:, None] - c)
    if boundary == "mirror_single":
        if n == 1:
            return np.zeros_like(i)
        p = 2 * n - 2
        i = np.mod(i, p)
        return np.where(i < n, i, p - i)
    if boundary == "mirror_double":
        p = 2 * n
        i = np.mod(i, p)
        return np.where(i < n, i, p - 1 - i)
    if boundary == "zero":
        return np.where((i >= 0) & (i < n), i, -1)
    if boundary == "circular":
        i = np.mod(i, period)
        return np.where(i < n, i, -1)
    raise ValueError(boundary)


def _np_convolve(v, psf, centre="half", boundary="mirror_single", flip=False, periods=None):
    v = np.asarray(v, np.float64)
    k = np.asarray(psf, np.float64)
    if flip:
        k = k[::-1, ::-1, ::-1]
    vz = np.concatenate([v, np.zeros((1,) + v.shape[1:])], axis=0)      # index -1 of z -> a plane of zeros
    vz = np.concatenate([vz, np.zeros(vz.shape[:1] + (1,) + vz.shape[2:])], axis=1)
    vz = np.concatenate([vz, np.zeros(vz.shape[:2] + (1,))], axis=2)
    maps = []
    for ax in range(3):
        n, kk = v.shape[ax], k.shape[ax]
        c = kk // 2 if centre == "half" else (kk - 1) // 2
        maps.append(_index_map(n, kk, c, boundary, None if periods is None else periods[ax]))
    out = np.zeros(v.shape)
    for cz in range(k.shape[0]):
        for cy in range(k.shape[1]):
            plane = vz[np.ix_(maps[0][cz], maps[1][cy])]
            for cx in range(k.shape[2]):
                w = k[cz, cy, cx]
                out += w * plane[:, :, maps[2][cx]]
    return out


def _sensitivity_sample():
    """Per role, the cheapest case with an even number of taps along some axis longer than one voxel (a wrong centre shows only
    there)."""
    out = []
    by = defaultdict(list)
    for c in S.conv_cases():
        by[c.role].append(c)
    for role, cs in sorted(by.items()):
        even = [c for c in cs if any(k % 2 == 0 and n > 1 for k, n in zip(c.kdim, c.dim))]
        assert even, role
        out.append(min(even, key=lambda c: (c.macs, c.id)))
    return out


@pytest.mark.parametrize("case", _sensitivity_sample(), ids=lambda c: c.id)
def test_sweep_inputs_expose_convolution_mistakes(orc, case):
    v, psf = _inputs(case)
    p = psf.copy()
    ref = orc.convolve_direct(v, p)                       # p normalised in place
    assert rel_to_max(_np_convolve(v, p), ref) <= 1e-6    # the restatement below is the oracle's sum
    P = case.padded()
    periods = (P[2], P[1], P[0]) if P else tuple(n + k - 1 for n, k in zip(case.shape, case.kshape))
    wrong = {
        "centre (K-1)/2": _np_convolve(v, p, centre="floor"),
        "mirror-double": _np_convolve(v, p, boundary="mirror_double"),
        "zero boundary": _np_convolve(v, p, boundary="zero"),
        "correlation (flipped PSF)": _np_convolve(v, p, flip=True),
        "circular wrap at P": _np_convolve(v, p, boundary="circular", periods=periods),
    }
    for name, w in wrong.items():
        assert rel_to_max(w, ref) > 100 * CONV_TOL, (name, rel_to_max(w, ref))


# ------------------------------------------------------------------------------------------------ GPU
_DEFAULTS = (("fft_zpass", "auto"), ("fft_backend", "custom"), ("fused_fftx", "auto"), ("exp", 0))


@pytest.fixture
def opts(ctx):
    def set_(**kw):
        for k, v in kw.items():
            ctx.set_option(k, v)
    yield set_
    for k, v in _DEFAULTS:
        ctx.set_option(k, v)


def _check_landing(mvs, case):
    dim, kdim, t = case.dim, case.kdim, case.target
    if case.role == "stencil":
        g = _stencil_geometry(mvs, kdim)
        assert g[0] == 4 * t["NG"] and S.stencil_near(dim, kdim) == bool(t["NEAR"])
        assert tuple(g[:3]) == S.stencil_geometry(kdim)
        return
    g = _fft_geometry(mvs, dim, kdim)
    if case.role == "fallback":
        assert g is None, g                                 # past the table: the library's rocFFT path
        return
    assert g is not None
    P = case.padded()
    assert (g[0], g[1]) == P[:2]
    if case.role in ("ylines", "split"):
        assert g[1] == t["L"]
    elif case.role == "xpass":
        assert g[0] == 2 * t["M"]
    elif case.role == "zfft":
        assert g[4] == 1 and P[2] == t["L"]                 # direct by default; the option forces the FFT z pass on P[2]
    elif case.role == "zfft_deep":
        assert g[4] == 0 and g[2] == t["L"]
    elif case.role == "zdirect":
        assert g[4] == 1 and g[2] == dim[2] and kdim[2] == t["Kz"]


def _convolve_cases():
    return [c for c in S.conv_cases() if c.role != "split"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", _convolve_cases(), ids=lambda c: c.id)
def test_convolution_sweep_matches_exact_sum(ctx, orc, mvs, opts, case):
    _check_landing(mvs, case)
    v, psf = _inputs(case)
    opts(**case.opts)
    got = ctx.convolve(v, psf.copy(), method=case.method)
    want = orc.convolve_direct(v, psf.copy())
    assert rel_to_max(got, want) <= CONV_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in S.cases() if c.role == "split"], ids=lambda c: c.id)
def test_split_y_lines_sweep(ctx, orc, mvs, opts, case):
    """The split lengths with the split form taken or declined (launch_lines), against the one-block transform (exp bit 8)."""
    _check_landing(mvs, case)
    assert S.split_taken(case.dim, case.kdim, case.opts.get("fft_zpass", "auto")) == (case.target["form"] == "split")
    assert not S.split_taken(case.dim, case.kdim, case.opts.get("fft_zpass", "auto"), exp=8)
    v, psf = _inputs(case)
    want = orc.convolve_direct(v, psf.copy())
    res = {}
    for exp in (0, 8):
        opts(exp=exp, **case.opts)
        res[exp] = ctx.convolve(v, psf.copy(), method=1)
        assert rel_to_max(res[exp], want) <= CONV_TOL, exp
    assert rel_to_max(res[0], res[8]) <= SPLIT_AGREE


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in S.cases() if c.role == "fused"], ids=lambda c: c.id)
def test_fused_rotate_x_transform_sweep(ctx, mvs, opts, case):
    """k_rotate_attenuate_fftx at every half length it serves: rot, att, con and acq identical to the separate kernels', with
    and without the intermediates requested (test_fused_rotate_attenuate_x_transform_is_bit_identical's contract)."""
    g = _fft_geometry(mvs, case.dim, case.kdim)
    assert g is not None and g[0] == 2 * case.target["M"] and g[4] == 1 and S.fused_g(case) == case.target["G"]
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    gt = rng.random(case.shape, dtype=np.float32) * (rng.random(case.shape, dtype=np.float32) < 0.7)
    psf = rng.random(case.kshape, dtype=np.float32) + 0.05
    inc = 1 + case.target["M"] % 2
    res = {}
    for mode in (0, 1):
        opts(fused_fftx=mode)
        p = ctx.view_params(degrees=S.fused_degrees(case), inc=inc, snr=25.0, seed=SEED, stream=5, conv_method=1)
        full = ctx.simulate_view(gt, psf.copy(), p, want=("rot", "att", "con", "acq"))
        only = ctx.simulate_view(gt, psf.copy(), p, want=("acq",))
        res[mode] = (full, only)
    for k in ("rot", "att", "con", "acq"):
        assert np.array_equal(res[0][0][k], res[1][0][k]), k
    assert np.array_equal(res[0][1]["acq"], res[1][1]["acq"])
    assert float(res[1][0]["acq"].max()) > 0
