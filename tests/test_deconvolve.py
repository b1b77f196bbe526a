"""The multi-view deconvolution on the GPU, against tests/decon_reference.py.

The two elementwise kernels are held bit for bit to the float32 restatement (every NaN equal to every NaN: its sign and payload
are the hardware's choice) over the head / body / tail forms, every pointer alignment and the launch cap; the whole recipe to
1e-4 of the fp64 result's range (the tolerance's derivation: test_deconvolve_host.py), on both convolution methods, even PSF
extents, the stencil path and longer lines of the hand-written FFT; then the identities of the driver and its argument checks."""
import ctypes as C
import math

import numpy as np
import pytest

from . import decon_reference as R

pytestmark = pytest.mark.gpu
F32 = np.float32
MIN_VALUE = float(F32(1e-4))
EPS = float(F32(1e-6))


class Dev:
    """Device copies of host arrays, each `offset` floats into its own allocation."""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def put(self, a, offset=0):
        a = np.ascontiguousarray(a, dtype=F32)
        base = self.ctx.dev_alloc(a.nbytes + 4 * offset + 64)
        self.ptrs.append(base)
        self.ctx.upload(base + 4 * offset, a)
        return base + 4 * offset

    def free(self):
        self.ctx.synchronize()
        for p in self.ptrs:
            self.ctx.dev_free(p)
        self.ptrs = []


@pytest.fixture()
def dev(ctx):
    d = Dev(ctx)
    yield d
    d.free()


def stage_sizes(mvs):
    cap, per = mvs.decon_geometry()
    return [1, 3, 4, 5, 255, 1027, cap * per + 5, 3 * cap * per + 7]


def stage_inputs(n, seed):
    rng = np.random.default_rng(seed)
    phi = rng.poisson(3.0, n).astype(F32)                       # holds zeros
    b = (rng.random(n) * 4 + 0.01).astype(F32)
    c = (rng.random(n) * 2).astype(F32)
    psi = (rng.random(n) * 5 + MIN_VALUE).astype(F32)
    w = rng.random(n).astype(F32)
    sb = np.array([0, -1.5, 1e-40, -1e-40, 1e-7, np.nan, np.inf, -np.inf], F32)
    sc = np.array([0, np.nan, np.inf, 1e-12], F32)
    step = max(1, n // 61)
    for k, v in enumerate(sb):
        b[(k * step + 1) % n::max(n // 7, len(sb) * step + 3)] = v
    for k, v in enumerate(sc):
        c[(k * step + 2) % n::max(n // 5, len(sc) * step + 5)] = v
    phi[::9] = 0
    psi[::11] = F32(MIN_VALUE)
    return phi, b, c, psi, w


OFFSETS3 = [(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)]


def offsets_for(n):
    return OFFSETS3 if n <= 4096 else [(0, 0, 0), (1, 1, 1), (0, 1, 0)]


@pytest.mark.parametrize("which", range(8))
def test_ratio_bit_for_bit(ctx, mvs, dev, which):
    n = stage_sizes(mvs)[which]
    phi, b, _, _, _ = stage_inputs(n, 100 + which)
    want = R.ratio32(phi, b, EPS)
    for op, ob, orr in offsets_for(n):
        dp, db, dr = dev.put(phi, op), dev.put(b, ob), dev.put(np.zeros(n, F32), orr)
        ctx.decon_ratio_dev(dp, db, n, EPS, dr)
        assert R.same_bits(ctx.download(dr, (n,)), want), (n, op, ob, orr)
        assert R.same_bits(ctx.download(db, (n,)), b), "the blurred input was written"
        ctx.decon_ratio_dev(dp, db, n, EPS, db)                 # in place over b
        assert R.same_bits(ctx.download(db, (n,)), want), (n, op, ob, "in place")
        dev.free()


@pytest.mark.parametrize("lam", [0.0, 0.006])
@pytest.mark.parametrize("which", range(8))
def test_update_bit_for_bit(ctx, mvs, dev, which, lam):
    n = stage_sizes(mvs)[which]
    _, _, c, psi, wr = stage_inputs(n, 200 + which)
    modes = {"null": None, "zeros": np.zeros(n, F32), "ones": np.ones(n, F32), "random": wr}
    combos = offsets_for(n)
    for mi, (name, w) in enumerate(modes.items()):
        want, _, _ = R.update32(psi, c, w, MIN_VALUE, lam)
        for op, oc, ow in (combos if n <= 4096 else combos[mi % 3:mi % 3 + 1] + [combos[(mi + 1) % 3]]):
            dp, dc = dev.put(psi, op), dev.put(c, oc)
            dw = dev.put(w, ow) if w is not None else 0
            ctx.decon_update_dev(dp, dc, dw, n, MIN_VALUE, lam)
            assert R.same_bits(ctx.download(dp, (n,)), want), (n, name, op, oc, ow, lam)
            assert R.same_bits(ctx.download(dc, (n,)), c), "the correlation was written"
            dev.free()


@pytest.mark.parametrize("lam", [0.0, 0.006])
@pytest.mark.parametrize("which", [5, 6, 7])
def test_update_stats(ctx, mvs, dev, which, lam):
    n = stage_sizes(mvs)[which]
    _, _, c, psi, wr = stage_inputs(n, 300 + which)
    c[np.isinf(c)] = 0.5                                        # finite estimates: the sum is a number (NaN and 0 stay: they floor)
    for w, off in ((None, 0), (wr, 1)):
        want, nfl, mc = R.update32(psi, c, w, MIN_VALUE, lam)
        exact = math.fsum(want.astype(np.float64).tolist())
        runs = []
        for _ in range(2):
            dp, dc = dev.put(psi, off), dev.put(c, off)
            dw = dev.put(w, off) if w is not None else 0
            st = ctx.decon_update_dev(dp, dc, dw, n, MIN_VALUE, lam, stats=True)
            assert R.same_bits(ctx.download(dp, (n,)), want)
            runs.append(st)
            dev.free()
        st = runs[0]
        print(f"n {n} lambda {lam}: sum rel err {abs(st['sum_psi'] - exact) / exact:.3g}, max_change {st['max_change']}, floored {st['n_floored']}")
        assert st["n_floored"] == nfl and nfl > 0
        assert F32(st["max_change"]) == mc
        assert abs(st["sum_psi"] - exact) <= n * 2.0 ** -52 * exact
        assert runs[0] == runs[1]


# ------------------------------------------------------------------------------------------------ the whole recipe
_CASES = {}


def case(name):
    if name not in _CASES:
        if name == "std":
            c = R.make_case()
        elif name == "ones":
            c = R.make_case(ones=True)
        elif name == "even":
            c = R.make_case(psf_shapes=((5, 6, 4),) + R.STD_PSF_SHAPES[1:])          # (4,6,5) as x, y, z
        elif name == "stencil":
            c = R.make_case(psf_shapes=((3, 3, 3), (2, 3, 4), (3, 4, 3)))            # (3,3,3), (4,3,2), (3,4,3) as x, y, z
        elif name == "large":
            c = R.make_case(shape_zyx=(40, 80, 96), psf_shapes=((11, 13, 15), (15, 13, 11)))
        c["ref"] = {}
        _CASES[name] = c
    return _CASES[name]


def reference(name, T, lam):
    c = case(name)
    if (T, lam) not in c["ref"]:
        c["ref"][(T, lam)] = R.deconvolve64(c["views"], c["psfs"], c["weights"], iterations=T, min_value=R.STD_MIN_VALUE, eps=R.STD_EPS, lam=lam)
    return c["ref"][(T, lam)]


def run_gpu(ctx, mvs, name, T, lam, method, **kw):
    c = case(name)
    p = mvs.decon_params(iterations=T, method=method, min_value=R.STD_MIN_VALUE, eps=R.STD_EPS, lambda_=lam)
    return ctx.deconvolve(c["views"], c["psfs"], kw.pop("weights", c["weights"]), p, **kw)


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("lam", [0.0, 0.006])
def test_standard_case(ctx, mvs, lam, method):
    got = run_gpu(ctx, mvs, "std", 3, lam, method)
    err = R.range_err(got, reference("std", 3, lam)[-1])
    print(f"standard case lambda {lam} method {method}: {err:.3g} of range")
    assert err <= R.TOL


@pytest.mark.parametrize("name,T,method", [("even", 3, 0), ("even", 3, 1), ("stencil", 3, 2), ("large", 2, 0)])
def test_further_cases(ctx, mvs, name, T, method):
    got = run_gpu(ctx, mvs, name, T, 0.0, method)
    err = R.range_err(got, reference(name, T, 0.0)[-1])
    print(f"{name} T {T} method {method}: {err:.3g} of range")
    assert err <= R.TOL


def test_quality_follows_the_reference(ctx, mvs):
    c = case("ones")
    ref = reference("ones", 3, 0.0)
    got = run_gpu(ctx, mvs, "ones", 3, 0.0, 0)
    q_gpu, q_ref, q0 = R.nrmse(got, c["truth"]), R.nrmse(ref[-1], c["truth"]), R.nrmse(ref[0] + 0 * c["truth"], c["truth"])
    print(f"NRMSE: GPU {q_gpu:.5f}, fp64 {q_ref:.5f}, start {q0:.5f}")
    assert abs(q_gpu - q_ref) <= 0.01 * q_ref
    assert q_gpu < q0


# ------------------------------------------------------------------------------------------------ identities
def test_null_weights_equal_unit_weights(ctx, mvs):
    """psi + 1 * (n - psi) is n bit for bit exactly where the float subtraction n - psi is exact, which Sterbenz' lemma grants for
    psi / 2 <= n <= 2 psi.  The recipe rounds the subtraction, so the identity is tested where that holds at every step: smooth views
    within +-25 % of their mean and no voxel near the floor (every ratio, hence every c, stays within [0.6, 1.6]).  On the standard
    case, whose first steps move voxels by far more than a factor of two, the two forms differ by that rounding; the figure is printed (measured on an MI355X: 4.19e-07 of range) and held to the tolerance."""
    z, y, x = np.meshgrid(np.arange(12), np.arange(20), np.arange(24), indexing="ij")
    truth = 10.0 * (1.0 + 0.25 * np.sin(0.5 * x + 0.3 * y) * np.cos(0.4 * z))
    psfs = [R.skewed_psf(s, i) for i, s in enumerate(R.STD_PSF_SHAPES)]
    views = [R.conv64(truth, R.normalise(p)).astype(F32) for p in psfs]
    ones = [np.ones(truth.shape, F32)] * 3
    p = mvs.decon_params(iterations=3, method=1)
    a = ctx.deconvolve(views, psfs, None, p)
    b = ctx.deconvolve(views, psfs, ones, p)
    assert R.same_bits(a, b)
    sa, sb = run_gpu(ctx, mvs, "ones", 3, 0.0, 1, weights=None), run_gpu(ctx, mvs, "ones", 3, 0.0, 1)
    print(f"standard case, null against unit weights: {R.range_err(sa, sb):.3g} of range")
    assert R.range_err(sa, sb) <= R.TOL


def test_unit_psf_returns_the_floored_view(ctx, mvs):
    phi = case("std")["views"][0]
    got = ctx.deconvolve([phi], [np.ones((1, 1, 1), F32)], None, mvs.decon_params(iterations=1, min_value=R.STD_MIN_VALUE))
    want = np.maximum(phi, F32(R.STD_MIN_VALUE))
    assert R.range_err(got, want) <= 1e-5


def test_host_equals_device_and_repeats(ctx, mvs, dev):
    c = case("std")
    p = mvs.decon_params(iterations=2, method=0, min_value=R.STD_MIN_VALUE, lambda_=0.006)
    psfs = [q.copy() for q in c["psfs"]]
    host, hstats = ctx.deconvolve(c["views"], psfs, c["weights"], p, stats=True)
    assert all(np.array_equal(a, b) for a, b in zip(psfs, c["psfs"])), "a caller's PSF was written"
    n = host.size
    dim = host.shape[::-1]
    dv = [dev.put(v) for v in c["views"]]
    dw = [dev.put(w) for w in c["weights"]]
    runs = []
    for _ in range(2):
        dpsi = dev.put(np.zeros(n, F32))
        st = ctx.deconvolve_dev(dv, dim, psfs, dpsi, dw, p, stats=True)
        runs.append((ctx.download(dpsi, host.shape), st))
    assert R.same_bits(runs[0][0], host) and runs[0][1] == hstats
    assert R.same_bits(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert len(hstats) == 2 and len(hstats[0]) == 3
    assert abs(hstats[-1][-1]["sum_psi"] - float(np.sum(host, dtype=np.float64))) <= 1e-9 * float(np.sum(host, dtype=np.float64))
    assert all(np.array_equal(a, b) for a, b in zip(psfs, c["psfs"]))


def test_restart_from_psi(ctx, mvs):
    c = case("std")
    kw = dict(method=0, min_value=R.STD_MIN_VALUE)
    two = ctx.deconvolve(c["views"], c["psfs"], c["weights"], mvs.decon_params(iterations=2, **kw))
    one = ctx.deconvolve(c["views"], c["psfs"], c["weights"], mvs.decon_params(iterations=1, **kw))
    keep = one.copy()
    again = ctx.deconvolve(c["views"], c["psfs"], c["weights"], mvs.decon_params(iterations=1, init_from_psi=1, **kw), psi=one)
    assert np.array_equal(one, keep)
    assert R.same_bits(again, two)
    assert not R.same_bits(one, two)


def test_constant_start(ctx, mvs):
    c = case("std")
    got = ctx.deconvolve(c["views"], c["psfs"], c["weights"], mvs.decon_params(iterations=1, init_value=7.5, min_value=R.STD_MIN_VALUE))
    ref = R.deconvolve64(c["views"], c["psfs"], c["weights"], iterations=1, init_value=7.5, min_value=R.STD_MIN_VALUE)[-1]
    assert R.range_err(got, ref) <= R.TOL


def test_stats_equal_the_stage_operators(ctx, mvs, dev):
    """One view, so the estimate in front of the last step is the result of one iteration less; a PSF of dyadic taps that sum to 1,
    so that normalising it a second time (mvsim_convolve_dev does) changes no bit."""
    c = case("std")
    phi, w = c["views"][0], c["weights"][0]
    t3, t4 = np.array([0.25, 0.5, 0.25]), np.array([0.25, 0.5, 0.125, 0.125])
    psf = (t3[:, None, None] * t3[None, :, None] * t4[None, None, :]).astype(F32)            # (4, 3, 3) as x, y, z: one even extent
    assert float(np.sum(psf, dtype=np.float64)) == 1.0
    n, dim = phi.size, phi.shape[::-1]
    dphi, dw = dev.put(phi), dev.put(w)
    d2, d1, db, dc = (dev.put(np.zeros(n, F32)) for _ in range(4))
    kw = dict(method=1, min_value=R.STD_MIN_VALUE, lambda_=0.006)
    st2 = ctx.deconvolve_dev([dphi], dim, [psf], d2, [dw], mvs.decon_params(iterations=2, **kw), stats=True)
    ctx.deconvolve_dev([dphi], dim, [psf], d1, [dw], mvs.decon_params(iterations=1, **kw))
    ctx.convolve_dev(d1, dim, psf.copy(), db, method=1)
    ctx.decon_ratio_dev(dphi, db, n, EPS, db)
    ctx.convolve_dev(db, dim, mvs.flip_psf(psf), dc, method=1)
    st = ctx.decon_update_dev(d1, dc, dw, n, R.STD_MIN_VALUE, 0.006, stats=True)
    assert R.same_bits(ctx.download(d1, (n,)), ctx.download(d2, (n,)))
    assert st == st2[1][0]
    assert st["n_floored"] > 0 and st["max_change"] > 0


def test_invalid_arguments(ctx, mvs, dev):
    L, h = ctx._L, ctx._h
    n, dim = 4 * 5 * 6, (C.c_int64 * 3)(6, 5, 4)
    dv, dw, dpsi = dev.put(np.ones(n, F32)), dev.put(np.ones(n, F32)), dev.put(np.ones(n, F32))
    psf = np.ones((3, 3, 3), F32)

    def call(views=(dv,), weights=(dw,), psfs=(psf.ctypes.data,), kd=(3, 3, 3), nv=1, dim_=dim, psi=dpsi, p=None, **kw):
        prm = mvs.decon_params(**{"iterations": 1, **kw}) if p is None else p
        arr = lambda t: (C.c_void_p * max(1, len(t)))(*t) if t is not None else None
        return L.mvsim_deconvolve_dev(h, arr(views), arr(weights), arr(psfs), (C.c_int64 * len(kd))(*kd) if kd else None, nv, dim_,
                                      C.byref(prm) if prm is not False else None, C.c_void_p(psi), None)
    E = mvs._lib.MVSIM_EINVAL
    assert call() == 0
    assert call(weights=None) == 0
    assert call(nv=0) == E and call(nv=33) == E
    assert call(iterations=0) == E
    assert call(views=None) == E and call(psfs=None) == E and call(kd=None) == E and call(psi=None) == E and call(dim_=None) == E
    assert call(p=False) == E
    assert call(views=(None,)) == E and call(weights=(None,)) == E and call(psfs=(None,)) == E
    assert call(kd=(3, 0, 3)) == E
    assert call(dim_=(C.c_int64 * 3)(6, 0, 4)) == E
    assert call(psi=dv) == E and call(psi=dw) == E and call(psi=dv + 4 * (n - 1)) == E
    assert call(method=3) == E and call(method=-1) == E
    assert call(eps=0.0) == E and call(min_value=0.0) == E and call(min_value=-1.0) == E
    assert call(lambda_=-1e-3) == E and call(lambda_=float("nan")) == E
    assert call(init_from_psi=2) == E
    assert b"deconvolve" in L.mvsim_last_error()
    # the stencil cannot take the 65 taps of a flipped PSF of 64; the automatic method takes the FFT
    big = np.ones((1, 1, 64), F32)
    wide = (C.c_int64 * 3)(96, 5, 4)
    w1, w2 = dev.put(np.ones(96 * 5 * 4, F32)), dev.put(np.ones(96 * 5 * 4, F32))
    assert call(views=(w1,), weights=None, psi=w2, dim_=wide, psfs=(big.ctypes.data,), kd=(64, 1, 1), method=2) == E
    assert call(views=(w1,), weights=None, psi=w2, dim_=wide, psfs=(big.ctypes.data,), kd=(64, 1, 1), method=0) == 0
    with pytest.raises(ValueError):
        ctx.deconvolve([np.ones((4, 5, 6), F32)], [psf, psf])
    with pytest.raises(ValueError):
        ctx.decon_ratio_dev(dv, dw, n, 0.0, dpsi)
    with pytest.raises(ValueError):
        ctx.decon_update_dev(dpsi, dv, 0, n, 0.0)
    ctx.synchronize()
