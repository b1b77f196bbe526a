"""The multi-view deconvolution without a GPU: the yardstick of tests/decon_reference.py against the oracle's exact convolution
and against the literal correlation sum, the library's host helpers (PSF flip, defaults, launch geometry), the yardstick's
sensitivity to every mistake the GPU tests are meant to catch, and its own quality on the standard case."""
import ctypes as C
import math

import numpy as np
import pytest

from . import decon_reference as R

F32 = np.float32


@pytest.fixture(scope="module")
def std():
    return R.make_case()


@pytest.mark.parametrize("kshape", [(5, 7, 9), (4, 6, 5)], ids=["odd", "even"])
def test_fp64_convolution_equals_oracle_direct(orc, kshape):
    rng = np.random.default_rng(3)
    img = rng.random((9, 11, 13)).astype(F32)
    psf = R.normalise(R.skewed_psf(kshape))
    want = orc.convolve_direct(img, psf.copy())              # normalises its copy again: a no-op up to float rounding
    got = R.conv64(img, psf)
    assert np.max(np.abs(got - want)) <= 4 * np.finfo(F32).eps * np.max(np.abs(want))


@pytest.mark.parametrize("kxyz", [(5, 7, 9), (4, 6, 5), (1, 3, 2), (1, 1, 1)], ids=str)
def test_flip_psf_equals_numpy_and_literal_correlation(mvs, kxyz):
    rng = np.random.default_rng(sum(kxyz))
    psf = rng.random(kxyz[::-1]).astype(F32)
    keep = psf.copy()
    got = mvs.flip_psf(psf)
    assert np.array_equal(psf, keep)
    want = R.flip_psf(psf)
    assert got.shape == want.shape == tuple(k | 1 for k in psf.shape)
    assert np.array_equal(got, want)
    # the recipe's c = conv(r, F) is the correlation sum, term by term; a plain flip is not where an extent is even
    r = rng.random((5, 6, 7))
    lit = R.corr_literal(r, psf)
    assert np.max(np.abs(R.conv64(r, want) - lit)) <= 1e-13 * max(1.0, np.max(np.abs(lit)))
    if any(k % 2 == 0 for k in kxyz):
        assert np.max(np.abs(R.conv64(r, psf[::-1, ::-1, ::-1]) - lit)) > 1e-3


def test_flip_psf_refuses_bad_arguments(mvs):
    L = mvs._lib.load()
    out = np.zeros(8, F32)
    od = (C.c_int64 * 3)()
    assert L.mvsim_decon_flip_psf(None, (C.c_int64 * 3)(1, 1, 1), C.c_void_p(out.ctypes.data), od) == mvs._lib.MVSIM_EINVAL
    assert L.mvsim_decon_flip_psf(C.c_void_p(out.ctypes.data), (C.c_int64 * 3)(1, 0, 1), C.c_void_p(out.ctypes.data), od) == mvs._lib.MVSIM_EINVAL
    assert L.mvsim_decon_geometry(None) == mvs._lib.MVSIM_EINVAL


def test_defaults_and_geometry(mvs):
    p = mvs.decon_params()
    assert p.iterations >= 1 and p.method == 0 and p.init_from_psi == 0 and p.init_value <= 0
    assert p.min_value == F32(1e-4) and p.eps == F32(1e-6) and p.lambda_ == 0.0
    q = mvs.decon_params(iterations=3, tikhonov=0.006)
    assert q.iterations == 3 and q.lambda_ == 0.006
    with pytest.raises(TypeError):
        mvs.decon_params(bogus=1)
    cap, per = mvs.decon_geometry()
    assert 256 <= cap <= 4096 and per % 256 == 0 and 256 <= per <= 4096
    assert C.sizeof(mvs.DeconParams) == 32 and C.sizeof(mvs._lib.DeconStat) == 24


def test_float32_steps_against_scalar_arithmetic():
    """ratio32 / update32 element by element against Python scalars rounded with numpy.float32."""
    rng = np.random.default_rng(11)
    psi = (rng.random(64) * 3).astype(F32)
    c = (rng.random(64) * 2).astype(F32)
    w = rng.random(64).astype(F32)
    c[:4] = [0, np.nan, np.inf, 1e-9]
    for lam in (0.0, 0.006):
        got, nfl, mc = R.update32(psi, c, w, 1e-4, lam)
        for i in range(64):
            n = F32(psi[i] * c[i])
            if lam > 0:
                with np.errstate(invalid="ignore"):
                    n = F32((np.sqrt(np.float64(1.0) + np.float64(2.0 * lam) * np.float64(n)) - 1.0) / lam)
            if not n >= F32(1e-4):
                n = F32(1e-4)
            want = F32(psi[i] + F32(w[i] * F32(n - psi[i])))
            assert R.same_bits(got[i], want), (i, lam)
    b = np.array([0, -1, 1e-40, 1e-7, np.nan, np.inf, 2], F32)
    r = R.ratio32(np.full(7, 3, F32), b, 1e-6)
    assert R.same_bits(r, np.array([F32(3) / F32(1e-6)] * 5 + [0, 1.5], F32))


@pytest.mark.parametrize("lam", [0.0, 0.006])
def test_yardstick_sees_every_mistake(std, lam):
    kw = dict(iterations=3, min_value=R.STD_MIN_VALUE, eps=R.STD_EPS, lam=lam)
    good = R.deconvolve64(std["views"], std["psfs"], std["weights"], **kw)[-1]
    mistakes = ["no_flip", "reversed", "simultaneous", "no_weights", "no_floor"] + (["no_lambda"] if lam > 0 else [])
    for m in mistakes:
        bad = R.deconvolve64(std["views"], std["psfs"], std["weights"], mistake=m, **kw)[-1]
        err = R.range_err(bad, good)
        print(f"lambda {lam} {m}: {err:.3g} of range")
        assert err > 100 * R.TOL, m
    assert R.range_err(R.deconvolve64(std["views"], std["psfs"], std["weights"], mistake="no_flip", **kw)[-1], good) >= 9e-2
    assert R.range_err(R.deconvolve64(std["views"], std["psfs"], std["weights"], mistake="reversed", **kw)[-1], good) >= 9e-2


def test_tolerance_covers_the_convolutions_bound(std):
    """Every convolution of the fp64 recipe perturbed by the library's full bound (1e-5 of its range) stays within TOL / 3."""
    rng = np.random.default_rng(1)

    def perturb(x):
        return x + (rng.random(x.shape) * 2 - 1) * 1e-5 * (x.max() - x.min())
    kw = dict(iterations=3, min_value=R.STD_MIN_VALUE, eps=R.STD_EPS)
    good = R.deconvolve64(std["views"], std["psfs"], std["weights"], **kw)[-1]
    err = R.range_err(R.deconvolve64(std["views"], std["psfs"], std["weights"], perturb=perturb, **kw)[-1], good)
    print(f"propagated bound: {err:.3g} of range")
    assert err <= R.TOL / 3


def test_reference_quality_falls_monotonically():
    c = R.make_case(ones=True)
    est = R.deconvolve64(c["views"], c["psfs"], c["weights"], iterations=5, min_value=R.STD_MIN_VALUE, eps=R.STD_EPS)
    q = [R.nrmse(e, c["truth"]) for e in est]
    print("NRMSE per iteration:", " ".join(f"{v:.4f}" for v in q))
    assert all(b < a for a, b in zip(q, q[1:])), q
    assert math.isfinite(q[-1]) and q[-1] < 0.5 * q[0]
