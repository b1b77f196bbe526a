"""The bead detector without a GPU: the library's host helpers (taps, defaults, geometry, every refusal) against the restatement of
tests/dog_reference.py, and the recipe on its own through the restatement -- bead volumes clean and noisy, and the half-voxel
case that the second refusal rule of the localisation exists for."""
import ctypes as C
import math

import numpy as np
import pytest

from . import dog_reference as R

F32 = np.float32
SIGMAS = [0.5, 1.0, 1.8, 1.8 * math.pow(2.0, 0.25), 3.0, 10.3]


@pytest.mark.parametrize("sigma", SIGMAS, ids=lambda s: f"{s:.4g}")
def test_taps_equal_the_restatement_bit_for_bit(mvs, sigma):
    got, want = mvs.dog_taps(sigma), R.taps(sigma)
    assert got.dtype == want.dtype == F32 and len(got) == R.diameter(sigma)
    assert R.same_bits(got, want)
    assert np.array_equal(got, got[::-1]) and abs(float(np.sum(got.astype(np.float64))) - 1.0) < 1e-6


def test_diameter_rule_and_the_cap(mvs):
    assert mvs.beads.kernel_diameter(1.8) == R.diameter(1.8) == 11
    for sigma, d in ((0.01, 3), (0.5, 5), (0.83, 5), (0.84, 7), (1.0, 7), (1.8, 11), (2.14, 13), (10.3, 63), (10.49, 63)):
        assert R.diameter(sigma) == d == len(mvs.dog_taps(sigma)) == mvs.beads.kernel_diameter(sigma), sigma
    for sigma in (10.5, 11.0, 100.0, 1e300, 0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            mvs.dog_taps(sigma)
    L = mvs._lib.load()
    n = C.c_int(0)
    assert L.mvsim_dog_taps(1.0, None, C.byref(n)) == mvs._lib.MVSIM_EINVAL
    assert L.mvsim_dog_taps(1.0, (C.c_float * 63)(), None) == mvs._lib.MVSIM_EINVAL


def test_defaults_and_geometry(mvs):
    p = mvs.dog_params()
    assert list(p.sigma1) == [1.8] * 3 and list(p.sigma2) == [1.8 * math.pow(2.0, 0.25)] * 3
    assert p.threshold == F32(0.008) and p.max_moves == 4
    q = mvs.dog_params(sigma1=(1.0, 2.5, 0.7), sigma2=2.0, threshold=5, max_moves=0)
    assert list(q.sigma1) == [1.0, 2.5, 0.7] and list(q.sigma2) == [2.0] * 3 and q.threshold == 5 and q.max_moves == 0
    with pytest.raises(TypeError):
        mvs.dog_params(bogus=1)
    assert C.sizeof(mvs.DogParams) == 56 and C.sizeof(mvs._lib.Peak) == 40 == mvs.detection.PEAK_DTYPE.itemsize == R.PEAK_DTYPE.itemsize
    g = mvs.dog_geometry()
    assert g["tile_x"] % 4 == 0 and 16 <= g["tile_x"] <= 256 and 4 <= g["tile_y"] <= 64 and 4 <= g["tile_z"] <= 256
    assert g["max_radius"] == (R.MAX_TAPS - 1) // 2 and g["peak_block_voxels"] % 256 == 0 and 256 <= g["peak_block_voxels"] <= 1 << 16
    assert mvs._lib.load().mvsim_dog_geometry(None) == mvs._lib.MVSIM_EINVAL
    d = mvs.DifferenceOfGaussian(sigma=(1.0, 1.0, 3.0), threshold=5)
    assert list(d.params.sigma2) == [v * 2.0 ** 0.25 for v in (1.0, 1.0, 3.0)] and d.params.threshold == 5


def test_every_refusal_is_reachable_without_a_device(mvs):
    """A null context is the LAST thing every entry point looks at: with good arguments the refusal names the context, with a bad one it
    names the argument."""
    L, EINVAL = mvs._lib.load(), mvs._lib.MVSIM_EINVAL
    buf = (C.c_char * 64)()
    ptr = C.c_void_p(C.addressof(buf))                     # never dereferenced: no call gets as far as a launch

    def dim(*v):
        return (C.c_int64 * 3)(*v)

    def msg():
        return (L.mvsim_last_error() or b"").decode()

    def detect(entry="mvsim_detect_beads_dev", img=ptr, src=0, d=dim(8, 8, 8), params=None, cap=4, peaks=ptr, n=ptr, **kw):
        p = mvs.dog_params(**kw) if params is None else params
        return getattr(L, entry)(None, img, src, d, C.byref(p) if p != 0 else None, cap, peaks, n)

    for entry in ("mvsim_detect_beads_dev", "mvsim_detect_beads"):
        assert detect(entry) == EINVAL and "ctx" in msg()
        bad = [dict(img=None), dict(peaks=None), dict(n=None), dict(d=None), dict(params=0), dict(src=2), dict(src=-1),
               dict(d=dim(8, 1, 8)), dict(d=dim(1, 8, 8)), dict(d=dim(8, 8, 0)), dict(sigma1=0.0), dict(sigma2=(1.0, -1.0, 1.0)),
               dict(sigma1=math.nan), dict(sigma2=math.inf), dict(sigma1=(1.0, 1.0, 10.5)), dict(threshold=math.nan), dict(cap=0),
               dict(cap=-3), dict(max_moves=-1)]
        for kw in bad:
            assert detect(entry, **kw) == EINVAL, kw
            assert "ctx" not in msg(), (kw, msg())
    p = mvs.dog_params()
    assert L.mvsim_dog_dev(None, ptr, 0, dim(8, 8, 8), C.byref(p), ptr) == EINVAL and "ctx" in msg()
    for args in ((None, 0, dim(8, 8, 8), C.byref(p), ptr), (ptr, 0, dim(8, 8, 8), C.byref(p), None), (ptr, 3, dim(8, 8, 8), C.byref(p), ptr),
                 (ptr, 0, dim(8, 8, 1), C.byref(p), ptr), (ptr, 0, dim(8, 8, 8), None, ptr),
                 (ptr, 0, dim(8, 8, 8), C.byref(mvs.dog_params(sigma1=-2.0)), ptr), (ptr, 0, dim(8, 8, 8), C.byref(mvs.dog_params(sigma2=20.0)), ptr)):
        assert L.mvsim_dog_dev(None, *args) == EINVAL and "ctx" not in msg(), msg()
    assert L.mvsim_find_peaks_dev(None, ptr, dim(8, 8, 8), 1.0, 4, ptr, ptr) == EINVAL and "ctx" in msg()
    assert L.mvsim_find_peaks_dev(None, ptr, dim(2, 2, 2), math.inf, 4, ptr, ptr) == EINVAL and "ctx" in msg()   # below 3: no error
    for args in ((None, dim(8, 8, 8), 1.0, 4, ptr, ptr), (ptr, dim(8, 8, 8), 1.0, 4, None, ptr), (ptr, dim(8, 8, 8), 1.0, 4, ptr, None),
                 (ptr, dim(8, 0, 8), 1.0, 4, ptr, ptr), (ptr, dim(8, 8, 8), math.nan, 4, ptr, ptr), (ptr, dim(8, 8, 8), 1.0, 0, ptr, ptr)):
        assert L.mvsim_find_peaks_dev(None, *args) == EINVAL and "ctx" not in msg(), msg()
    assert L.mvsim_localise_peaks_dev(None, ptr, dim(8, 8, 8), ptr, ptr, 4, 4, ptr) == EINVAL and "ctx" in msg()
    for args in ((None, dim(8, 8, 8), ptr, ptr, 4, 4, ptr), (ptr, dim(8, 8, 8), None, ptr, 4, 4, ptr), (ptr, dim(8, 8, 8), ptr, None, 4, 4, ptr),
                 (ptr, dim(8, 8, 8), ptr, ptr, 4, 4, None), (ptr, dim(8, 8, 8), ptr, ptr, 0, 4, ptr), (ptr, dim(8, 8, 8), ptr, ptr, 4, -1, ptr),
                 (ptr, None, ptr, ptr, 4, 4, ptr)):
        assert L.mvsim_localise_peaks_dev(None, *args) == EINVAL and "ctx" not in msg(), msg()


# ---- the recipe on its own ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,n_beads", [((64, 80, 96), 40), ((48, 40, 56), 12)], ids=["96x80x64", "56x40x48"])
@pytest.mark.parametrize("noisy", [False, True], ids=["clean", "poisson"])
def test_recipe_finds_every_bead_in_its_voxel(shape, n_beads, noisy):
    """Beads of sigma (1, 1, 3), amplitude 1000, >= 12 voxels apart and >= 8 from every face; default sigmas, threshold 5.  As many
    detections as beads and one within 0.5 voxel of each: the 0.5 is a condition, not a measurement (a float32 run over five seeds
    found 0.094 clean and 0.115 noisy at the most)."""
    rng = np.random.default_rng(7 + n_beads)
    pts = R.draw_positions(shape, n_beads, rng)
    img = R.render_beads(shape, pts)
    if noisy:
        img = R.add_poisson(img, rng)
    peaks, D = R.detect(img, threshold=5)
    dist = R.nearest(pts, peaks["pos"])
    print(f"{len(peaks)} detections of {n_beads} beads, largest distance {dist.max():.4f}, flags {sorted(set(peaks['flags'].tolist()))}")
    assert len(peaks) == n_beads
    assert np.all(dist <= 0.5)
    assert np.all(np.diff(R.find_peaks(D, 5)) > 0)


def test_half_voxel_beads_need_the_second_refusal_rule():
    """A bead centred 0.496 .. 0.506 off a voxel along z: the recipe's rule lands within 0.5 voxel (and says FROZEN where it had to
    refuse), the plain rule is left a voxel off on at least one of the positions."""
    shape = (48, 24, 24)
    plain_bad = 0
    for k in range(11):
        off = 0.496 + 0.001 * k
        p = np.array([[12.3, 12.7, 24.0 + off]])
        D = R.dog_sigmas(R.render_beads(shape, p))
        vox = R.find_peaks(D, 5)
        assert len(vox) == 1
        got = R.localise(D, vox, 4)
        d_recipe = R.nearest(p, got["pos"])[0]
        d_plain = R.nearest(p, [R.localise_plain(D, int(vox[0]), 4)])[0]
        print(f"z offset {off:.3f}: recipe {d_recipe:.4f} (flags {int(got['flags'][0])}), plain rule {d_plain:.4f}")
        assert d_recipe <= 0.5
        plain_bad += d_plain > 0.5
    assert plain_bad >= 1
