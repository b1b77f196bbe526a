"""The fused rotate + attenuate + x transform kernel with its waves split into walkers and transformers (rotate_fft.hip:
k_rotate_attenuate_fftx_roles, option fused_fftx=roles) against the kernel every wave walks and transforms in (fused_fftx=1)
and against the separate kernels (fused_fftx=0): only who does the work changes, so every output is identical bit for bit."""
import numpy as np
import pytest

SEED = 464232194

#        (nz, ny, nx)     PSF (kz, ky, kx)  degrees
CASES = [((8, 64, 64), (5, 5, 5), 33),          # one walker wave, whole batches
         ((6, 77, 70), (5, 5, 7), -52),         # inactive lanes, a partial last batch, Ny > Nx: rows the attenuation never visits
         ((5, 200, 192), (9, 9, 15), 60),       # three walkers, transformer rows wrap
         ((3, 520, 448), (3, 7, 31), 15),       # seven walkers
         ((4, 512, 512), (3, 7, 31), 15),       # the flagship's instance
         ((4, 512, 512), (3, 7, 31), 90),       # taps exactly on the grid, face rows take the masked path
         ((3, 600, 576), (3, 5, 9), 25)]        # nine waves: today's kernel under every setting
VOLUMES = ("phantom", "dense", "zero")


def _same(a, b):
    """np.array_equal on the bit patterns: an all-zero volume has no mean to adjust to, its `con` is NaN in every mode."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _volume(synth, kind, shape):
    rng = np.random.default_rng(77)
    if kind == "phantom":   # as test_fused_rotate_attenuate_x_transform_is_bit_identical builds it
        return synth.sphere_phantom(shape[2], shape[1], shape[0]) + (rng.random(shape, dtype=np.float32) < 0.02).astype(np.float32)
    if kind == "dense":
        return rng.random(shape, dtype=np.float32) + np.float32(0.01)
    return np.zeros(shape, dtype=np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("volume", VOLUMES)
@pytest.mark.parametrize("shape,kshape,degrees", CASES)
def test_walkers_and_transformers_keep_every_output(mvs, synth, shape, kshape, degrees, volume):
    gt = _volume(synth, volume, shape)
    psf = np.random.default_rng(78).random(kshape, dtype=np.float32) + 0.05
    res, stats = {}, {}
    for mode in ("roles", 1, 0):
        with mvs.Context(0) as c:
            c.set_option("fused_fftx", mode)
            p = c.view_params(degrees=degrees, inc=1, snr=25.0, seed=SEED, stream=3, conv_method=1)
            full = c.simulate_view(gt, psf.copy(), p, want=("rot", "att", "con", "acq"))
            only = c.simulate_view(gt, psf.copy(), p, want=("acq",))
            res[mode], stats[mode] = (full, only), c.plane_stats()
    for other in (1, 0):
        for k in ("rot", "att", "con", "acq"):
            assert _same(res["roles"][0][k], res[other][0][k]), (k, other)
        assert _same(res["roles"][1]["acq"], res[other][1]["acq"]), other
    # the plane flags (which planes hold a non-zero attenuated voxel) exist on the fused path only
    assert stats["roles"] == stats[1]
    if volume == "zero":
        assert stats["roles"][1] == stats["roles"][0]                       # every flagged plane is empty
        assert not res["roles"][0]["att"].any() and res["roles"][0]["acq"].shape == res[0][0]["acq"].shape
    else:
        assert float(res["roles"][0]["att"].max()) > 0
