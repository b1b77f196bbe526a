"""GPU parity: the HIP path (through the C ABI) against the CPU oracle, the committed golden
fixtures and size-independent properties at full size.  All tests need a real MI355X.

Tolerances (BASELINE.json north_star / SURVEY.md H2,H3):
  * integer / index work (extractSlices copy, Poisson counts on identical lambda): bit-exact
  * rotate / attenuate: bit-exact against the oracle's restatement of the ImgLib2 arithmetic
  * convolve (float32 FFT): max|a-b| <= 1e-5 * max|b|  (range-normalised), tolerance written below
"""
import importlib
import os

import numpy as np
import pytest

from .conftest import ROOT, rel_to_max

pytestmark = pytest.mark.gpu

CONV_TOL = 1e-5          # range-normalised, north_star "<= 1e-5"
SEED = 464232194


# ------------------------------------------------------------------------------------------------ rotate
@pytest.mark.parametrize("shape", [(9, 9, 9), (12, 14, 10), (16, 24, 20), (33, 32, 64), (5, 7, 3)])
@pytest.mark.parametrize("axis,deg", [(0, 0), (0, 15), (0, 60), (0, 90), (0, -52), (1, 37), (2, 123), (1, 180)])
def test_rotate_matches_oracle_bit_exact(ctx, orc, shape, axis, deg):
    v = np.random.default_rng(hash((shape, axis, deg)) & 0xFFFF).random(shape, dtype=np.float32)
    got = ctx.rotate_around_axis(v, axis, deg)
    want = orc.rotate_around_axis(v, axis, deg)
    assert np.array_equal(got, want), rel_to_max(got, want)


def test_rotate_strided_view_input(ctx, orc):
    """Callers pass arbitrary RAI views (SimulateTileStitching.java:152-156)."""
    big = np.random.default_rng(1).random((20, 22, 24), dtype=np.float32)
    view = big[2:18, 3:19, 4:20]
    assert np.array_equal(ctx.rotate_around_axis(view, 0, 33), orc.rotate_around_axis(view, 0, 33))


# ------------------------------------------------------------------------------------------------ attenuate
@pytest.mark.parametrize("shape", [(8, 8, 8), (5, 64, 64), (3, 70, 70), (4, 40, 17), (6, 16, 16)])
@pytest.mark.parametrize("delta", [0.0, 0.01, 0.3])
def test_attenuate_matches_oracle_bit_exact(ctx, orc, shape, delta):
    v = np.random.default_rng(2).random(shape, dtype=np.float32) * 4
    assert np.array_equal(ctx.attenuate3d(v, delta), orc.attenuate3d(v, delta))


def test_attenuate_rejects_nx_gt_ny(ctx):
    with pytest.raises(ValueError):
        ctx.attenuate3d(np.ones((2, 4, 8), np.float32), 0.01)


# ------------------------------------------------------------------------------------------------ convolve
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("shape,kshape", [((20, 20, 20), (9, 5, 7)), ((16, 24, 32), (5, 5, 5)), ((24, 17, 19), (3, 7, 5)),
                                          ((12, 12, 12), (4, 6, 2)), ((8, 8, 8), (15, 15, 15)), ((10, 1, 13), (3, 1, 5))])
def test_convolve_matches_oracle(ctx, orc, synth, method, shape, kshape):
    rng = np.random.default_rng(3)
    v = rng.random(shape, dtype=np.float32)
    psf = rng.random(kshape, dtype=np.float32) + 0.01
    p1, p2 = psf.copy(), psf.copy()
    got = ctx.convolve(v, p1, method=method)
    want = orc.convolve_direct(v, p2)
    assert rel_to_max(got, want) <= CONV_TOL
    # PSF normalised in place (Q5), same values as Tools.normImage would leave
    assert np.allclose(p1, p2, rtol=0, atol=1e-9) and abs(float(p1.astype(np.float64).sum()) - 1) < 1e-6


@pytest.mark.parametrize("shape,kshape", [((33, 100, 66), (8, 13, 15)),     # padded 40 (5*8), 112 (7*4*4), 2*40
                                          ((130, 50, 270), (11, 7, 11)),    # padded 140 (7*5*4), 56 (7*8), 2*140
                                          ((150, 36, 40), (11, 5, 9))])     # padded 160 (5*8*4), 40, 2*24
def test_convolve_radix5_7_sizes(ctx, orc, shape, kshape):
    rng = np.random.default_rng(13)
    v = rng.random(shape, dtype=np.float32)
    psf = rng.random(kshape, dtype=np.float32) + 0.01
    got = ctx.convolve(v, psf.copy(), method=1)
    want = orc.convolve_fft(v, psf.copy())          # float32 FFT restatement (the direct sum is slow at these sizes)
    assert rel_to_max(got, want) <= CONV_TOL
    got2 = ctx.convolve(v, psf.copy(), method=2)    # and the FFT-independent stencil
    assert rel_to_max(got, got2) <= CONV_TOL


@pytest.mark.parametrize("shape,kshape,zpass", [((8, 1040, 1040), (3, 15, 15), "auto"),      # x: 2 * 540 (9*5*4*3), y: 1080 (9*8*5*3)
                                                ((1040, 20, 24), (15, 5, 5), "fft"),          # z: 1080 through the FFT z pass
                                                ((300, 20, 24), (51, 5, 5), "fft"),           # z: 350 (7*10*5)
                                                ((8, 300, 310), (3, 51, 51), "auto")])        # x: 2 * 180 (9*5*4), y: 350
def test_convolve_sizes_added_in_round_4(ctx, orc, options, shape, kshape, zpass):
    """The padded lengths a 1024-voxel axis takes with PSFs of up to 57 taps (1024 + 30 = 1054 -> 1080 instead of 1120; configs[3])."""
    rng = np.random.default_rng(17)
    v = rng.random(shape, dtype=np.float32)
    psf = rng.random(kshape, dtype=np.float32) + 0.01
    options(fft_zpass=zpass)
    got = ctx.convolve(v, psf.copy(), method=1)
    want = orc.convolve_fft(v, psf.copy())
    assert rel_to_max(got, want) <= CONV_TOL


@pytest.mark.parametrize("method", [1, 2])
def test_convolve_delta_shift_kat(ctx, method):
    v = np.random.default_rng(4).random((10, 11, 12), dtype=np.float32)
    psf = np.zeros((5, 5, 5), np.float32)
    s = (1, -2, 2)
    psf[2 + s[0], 2 + s[1], 2 + s[2]] = 3.0
    out = ctx.convolve(v, psf, method=method)
    idx = [np.arange(n) - d for n, d in zip(v.shape, s)]
    idx = [np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i)) for i, n in zip(idx, v.shape)]
    assert rel_to_max(out, v[np.ix_(*idx)]) <= 2e-6


def test_convolve_phantom_gaussian_64(ctx, orc, synth):
    v = synth.sphere_phantom(64)
    psf = synth.gaussian_psf(15, sigma=(2, 2, 2))
    got = ctx.convolve(v, psf.copy(), method=1)
    want = orc.convolve_direct(v, psf.copy())
    assert rel_to_max(got, want) <= CONV_TOL
    rel = np.abs(got - want)[want >= 1e-2 * want.max()] / want[want >= 1e-2 * want.max()]
    assert rel.max() <= 1e-4          # per-voxel relative where the signal is (H2)
    got2 = ctx.convolve(v, psf.copy(), method=2)
    assert rel_to_max(got2, want) <= CONV_TOL


@pytest.mark.parametrize("shape,kshape", [((40, 70, 50), (29, 17, 33)),      # PSF chunked in y AND z, 9 groups of 4 x taps
                                          ((21, 30, 45), (64, 2, 11)),      # the deepest PSF the kernel takes; volume thinner than the PSF
                                          ((18, 18, 70), (7, 64, 64))])     # 64 taps along x and y (KXP = 64: the largest instance)
def test_stencil_chunked_psf_matches_oracle(ctx, orc, shape, kshape):
    """The direct stencil cuts the PSF into (y, z) chunks that fit half a CU's LDS (stencil.hip: stencil_geometry); every
    chunk boundary, the mirror halo on all faces and volumes smaller than the PSF against the exact direct sum."""
    rng = np.random.default_rng(31)
    v = rng.random(shape, dtype=np.float32)
    psf = rng.random(kshape, dtype=np.float32) + 0.01
    got = ctx.convolve(v, psf.copy(), method=2)
    want = orc.convolve_direct(v, psf.copy())
    assert rel_to_max(got, want) <= CONV_TOL


def test_stencil_rejects_more_than_64_taps(ctx):
    with pytest.raises(ValueError):
        ctx.convolve(np.ones((8, 8, 8), np.float32), np.ones((3, 3, 65), np.float32), method=2)


@pytest.mark.parametrize("psf_kind", ["measured_like_51", "hourglass_63"])
def test_stencil_takes_the_psfs_the_path_uses(ctx, orc, synth, psf_kind):
    """SimulateMultiViewDataset.java:579 loads 51^3 PSF stacks and BASELINE configs[4] names the direct stencil for a
    measured, non-separable 63^3 PSF: method=2 on a 256 x 256 x 64 sub-volume of a sphere phantom against (a) the exact
    fp64 direct sum of the oracle at sampled voxels -- two corner blocks, where all three mirror boundaries act, plus
    random voxels -- and (b) the FFT path on the whole sub-volume.  Tolerance 1e-5, range-normalised."""
    v = np.ascontiguousarray(synth.sphere_phantom(256)[96:160])
    psf = synth.measured_like_psf(51) if psf_kind == "measured_like_51" else synth.hourglass_psf(63)
    p2 = psf.copy()
    got2 = ctx.convolve(v, p2, method=2)
    got1 = ctx.convolve(v, psf.copy(), method=1)
    scale = float(np.abs(got1).max())
    assert scale > 0 and rel_to_max(got2, got1) <= CONV_TOL
    nz, ny, nx = v.shape
    zz, yy, xx = np.meshgrid(np.arange(3), np.arange(6), np.arange(40), indexing="ij")
    corner = (xx + nx * (yy + ny * zz)).ravel()
    far = ((nx - 1 - xx) + nx * ((ny - 1 - yy) + ny * (nz - 1 - zz))).ravel()
    rnd = np.random.default_rng(7).integers(0, v.size, 1500)
    bright = np.flatnonzero(got1.ravel() > 0.25 * scale)[::997][:500]
    idx = np.unique(np.concatenate([corner, far, rnd, bright]))
    want = orc.convolve_direct_at(v, p2, idx)            # p2 was normalised in place by the call above (Q5)
    assert float(np.abs(want).max()) > 0.1 * scale
    assert float(np.abs(got2.ravel()[idx] - want).max()) <= CONV_TOL * scale
    assert float(np.abs(got1.ravel()[idx] - want).max()) <= CONV_TOL * scale


def test_stencil_at_config1_size_against_fft_and_sampled_oracle(ctx, orc, synth):
    """The direct stencil on a whole BASELINE configs[1] volume (512^3, 31^3 anisotropic Gaussian; 8 Tflop, ~0.1 s): against
    the FFT passes on every voxel and against the oracle's exact fp64 direct sum at 3 000 sampled voxels (boundary blocks at
    two opposite corners, random and bright voxels).  1e-5 of the range, as everywhere."""
    v = synth.sphere_phantom(512)
    psf = synth.gaussian_psf(31, sigma=(2.0, 2.2, 6.0))
    p2 = psf.copy()
    got2 = ctx.convolve(v, p2, method=2)
    got1 = ctx.convolve(v, psf.copy(), method=1)
    scale = float(np.abs(got1).max())
    assert scale > 0
    # chunked comparison: no 512 MB temporaries beyond the two results
    worst = max(float(np.abs(got2[z0:z0 + 64] - got1[z0:z0 + 64]).max()) for z0 in range(0, 512, 64))
    assert worst <= CONV_TOL * scale
    nz, ny, nx = v.shape
    zz, yy, xx = np.meshgrid(np.arange(4), np.arange(8), np.arange(24), indexing="ij")
    corner = (xx + nx * (yy + ny * zz)).ravel()
    far = ((nx - 1 - xx) + nx * ((ny - 1 - yy) + ny * (nz - 1 - zz))).ravel()
    rnd = np.random.default_rng(11).integers(0, v.size, 1200)
    bright = np.flatnonzero(got1[200:312].ravel() > 0.25 * scale)[::4001][:300] + 200 * ny * nx
    idx = np.unique(np.concatenate([corner, far, rnd, bright]))
    want = orc.convolve_direct_at(v, p2, idx)
    assert float(np.abs(got2.ravel()[idx] - want).max()) <= CONV_TOL * scale
    assert float(np.abs(got1.ravel()[idx] - want).max()) <= CONV_TOL * scale


# ------------------------------------------------------------------------------------------------ adjust / norm
def test_adjust_and_norm_match_oracle(ctx, orc):
    rng = np.random.default_rng(5)
    a = rng.random((20, 21, 22), dtype=np.float32) * 2
    b = a.copy()
    c1 = ctx.adjust_image(a, 1e-4, 1.0)
    c2 = orc.adjust_image(b, 1e-4, 1.0)
    assert abs(c1 - c2) <= 4e-16 * c2
    # two-rounding rule reproduced; a 1-ulp-of-double wobble in corr may flip isolated float roundings
    assert np.mean(a != b) < 1e-4 and np.max(np.abs(a - b) / b) <= 1.2e-7
    p, q = rng.random((7, 7, 7), dtype=np.float32), None
    q = p.copy()
    ctx.norm_image(p)
    orc.norm_image(q)
    assert np.max(np.abs(p - q) / q) <= 1.2e-7


# ------------------------------------------------------------------------------------------------ extract / Poisson
@pytest.mark.parametrize("inc", [1, 2, 3, 4, 7, 100])
def test_extract_copy_bit_exact(ctx, inc):
    v = np.random.default_rng(6).random((13, 10, 12), dtype=np.float32)
    out = ctx.extract_slices(v, inc, -1.0, 0)
    assert out.shape == ((13 - 1) // inc + 1, 10, 12) and np.array_equal(out, v[::inc])


def test_extract_invalid_inc(ctx):
    with pytest.raises(ValueError):
        ctx.extract_slices(np.zeros((4, 4, 4), np.float32), 0, 25.0, 1)


@pytest.mark.parametrize("inc,stream", [(1, 0), (3, 5)])
def test_poisson_counts_bit_exact_on_identical_lambda(ctx, orc, inc, stream):
    rng = np.random.default_rng(7)
    # lambda spans both sampler branches: background 1e-4 .. bright ~ 180 (x125) plus zeros/negatives
    v = (rng.random((9, 32, 32), dtype=np.float32) ** 6) * 180
    v[0, 0, :8] = [0.0, -1.0, 1e-4, 0.0799, 0.08, 0.0801, 50.0, 1e-30]
    got = ctx.extract_slices(v, inc, 25.0, SEED, stream)
    want = orc.extract_slices_counter(v, inc, 25.0, SEED, stream)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("lo,hi", [(-3, 4), (1, 7), (6, 11)])
def test_poisson_counts_bit_exact_over_the_lambda_range(ctx, orc, lo, hi):
    """lambda log-uniform over decades (10^lo .. 10^hi): the single-precision squeeze of phase 1 (guard bands scaled with
    sqrt(lambda); off above 1e9), the pair compaction, the inversion shortcut and the resolver against the oracle's
    plain fp64 recipe -- identical counts, whatever the magnitude."""
    rng = np.random.default_rng(70 + lo)
    mul = orc.poisson_mul(25.0)
    lam = 10.0 ** rng.uniform(lo, hi, size=(32, 64, 64))
    v = (lam / mul).astype(np.float32)
    v[3, :, ::7] = 0.0                                         # holes inside bright pairs / groups
    v[5, ::3, :] = np.float32(10.0 / mul)                      # the regime boundary itself
    got = ctx.extract_slices(v, 1, 25.0, SEED, 4)
    want = orc.extract_slices_counter(v, 1, 25.0, SEED, 4)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("shape,inc", [((24, 64, 64), 1), ((25, 61, 63), 1), ((25, 61, 63), 3), ((31, 64, 64), 2)])
def test_poisson_queue_share_keeps_the_counts(ctx, orc, shape, inc):
    """Option poisson_queue_share: a work queue whose per-block segments hold 1/16 of the block's voxels instead of all of them.  What a
    full segment refuses is marked in the output and sampled where it stands by k_poisson_refused: same (voxel, attempt) arithmetic, so the
    counts equal the oracle's and the full queue's, voxel for voxel -- on volumes built to overflow it (every voxel pending in the
    inversion regime; every voxel bright at lambda ~ 10, where the attempt-0 squeeze settles about a third), through the 16-byte kernel
    (64 x 64 planes) and the group-by-group one (63 x 61).  The statistics say the path was really taken."""
    rng = np.random.default_rng(5 + inc)
    mul = orc.poisson_mul(25.0)
    lam = np.empty(shape)
    lam[: shape[0] // 3] = rng.uniform(1.5, 9.5, size=lam[: shape[0] // 3].shape)             # inversion regime, never the shortcut
    lam[shape[0] // 3: 2 * shape[0] // 3] = rng.uniform(10.0, 14.0, size=lam[shape[0] // 3: 2 * shape[0] // 3].shape)
    lam[2 * shape[0] // 3:] = 10.0 ** rng.uniform(-2, 4, size=lam[2 * shape[0] // 3:].shape)
    v = (lam / mul).astype(np.float32)
    v[1, ::5, ::3] = 0.0
    want = orc.extract_slices_counter(v, inc, 25.0, SEED, 3)
    stats = {}
    try:
        for share in (16, 1, 4):
            ctx.set_option("poisson_queue_share", share)
            got = ctx.extract_slices(v, inc, 25.0, SEED, 3)
            assert np.array_equal(got, want), share
            stats[share] = ctx.queue_stats()
    finally:
        ctx.set_option("poisson_queue_share", 16)
    full, tight = stats[16], stats[1]
    assert full["refused"] == 0 and full["bright"] + full["inversion"] > 0.3 * want.size
    assert tight["refused"] > 0 and tight["segment_items"] * 8 <= full["segment_items"]
    # every pending voxel is either in the queue or refused: the two builds settle the same voxels
    assert tight["bright"] + tight["inversion"] + tight["refused"] == full["bright"] + full["inversion"]
    assert stats[4]["refused"] > 0 and stats[4]["refused"] < tight["refused"]


def test_poisson_queue_grows_to_what_the_views_need(mvs):
    """Option poisson_queue_share=auto: a context starts its queue at 5 sixteenths of the full size (queues above 64 MiB), a view whose blocks have more
    pending than that still gets the right counts -- the third kernel samples what was refused --, leaves what it would have needed in a
    page-locked word, and the context's NEXT view is given that much: no refusals from then on.  A volume of 5 M voxels with every voxel
    at lambda ~ 11 (about two thirds of them wait for the resolver) against the same counts from a full-size queue."""
    rng = np.random.default_rng(11)
    v = (rng.uniform(10.5, 11.5, size=(160, 176, 176)) / 124.99999999999997).astype(np.float32)
    with mvs.Context(0) as c:
        want = c.extract_slices(v, 1, 25.0, 99, 1)                  # the default: every voxel of a block fits its segment
        full = c.queue_stats()
    assert full["refused"] == 0 and full["bright"] > 0.5 * v.size
    with mvs.Context(0) as c:                                      # a fresh context: nothing learned yet
        c.set_option("poisson_queue_share", "auto")
        first = c.extract_slices(v, 1, 25.0, 99, 1)
        st1 = c.queue_stats()
        second = c.extract_slices(v, 1, 25.0, 99, 1)
        st2 = c.queue_stats()
    assert np.array_equal(first, want) and np.array_equal(second, want)
    assert st1["refused"] > 0 and st1["segment_items"] * 16 == 5 * full["segment_items"] and st1["bytes"] < 0.4 * full["bytes"]
    assert st2["refused"] == 0 and st1["segment_items"] < st2["segment_items"] <= full["segment_items"]
    assert st2["segment_items"] >= st2["fullest_block"] == full["fullest_block"]


def test_poisson_queue_share_in_whole_views(ctx, synth):
    """The same through the view pipeline, one view at a time and stacked: shares 1 and 16 give identical acquisitions (the queue's size
    is invisible in the result), for a plane size that is a multiple of four voxels and one that is not."""
    for n in (48, 45):
        gt = synth.sphere_phantom(n) + np.float32(0.5)             # no empty voxel: every voxel of the view is bright at this SNR
        psf = synth.gaussian_psf(7)
        ps = [ctx.view_params(axis=0, degrees=d, delta=0.01, min_value=0.0, target_average=1.0, inc=2, snr=14.0, seed=7 + d, stream=i)
              for i, d in enumerate((0, 90, 135))]
        res = {}
        try:
            for share in (16, 1):
                ctx.set_option("poisson_queue_share", share)
                seq = [ctx.simulate_view(gt, psf.copy(), p)["acq"] for p in ps]
                stacked = ctx.simulate_views(gt, [psf.copy() for _ in ps], ps)
                for a, b in zip(seq, stacked):
                    assert np.array_equal(a, b)
                res[share] = seq
                if share == 1:
                    assert ctx.queue_stats()["refused"] > 0
        finally:
            ctx.set_option("poisson_queue_share", 16)
        for a, b in zip(res[16], res[1]):
            assert np.array_equal(a, b)


def test_poisson_process_in_place_and_offsets(ctx, orc):
    rng = np.random.default_rng(8)
    img = rng.random((40, 50), dtype=np.float32) * 2
    a = img.copy()
    ctx.poisson_process(a, 25.0, 99, stream=2, index_offset=1000)
    mul = orc.poisson_mul(25.0)
    want = np.array([orc.poisson_counter(float(x) * mul, 99, 2, 1000 + i) for i, x in enumerate(img.ravel())],
                    np.float32).reshape(img.shape)
    assert np.array_equal(a, want)


@pytest.mark.parametrize("lam", [0.0125, 1.0, 9.99, 10.0, 125.0, 4000.0, 22000.0])
def test_poisson_distribution_moments(ctx, lam):
    n = 1 << 20
    mul = 124.99999999999997
    img = np.full(n, lam / mul, np.float32)
    lam_eff = float(np.float64(img[0]) * mul)
    ctx.poisson_process(img, 25.0, 4242)
    m, var = img.astype(np.float64).mean(), img.astype(np.float64).var()
    assert abs(m - lam_eff) < 5 * np.sqrt(lam_eff / n)
    assert abs(var - lam_eff) < 5 * lam_eff * np.sqrt(2.0 / n + 1.0 / (lam_eff * n))
    assert np.all(img == np.round(img)) and img.min() >= 0


def test_poisson_matches_reference_sampler_distribution(ctx, orc):
    """HIP sampler vs the reference's own inter-arrival sampler on java.util.Random (chi-square)."""
    for lam in (3.0, 30.0):
        n = 200000
        img = np.full(n, lam / 124.99999999999997, np.float32)
        lam_eff = float(np.float64(img[0]) * 124.99999999999997)
        ctx.poisson_process(img, 25.0, 31337)
        r = orc.JRandom(SEED)
        ref = np.array([r.poisson(lam_eff) for _ in range(n)])
        hi = int(lam + 8 * np.sqrt(lam))
        ha = np.bincount(np.minimum(img.astype(int), hi), minlength=hi + 1).astype(float)
        hb = np.bincount(np.minimum(ref, hi), minlength=hi + 1).astype(float)
        msk = (ha + hb) > 20
        chi2 = np.sum((ha[msk] - hb[msk]) ** 2 / (ha[msk] + hb[msk]))
        assert chi2 < msk.sum() + 6 * np.sqrt(2 * msk.sum()), (lam, chi2, msk.sum())


# ------------------------------------------------------------------------------------------------ next items
def test_make_isotropic_and_weight_image(ctx, orc):
    v = np.random.default_rng(9).random((7, 6, 5), dtype=np.float32)
    for inc in (1, 3, 4):
        assert np.array_equal(ctx.make_isotropic(v, inc), orc.make_isotropic(v, inc))
    w = ctx.compute_weight_image((3, 100, 4))
    assert np.max(np.abs(w - orc.compute_weight_image((3, 100, 4)))) <= 6e-8


# ------------------------------------------------------------------------------------------------ phantom (8f rank 3)
@pytest.mark.parametrize("canvas,scale,half", [(160, 1, False), (160, 1, True), (260, 2, False), (150, 1, False)])
def test_draw_spheres_bit_exact_and_random_stream(ctx, mvs, orc, canvas, scale, half):
    """SMVD:436-522: same spheres, same voxels, same java.util.Random state afterwards as the oracle."""
    seed = 464232194
    a = np.zeros((canvas,) * 3, np.float32)
    ro = orc.JRandom(seed)
    n_o = orc.draw_spheres(a, 0.0, 1.0, scale, half, ro)
    b = np.zeros_like(a)
    rg = mvs.JavaRandom(seed)
    n_g = ctx.draw_spheres(b, 0.0, 1.0, scale, half, rg)
    assert n_g == n_o and n_o > 10
    assert rg._s == int(ro.st.s)
    assert np.array_equal(a, b)
    # a second call continues the same random stream and composites on top (Math.max)
    n_o2 = orc.draw_spheres(a, 0.25, 0.75, scale, half, ro)
    n_g2 = ctx.draw_spheres(b, 0.25, 0.75, scale, half, rg)
    assert n_g2 == n_o2 and rg._s == int(ro.st.s) and np.array_equal(a, b)


def test_draw_spheres_non_cubic_and_negative_canvas(ctx, mvs, orc):
    a = np.full((140, 150, 170), -0.5, np.float32)          # mixed signs exercise both branches of the atomic max
    b = a.copy()
    ro, rg = orc.JRandom(7), mvs.JavaRandom(7)
    assert orc.draw_spheres(a, -1.0, 1.0, 1, False, ro) == ctx.draw_spheres(b, -1.0, 1.0, 1, False, rg)
    assert np.array_equal(a, b) and (b > 0).any() and (b[b != -0.5] > -0.5).all()
    with pytest.raises(ValueError):
        ctx.draw_spheres(np.zeros((64, 64, 64), np.float32), 0.0, 1.0, 1, False, mvs.JavaRandom(1))   # radius < 0


@pytest.mark.parametrize("shape", [(10, 13, 16), (9, 8, 21), (64, 64, 64)])
def test_downsample2x_bit_exact(ctx, orc, shape):
    v = np.random.default_rng(31).random(shape, dtype=np.float32)
    got = ctx.downsample2x(v)
    assert got.shape == tuple(s // 2 - 1 for s in shape)
    assert np.array_equal(got, orc.downsample2x(v))


def test_golden_phantom_fixture(ctx, mvs, golden_dir):
    import hashlib
    import json
    g = json.load(open(os.path.join(golden_dir, "phantom_vectors.json")))
    img = np.zeros((g["canvas"],) * 3, np.float32)
    r = mvs.JavaRandom(g["seed"])
    assert ctx.draw_spheres(img, 0.0, 1.0, g["scale"], False, r) == g["n_spheres"]
    assert r._s == g["rnd_state_after"]
    assert hashlib.sha256(img.tobytes()).hexdigest() == g["canvas_sha256"]
    assert hashlib.sha256(ctx.downsample2x(img).tobytes()).hexdigest() == g["downsampled_sha256"]


def test_simulate_phantom_full_size(mvs, orc):
    """`simulate()` (SMVD:366-392) at the reference's size: 580^3 canvas in HBM, 289^3 result; bit-exact against
    the oracle, and the facade's static generator continues like the reference's static `rnd`."""
    S = mvs.SimulateMultiViewDataset
    r = mvs.JavaRandom(464232194)
    got = S.simulate(False, r)
    assert got.shape == (289, 289, 289) and got.dtype == np.float32
    ro = orc.JRandom(464232194)
    ref = orc.simulate_phantom(rnd=ro)
    assert r._s == int(ro.st.s)
    assert np.array_equal(got, ref)
    assert 0.1 < float((got > 0).mean()) < 0.3 and float(got.max()) < 1.0


def test_reference_configuration_view(ctx, mvs, orc, psf51_tif):
    """The reference's own run (SimulateMultiViewDataset.main, :524-613): 289^3 sphere phantom from `simulate()`, a
    51^3 PSF stack `Angle0.tif` through Tools.open(file, true) (synthesised: the shipped stacks are GPL data), first
    view of `main` (angle 0 + offset 15, spacing 3, SNR 25, attenuation = 0.01f widened to double)."""
    S, T = mvs.SimulateMultiViewDataset, mvs.Tools
    rendered = S.simulate(False, mvs.JavaRandom(464232194))
    psf_raw = T.open(psf51_tif, True)
    assert rendered.shape == (289, 289, 289) and psf_raw.shape == (51, 51, 51)
    delta = float(np.float32(0.01))                                       # SMVD:533,573
    p = ctx.view_params(degrees=15, inc=3, snr=25.0, seed=464232194, stream=0)
    assert p.delta == delta                                               # the C default is the reference's value
    psf_g = psf_raw.copy()
    got = ctx.simulate_view(rendered, psf_g, p, want=("rot", "att", "con", "acq"))
    psf_o = psf_raw.copy()
    ref = orc.simulate_view(rendered, psf_o, 15, delta=delta, inc=3, snr=25.0, seed=464232194, stream=0, conv="fft")
    assert np.array_equal(psf_g, psf_o)                                   # normalised in place, identically
    assert np.array_equal(got["rot"], ref["rot"]) and np.array_equal(got["att"], ref["att"])
    assert rel_to_max(got["con"], ref["con"]) <= CONV_TOL
    assert got["acq"].shape == ref["acq"].shape == (97, 289, 289)
    # counts differ only where the 1e-7 wobble of `con` crosses a decision boundary of the sampler (a flipped
    # rejection test draws a fresh candidate, so a differing count may differ by a whole Poisson deviation)
    diff = got["acq"] != ref["acq"]
    assert diff.mean() < 0.01
    lam = np.maximum(ref["acq"][diff], 1.0)
    assert np.all(np.abs(got["acq"][diff] - ref["acq"][diff]) <= 8.0 * np.sqrt(lam) + 8.0)
    assert abs(float(got["acq"].mean()) - float(ref["acq"].mean())) < 0.02


def test_simulate_tile_stitching_pair(mvs, orc, psf51_tif):
    """SimulateTileStitching.java:43-246 at the reference's size: phantom from `new Random(rnd.nextInt())`, no
    rotation, 51^3 PSF; tiles are sub-intervals of the convolved volume run through extractSlices."""
    S, T = mvs.SimulateMultiViewDataset, mvs.Tools
    psf = T.open(psf51_tif, True)
    sts = mvs.SimulateTileStitching(mvs.JavaRandom(5), True, (0.2, 0.2, 0.2), None, psf=psf.copy())
    assert sts.con.shape == sts.conHalfPixel.shape == (289, 289, 289)
    assert sts.overlap == [29, 29, 29]                                   # round(289 * 0.2 / 2)
    assert sts.getInterval(0) == ([0, 0, 0], [173, 173, 173]) and sts.getInterval(1) == ([115, 115, 115], [288, 288, 288])
    assert sts.getCorrectTranslation() == [114.5, 114.5, 115 / 3]
    # the convolved phantom against the oracle's composition of the same calls
    j = mvs.JavaRandom(5)
    seed = j.nextInt()
    gt = orc.simulate_phantom(rnd=orc.JRandom(seed))
    po = psf.copy()
    con = orc.convolve_fft(orc.attenuate3d(gt, float(np.float32(0.01))), po)
    orc.adjust_image(con, 1e-4, 1.0)
    assert rel_to_max(sts.con, con) <= CONV_TOL
    # half-pixel variant: every small sphere moved by (+1, +1, 0) on the 2x canvas
    assert not np.array_equal(sts.con, sts.conHalfPixel)
    left, right = sts.getNextPair(-1.0)                                  # snr < 0: plain strided copies of the tiles
    assert left.shape == (58, 174, 174) and right.shape == (58, 174, 174)
    assert np.array_equal(left, sts.con[0:174:3, 0:174, 0:174])
    assert np.array_equal(right, sts.conHalfPixel[115:289:3, 115:289, 115:289])
    l8, r8 = sts.getNextPair(8.0)                                        # the reference's main(): snr = 8
    mul = (8.0 / np.sqrt(5.0)) ** 2
    assert l8.shape == left.shape and np.all(l8 == np.round(l8)) and abs(l8.mean() / (left.mean() * mul) - 1) < 0.01
    assert abs(r8.mean() / (right.mean() * mul) - 1) < 0.01
    l8b, _ = sts.getNextPair(8.0)                                        # next pair: new seeds from the same generator
    assert not np.array_equal(l8, l8b)


# ------------------------------------------------------------------------------------------------ BASELINE configs at size
REF_DELTA = float(np.float32(0.01))      # `final float attenuation = 0.01f` widened to double (SMVD:533,573)


def _view_against_oracle(ctx, orc, gt, psf_raw, degrees, inc, stream):
    """One fused view against the oracle's composition of the same stages: rot/att bit-exact, con within the 1e-5
    contract, and -- Poisson being discontinuous in lambda -- the counts bit-exact on IDENTICAL lambda, i.e. the oracle's
    second implementation of the sampler run on the GPU's own adjusted `con`."""
    p = ctx.view_params(degrees=degrees, delta=REF_DELTA, inc=inc, snr=25.0, seed=SEED, stream=stream, conv_method=1)
    psf_g, psf_o = psf_raw.copy(), psf_raw.copy()
    got = ctx.simulate_view(gt, psf_g, p, want=("rot", "att", "con", "acq"))
    ref = orc.simulate_view(gt, psf_o, degrees, delta=REF_DELTA, inc=inc, snr=25.0, seed=SEED, stream=stream, conv="fft")
    assert np.array_equal(psf_g, psf_o)
    assert np.array_equal(got["rot"], ref["rot"]) and np.array_equal(got["att"], ref["att"])
    assert rel_to_max(got["con"], ref["con"]) <= CONV_TOL
    assert abs(got["corr"] - ref["corr"]) <= 1e-6 * ref["corr"]
    acq_same_lambda = orc.extract_slices_counter(got["con"], inc, 25.0, SEED, stream)
    assert got["acq"].shape == acq_same_lambda.shape
    assert np.array_equal(got["acq"], acq_same_lambda)
    # and end to end: the 1e-7 wobble of `con` moves a small fraction of the counts
    assert (got["acq"] != ref["acq"]).mean() < 0.01
    return got, ref


def test_config0_128_cubed_psf15_view_matches_oracle(ctx, orc, synth):
    """BASELINE configs[0] at its real size: 128^3 float volume, 1 view, 15^3 Gaussian PSF, FFT convolution + Poisson
    (the reference runs it on the host JVM; here the same view on the GPU against the CPU oracle)."""
    gt = synth.sphere_phantom(128)
    psf = synth.gaussian_psf(15, sigma=(2.0, 2.0, 2.0))
    got, _ = _view_against_oracle(ctx, orc, gt, psf, degrees=15, inc=1, stream=0)
    assert got["acq"].shape == (128, 128, 128)
    lam = got["con"].astype(np.float64) * 124.99999999999997
    assert (lam >= 10.0).mean() > 0.02 and (lam < 1.0).mean() > 0.5       # both sampler regimes are populated


def test_full_width_512x512x64_view_matches_oracle(ctx, orc, synth):
    """A full-width slab of the headline workload (the central 64 planes of the 512^3 phantom, 31^3 PSF): 1.6e7 voxels
    through the production kernels (fused rotate+attenuate, hand-written FFT passes at 560 x 560, work-queue Poisson),
    counts bit-exact on identical lambda.  Rotation by 15 degrees keeps half of the thin slab inside the volume, so the
    lambda histogram has the bright tail of the real workload; 60 degrees is covered at 512^3 by the property test."""
    full = np.ascontiguousarray(synth.sphere_phantom(512)[224:288])
    assert full.shape == (64, 512, 512)
    psf = synth.gaussian_psf(31, sigma=(2.0, 2.2, 6.0))
    got, _ = _view_against_oracle(ctx, orc, full, psf, degrees=15, inc=1, stream=2)
    assert got["acq"].size >= 1.6e7
    lam = got["con"].astype(np.float64) * 124.99999999999997
    assert (lam >= 10.0).mean() > 0.1 and lam.max() > 500.0


def test_context_options_select_identical_variants(ctx, orc, synth, options):
    """mvsim_set_option: separate rotate and attenuate kernels, single-launch Poisson and the sum taken from pass E
    give the same voxels as the production variants (fp64-defined or integer arithmetic: bit-identical)."""
    gt = synth.sphere_phantom(48)
    psf = synth.gaussian_psf(9, sigma=(1.2, 1.4, 2.5))
    p = ctx.view_params(degrees=33, delta=REF_DELTA, inc=2, snr=25.0, seed=SEED, stream=2, conv_method=1)
    a = ctx.simulate_view(gt, psf.copy(), p, want=("rot", "att", "con", "acq"))
    options(fused_rotate=0)
    b = ctx.simulate_view(gt, psf.copy(), p, want=("rot", "att", "con", "acq"))
    options(fused_rotate=1, poisson_queue=0)
    c = ctx.simulate_view(gt, psf.copy(), p, want=("rot", "att", "con", "acq"))
    options(fused_rotate="auto", poisson_queue=1, psf_overlap=1)      # PSF spectrum on the side stream (taken from 2^24 voxels up)
    d = ctx.simulate_view(gt, psf.copy(), p, want=("rot", "att", "con", "acq"))
    for k in ("rot", "att", "con", "acq"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]) and np.array_equal(a[k], d[k]), k
    with pytest.raises(ValueError):
        ctx.set_option("fft_zpass", "sideways")
    with pytest.raises(ValueError):
        ctx.set_option("no_such_switch", 1)


# ------------------------------------------------------------------------------------------------ fused view + golden
def test_golden_view_fixture(ctx, golden_dir):
    g = np.load(os.path.join(golden_dir, "view_24.npz"))
    psf = g["psf_raw"].copy()
    p = ctx.view_params(degrees=int(g["degrees"]), delta=float(g["delta"]), inc=int(g["inc"]), snr=float(g["snr"]),
                        seed=int(g["seed"]), stream=int(g["stream"]), conv_method=1)
    res = ctx.simulate_view(g["gt"], psf, p, want=("rot", "att", "con", "acq"))
    assert np.array_equal(res["rot"], g["rot"])
    assert np.array_equal(res["att"], g["att"])
    assert rel_to_max(res["con"], g["con"]) <= CONV_TOL
    assert abs(res["corr"] - float(g["corr"])) <= 1e-6 * float(g["corr"])
    assert np.allclose(psf, g["psf_norm"], rtol=0, atol=1e-9)
    # Poisson is discontinuous in lambda: compare on identical lambda below; here bound the flips (H3).  A flipped
    # rejection test draws a fresh candidate, so a differing count may differ by a whole Poisson deviation.
    d = np.abs(res["acq"] - g["acq"])
    assert np.mean(d > 0) < 5e-3
    assert np.all(d <= 8.0 * np.sqrt(np.maximum(g["acq"], 1.0)) + 8.0)


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("inc,snr", [(1, 25.0), (3, 25.0), (4, -1.0)])
def test_fused_view_equals_staged_ops(ctx, orc, synth, options, method, inc, snr):
    options(early_sum=0)      # adjustImage's sum from pass E: the only difference to the staged sum is its summation order
    gt = synth.sphere_phantom(32)
    psf0 = synth.gaussian_psf(7, 7, 9, sigma=(1.2, 1.4, 2.5))
    p = ctx.view_params(degrees=60, inc=inc, snr=snr, seed=SEED, stream=3, conv_method=method)
    fused = ctx.simulate_view(gt, psf0.copy(), p, want=("rot", "att", "con", "acq"))
    only = ctx.simulate_view(gt, psf0.copy(), p, want=("acq",))
    # staged through the individual entry points
    rot = ctx.rotate_around_axis(gt, 0, 60)
    att = ctx.attenuate3d(rot, p.delta)
    con = ctx.convolve(att, psf0.copy(), method=method)
    corr = ctx.adjust_image(con, 1e-4, 1.0)
    acq = ctx.extract_slices(con, inc, snr, SEED, 3)
    assert np.array_equal(fused["rot"], rot) and np.array_equal(fused["att"], att)
    # the fused path takes the mean from the convolution's crop epilogue, the staged adjustImage from its
    # own reduction: the two double sums may differ in the last bit, which can flip isolated float roundings
    assert abs(fused["corr"] - corr) <= 1e-15 * corr
    assert np.max(np.abs(fused["con"] - con) / con) <= 1.2e-7 and np.mean(fused["con"] != con) < 1e-3
    assert np.array_equal(fused["acq"], ctx.extract_slices(fused["con"], inc, snr, SEED, 3))
    assert np.array_equal(only["acq"], fused["acq"])   # un-materialised adjust path gives identical voxels
    d = np.abs(acq - fused["acq"])
    assert d.max() <= 1 and np.mean(d > 0) < 1e-3
    # and against the oracle: deterministic stages within tolerance, noise on identical lambda bit-exact
    o = orc.simulate_view(gt, psf0.copy(), 60, inc=inc, snr=snr, seed=SEED, stream=3)
    assert np.array_equal(rot, o["rot"]) and np.array_equal(att, o["att"])
    assert rel_to_max(con, o["con"]) <= CONV_TOL
    assert np.array_equal(acq, orc.extract_slices_counter(con, inc, snr, SEED, 3))


def test_reference_named_facade(mvs, orc, synth):
    S, T = mvs.SimulateMultiViewDataset, mvs.Tools
    gt = synth.sphere_phantom(24)
    rot = S.rotateAroundAxis(gt, 0, 15)
    att = S.attenuate3d(rot, 0.01)
    psf = synth.gaussian_psf(5)
    con = S.convolve(att, psf, None)
    assert abs(float(psf.astype(np.float64).sum()) - 1) < 1e-6
    corr = T.adjustImage(con, S.minValue, S.avgIntensity)
    assert corr > 0 and abs(con.astype(np.float64).mean() - 1) < 1e-5
    rnd = mvs.JavaRandom(5)
    acq = S.extractSlices(con, 3, 25.0, rnd)
    seed = mvs.JavaRandom(5).nextLong() & 0xFFFFFFFFFFFFFFFF
    assert np.array_equal(acq, orc.extract_slices_counter(con, 3, 25.0, seed, 0))
    assert np.array_equal(S.extractSlices(con, 3, -1.0), con[::3])
    iso = S.makeIsotropic(acq, 3)
    assert iso.shape[0] == (acq.shape[0] - 1) * 3 + 1
    assert S.computeWeightImage(rot).shape == rot.shape
    n = S.poissonProcess(con[0], 25.0, mvs.JavaRandom(6))
    assert n.shape == con[0].shape and np.all(n == np.round(n))


# ------------------------------------------------------------------------------------------------ full-size properties
def _dev_volume(ctx, arr):
    d = ctx.dev_alloc(arr.nbytes)
    ctx.upload(d, arr)
    return d


def test_full_size_512_properties(ctx, synth):
    """BASELINE config 2 size (512^3, 31^3 PSF): properties that need no oracle run."""
    n = 512
    dims = (n, n, n)
    rng = np.random.default_rng(10)
    gt = synth.sphere_phantom(n)
    d_gt = _dev_volume(ctx, gt)
    d_a = ctx.dev_alloc(gt.nbytes)
    d_b = ctx.dev_alloc(gt.nbytes)
    try:
        # rotate by 0 degrees is the identity, bit-exact
        ctx.rotate_around_axis_dev(d_gt, dims, 0, 0, d_a)
        assert np.array_equal(ctx.download(d_a, gt.shape), gt)
        # attenuate with delta 0 is the identity, bit-exact
        ctx.attenuate3d_dev(d_gt, dims, 0.0, d_a)
        assert np.array_equal(ctx.download(d_a, gt.shape), gt)
        # attenuation never brightens and is monotone in delta
        ctx.attenuate3d_dev(d_gt, dims, 0.01, d_a)
        att = ctx.download(d_a, gt.shape)
        assert np.all(att <= gt) and np.all(att >= 0)
        # convolution with a centred delta is the identity to FFT rounding; mass is preserved
        delta = np.zeros((31, 31, 31), np.float32)
        delta[15, 15, 15] = 2.0
        ctx.convolve_dev(d_a, dims, delta, d_b, method=1)
        con = ctx.download(d_b, gt.shape)
        assert rel_to_max(con, att) <= CONV_TOL
        psf = synth.gaussian_psf(31, sigma=(2.0, 2.2, 6.0))
        ctx.convolve_dev(d_a, dims, psf, d_b, method=1)
        con = ctx.download(d_b, gt.shape)
        # mirror boundary + normalised PSF conserve the total only approximately at the border; the phantom
        # is zero near the border, so the sums agree to float accumulation error
        assert abs(con.astype(np.float64).sum() / att.astype(np.float64).sum() - 1) < 1e-5
        assert con.min() > -1e-5 * con.max()
        # adjust: mean 1, min >= minValue-ish
        corr = ctx.adjust_image_dev(d_b, gt.size, 1e-4, 1.0)
        adj = ctx.download(d_b, gt.shape)
        assert abs(adj.astype(np.float64).mean() - 1.0) < 1e-5 and corr > 0
        # extract copy is a bit-exact strided copy; Poisson counts are integers with mean ~ lambda mean
        d_o = ctx.dev_alloc(gt.nbytes)
        try:
            ctx.extract_slices_dev(d_b, dims, 3, -1.0, 0, 0, d_o)
            nzo = (n - 1) // 3 + 1
            assert np.array_equal(ctx.download(d_o, (nzo, n, n)), adj[::3])
            ctx.extract_slices_dev(d_b, dims, 1, 25.0, SEED, 0, d_o)
            acq = ctx.download(d_o, gt.shape)
            assert np.all(acq == np.round(acq)) and acq.min() >= 0
            lam_mean = adj.astype(np.float64).mean() * 124.99999999999997
            assert abs(acq.astype(np.float64).mean() / lam_mean - 1) < 1e-3
            # determinism + stream separation
            ctx.extract_slices_dev(d_b, dims, 1, 25.0, SEED, 0, d_a)
            assert np.array_equal(ctx.download(d_a, gt.shape), acq)
        finally:
            ctx.dev_free(d_o)
    finally:
        for d in (d_gt, d_a, d_b):
            ctx.dev_free(d)
    del rng


def test_linearity_of_convolution_256(ctx, synth):
    rng = np.random.default_rng(11)
    a = rng.random((256, 256, 256), dtype=np.float32)
    b = synth.sphere_phantom(256)
    psf = synth.gaussian_psf(31, sigma=(2.0, 2.2, 6.0))
    lhs = ctx.convolve(a + b, psf.copy(), method=1)
    rhs = ctx.convolve(a, psf.copy(), method=1) + ctx.convolve(b, psf.copy(), method=1)
    assert rel_to_max(lhs, rhs) <= CONV_TOL


def test_normalize_weights_matches_oracle(ctx, mvs, orc):
    rng = np.random.default_rng(21)
    ws = [rng.random((6, 16, 20), dtype=np.float32) * (rng.random((6, 16, 20)) > 0.3) for _ in range(7)]
    ws = [np.ascontiguousarray(w, dtype=np.float32) for w in ws]
    a = [w.copy() for w in ws]
    b = [w.copy() for w in ws]
    ctx.normalize_weights(a, 3.0)
    orc.normalize_weights(b, 3.0)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    # device-resident form with an externally supplied sum (the sharded multi-GPU case)
    n = ws[0].size
    d = [ctx.dev_alloc(n * 4) for _ in ws]
    d_sum = ctx.dev_alloc(n * 4)
    try:
        for p, w in zip(d, ws):
            ctx.upload(p, w)
        ctx.sum_views_dev(d, n, d_sum)
        tot = ctx.download(d_sum, ws[0].shape)
        s = np.zeros_like(ws[0])
        for w in ws:
            s = s + w
        assert np.array_equal(tot, s)
        ctx.normalize_weights_dev(d[:3], n, 3.0, sum_dptr=d_sum)     # "this rank" owns views 0..2
        for p, y in zip(d[:3], b[:3]):
            assert np.array_equal(ctx.download(p, ws[0].shape), y)
    finally:
        for p in d + [d_sum]:
            ctx.dev_free(p)
    with pytest.raises(ValueError):
        ctx.normalize_weights([np.zeros(4, np.float32)] * 40, 3.0)


# ------------------------------------------------------------------------------------------------ edge cases
def test_degenerate_and_ragged_shapes(ctx, orc):
    """1-voxel volumes, PSFs larger than the image (multiple mirror reflections), inc beyond Nz."""
    one = np.full((1, 1, 1), 2.5, np.float32)
    p1 = np.full((1, 1, 1), 7.0, np.float32)
    assert np.array_equal(ctx.rotate_around_axis(one, 0, 37), orc.rotate_around_axis(one, 0, 37))
    assert np.array_equal(ctx.attenuate3d(one, 0.1), orc.attenuate3d(one, 0.1))
    for method in (1, 2):
        assert np.allclose(ctx.convolve(one, p1.copy(), method=method), 2.5, rtol=1e-6)
    assert np.array_equal(ctx.extract_slices(one, 5, -1.0, 0), one)
    rng = np.random.default_rng(30)
    small = rng.random((4, 5, 6), dtype=np.float32)
    big_psf = rng.random((9, 11, 13), dtype=np.float32) + 0.01
    want = orc.convolve_direct(small, big_psf.copy())
    for method in (1, 2):
        assert rel_to_max(ctx.convolve(small, big_psf.copy(), method=method), want) <= CONV_TOL
    v = rng.random((3, 6, 6), dtype=np.float32)
    assert np.array_equal(ctx.extract_slices(v, 100, -1.0, 0), v[:1])
    assert ctx.extract_slices(v, 3, 25.0, 9).shape == (1, 6, 6)


def test_fused_view_other_axes_and_odd_dims(ctx, orc):
    """axis != 0 and odd sizes take the generic rotate + separate attenuate path inside simulate_view."""
    rng = np.random.default_rng(31)
    gt = rng.random((11, 13, 9), dtype=np.float32)
    psf0 = rng.random((3, 5, 3), dtype=np.float32) + 0.05
    for axis, deg in ((1, 40), (2, -25), (0, 77)):
        p = ctx.view_params(axis=axis, degrees=deg, inc=2, snr=25.0, seed=SEED, stream=2, conv_method=1)
        res = ctx.simulate_view(gt, psf0.copy(), p, want=("rot", "att", "con", "acq"))
        rot = orc.rotate_around_axis(gt, axis, deg)
        att = orc.attenuate3d(rot, p.delta)
        assert np.array_equal(res["rot"], rot) and np.array_equal(res["att"], att)
        con = orc.convolve_direct(att, psf0.copy())
        orc.adjust_image(con, 1e-4, 1.0)
        assert rel_to_max(res["con"], con) <= CONV_TOL
        assert np.array_equal(res["acq"], orc.extract_slices_counter(res["con"], 2, 25.0, SEED, 2))


def test_context_reuse_across_sizes_and_cache_release(mvs, orc, synth):
    """Workspaces and plans regrow / are rebuilt when the same context sees different problem sizes."""
    with mvs.Context(0) as c:
        outs = []
        for n, k in ((24, 5), (40, 9), (16, 3), (40, 9)):
            v = synth.sphere_phantom(n)
            psf = synth.gaussian_psf(k, sigma=(1.0, 1.2, 1.5))
            got = c.convolve(v, psf.copy(), method=1)
            assert rel_to_max(got, orc.convolve_fft(v, psf.copy())) <= CONV_TOL
            outs.append(got)
        assert np.array_equal(outs[1], outs[3])          # same inputs, same context -> same bits
        c.release_caches()
        again = c.convolve(synth.sphere_phantom(40), synth.gaussian_psf(9, sigma=(1.0, 1.2, 1.5)), method=1)
        assert np.array_equal(again, outs[1])


def test_invalid_arguments_are_rejected(ctx):
    v = np.zeros((4, 4, 4), np.float32)
    with pytest.raises(ValueError):
        ctx.rotate_around_axis(v, 3, 10)
    with pytest.raises(ValueError):
        ctx.rotate_around_axis(np.zeros((4, 4), np.float32), 0, 10)
    with pytest.raises(ValueError):
        ctx.convolve(v, np.ones((3, 3, 3), np.float32), method=7)
    with pytest.raises(ValueError):
        ctx.make_isotropic(v, 0)
    with pytest.raises(ValueError):
        ctx.adjust_image(np.zeros((4, 4, 4), np.float64), 1e-4, 1.0)      # wrong dtype for an in-place operator
    with pytest.raises(ValueError):
        ctx.simulate_view(v, np.ones((3, 3, 3), np.float32), ctx.view_params(inc=0))


# ------------------------------------------------------------------------------------------------ alternative conv paths
@pytest.fixture
def options(ctx):
    """Run-time switches of the context (mvsim_set_option; nothing on a launch path reads the environment); the defaults
    are restored afterwards."""
    def set_(**kw):
        for k, v in kw.items():
            ctx.set_option(k, v)
    yield set_
    for k, v in (("fft_zpass", "auto"), ("fft_backend", "custom"), ("fft_pad", "auto"), ("fused_rotate", 1),
                 ("poisson_queue", 1), ("early_sum", 1), ("fuse_tail", 0), ("graph", 0), ("attenuate", "serial"), ("psf_overlap", 1), ("tail_overlap", 1),
                 ("zconv_strided", 1), ("exp", 0)):
        ctx.set_option(k, v)


@pytest.mark.parametrize("shape,kshape", [((40, 48, 56), (9, 7, 5)), ((64, 64, 64), (15, 15, 15)), ((33, 70, 45), (31, 5, 11))])
def test_convolve_fft_z_pass_and_rocfft_fallback_agree(ctx, orc, options, shape, kshape):
    """The three transform-domain formulations -- direct z pass (default for Kz <= 64), FFT z pass with the expanded
    PSF spectrum (deep PSFs), rocFFT (sizes outside the pass table) -- all meet the 1e-5 contract."""
    rng = np.random.default_rng(44)
    v = rng.random(shape, dtype=np.float32)
    psf = rng.random(kshape, dtype=np.float32) + 0.1
    ref = orc.convolve_fft(v, psf.copy())
    options(fft_zpass="auto", fft_backend="custom")
    direct = ctx.convolve(v, psf.copy(), method=1)
    options(fft_zpass="fft")
    zfft = ctx.convolve(v, psf.copy(), method=1)
    options(fft_zpass="auto", fft_backend="rocfft")
    roc = ctx.convolve(v, psf.copy(), method=1)
    options(fft_backend="rocfft", fft_pad="64,72,80")        # explicit padded sizes on the library path
    roc2 = ctx.convolve(v, psf.copy(), method=1) if max(s + k - 1 for s, k in zip(shape, kshape)) <= 64 else roc
    assert rel_to_max(roc2, ref) <= CONV_TOL
    for got in (direct, zfft, roc):
        assert rel_to_max(got, ref) <= CONV_TOL
    assert rel_to_max(direct, zfft) <= 2e-6 and rel_to_max(direct, roc) <= 2e-6


@pytest.mark.parametrize("shape,kshape", [((17, 20, 24), (2, 3, 4)), ((5, 6, 7), (1, 1, 1)), ((70, 18, 22), (64, 3, 3)),
                                          ((16, 21, 19), (33, 5, 5)), ((3, 9, 40), (7, 4, 6)), ((257, 10, 12), (9, 1, 2))])
def test_direct_z_pass_odd_geometries(ctx, orc, shape, kshape):
    """Direct z pass at its edges: even PSF sizes (centre K/2), single planes, 64 taps, a halo longer than the volume
    (repeated reflections), plane counts that do not fill the last tile."""
    rng = np.random.default_rng(sum(shape) + sum(kshape))
    v = rng.random(shape, dtype=np.float32)
    psf = rng.random(kshape, dtype=np.float32) + 0.05
    got = ctx.convolve(v, psf.copy(), method=1)
    assert rel_to_max(got, orc.convolve_fft(v, psf.copy())) <= CONV_TOL
    if np.prod(shape) * np.prod(kshape) < 4e8:
        assert rel_to_max(got, orc.convolve_direct(v, psf.copy())) <= CONV_TOL


def test_convolve_deep_psf_takes_the_fft_z_pass(ctx, orc, synth):
    """Kz > 64 taps: the direct z pass is not offered, the FFT z pass runs (and agrees with the oracle)."""
    v = synth.sphere_phantom(72)
    psf = synth.gaussian_psf(7, 7, 71, sigma=(1.2, 1.3, 14.0))
    got = ctx.convolve(v, psf.copy(), method=1)
    assert rel_to_max(got, orc.convolve_fft(v, psf.copy())) <= CONV_TOL


def test_view_with_fft_z_pass_is_a_valid_view(ctx, orc, synth, options):
    """The fused view on the FFT z pass: rot/att bit-exact, con within tolerance, same acquisition statistics."""
    gt = synth.sphere_phantom(48)
    psf = synth.gaussian_psf(9, sigma=(1.2, 1.4, 2.5))
    p = ctx.view_params(degrees=33, delta=0.01, inc=2, snr=25.0, seed=SEED, stream=2)
    a = ctx.simulate_view(gt, psf.copy(), p, want=("att", "con", "acq"))
    options(fft_zpass="fft")
    b = ctx.simulate_view(gt, psf.copy(), p, want=("att", "con", "acq"))
    assert np.array_equal(a["att"], b["att"])
    assert rel_to_max(a["con"], b["con"]) <= 2e-6
    assert (a["acq"] != b["acq"]).mean() < 0.02


def test_page_locked_buffers_and_preallocated_outputs(ctx, synth):
    """mvsim_host_alloc blocks as numpy arrays: same results as pageable buffers; `out=` reuses destinations."""
    gt = synth.sphere_phantom(40)
    psf = synth.gaussian_psf(7, sigma=(1.1, 1.2, 1.8))
    p = ctx.view_params(degrees=25, inc=2, snr=25.0, seed=SEED, stream=1)
    ref = ctx.simulate_view(gt, psf.copy(), p, want=("con", "acq"))
    g = ctx.pinned_empty(gt.shape)
    g[...] = gt
    dst = {"acq": ctx.pinned_empty(ref["acq"].shape), "con": ctx.pinned_empty(gt.shape)}
    for _ in range(2):
        got = ctx.simulate_view(g, psf.copy(), p, want=("con", "acq"), out=dst)
        assert got["acq"] is dst["acq"] and got["con"] is dst["con"]
        assert np.array_equal(got["acq"], ref["acq"]) and np.array_equal(got["con"], ref["con"])
    with pytest.raises(ValueError):
        ctx.simulate_view(g, psf.copy(), p, out={"acq": np.empty((3, 3, 3), np.float32)})
    view = dst["acq"][1:3]            # a view keeps the block alive after the owner is dropped
    del dst, got
    import gc
    gc.collect()
    assert np.array_equal(view, ref["acq"][1:3])


@pytest.mark.gpu
def test_c_abi_plain_c_consumer_runs(tmp_path):
    """tests/c_abi/smoke.c: a C99 program drives a whole view through the C ABI, no Python or torch in the process."""
    import subprocess
    from .test_host_logic import _build_c_smoke
    r = subprocess.run([_build_c_smoke(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "c-abi smoke ok" in r.stdout


# ------------------------------------------------------------------------------------------------ z-slab tiling
@pytest.mark.parametrize("n,kz,inc,nslabs", [(64, 9, 1, 2), (72, 15, 3, 3), (48, 31, 2, 4), (40, 5, 4, 5)])
def test_view_slab_tiling_matches_the_whole_view(mvs, synth, n, kz, inc, nslabs):
    """One view split into z slabs, one context per slab as one GPU per rank would have it: rotate and
    attenuate recompute the halo, the mirror boundary acts at the global faces only, the adjustImage sum is the only
    exchange, Poisson counters are global -- the stitched acquisition equals the untiled one."""
    gt = synth.sphere_phantom(n)
    psf = synth.gaussian_psf(7, 9, kz, sigma=(1.3, 1.5, max(1.0, kz / 5)))
    dims = (n, n, n)
    nzo = (n - 1) // inc + 1
    with mvs.Context(0) as whole:
        p = whole.view_params(degrees=50, delta=0.01, inc=inc, snr=25.0, seed=SEED, stream=5, conv_method=1)
        ref = whole.simulate_view(gt, psf.copy(), p, want=("con", "acq"))
        ref_noise_free = whole.simulate_view(gt, psf.copy(), whole.view_params(degrees=50, delta=0.01, inc=inc, snr=-1.0,
                                                                              conv_method=1), want=("acq",))["acq"]
    ctxs = [mvs.Context(0) for _ in range(nslabs)]
    try:
        ranges = [ctxs[0].slab_range(n, nslabs, r) for r in range(nslabs)]
        assert ranges[0][0] == 0 and ranges[-1][1] == n and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
        d_gt = [_dev_volume(c, gt) for c in ctxs]                      # every "rank" holds the broadcast ground truth
        sums = [c.view_slab_convolve_dev(d, dims, psf.copy(), p, z0, z1) for c, d, (z0, z1) in zip(ctxs, d_gt, ranges)]
        total = float(np.sum(np.array(sums, dtype=np.float64)))       # what the all-reduce delivers
        for noise in (False, True):
            pp = p if noise else ctxs[0].view_params(degrees=50, delta=0.01, inc=inc, snr=-1.0, conv_method=1)
            parts = []
            for c, (z0, z1) in zip(ctxs, ranges):
                d_acq = c.dev_alloc(max(1, ((z1 - z0) // inc + 2)) * n * n * 4)
                try:
                    k = c.view_slab_finish_dev(dims, pp, z0, z1, total, d_acq)
                    parts.append(c.download(d_acq, (k, n, n)) if k else np.zeros((0, n, n), np.float32))
                finally:
                    c.dev_free(d_acq)
            got = np.concatenate(parts, axis=0)
            assert got.shape == (nzo, n, n)
            if not noise:
                # same per-plane transforms, same z taps in the same order: only the order of the global sum differs
                assert rel_to_max(got, ref_noise_free) <= 1e-6
            else:
                assert np.all(got == np.round(got))
                assert (got != ref["acq"]).mean() < 0.005
                assert abs(got.mean() / ref["acq"].mean() - 1) < 1e-3
        for c, d in zip(ctxs, d_gt):
            c.dev_free(d)
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("n,kz,inc,nslabs", [(128, 15, 2, 2), (96, 9, 1, 3), (128, 31, 4, 1)])
def test_view_slab_in_one_call_on_the_device(mvs, synth, n, kz, inc, nslabs):
    """Round 6: `mvsim_view_slab_dev` -- convolve, reduce, finish as ONE asynchronous call whose slab sum never
    leaves the device -- and the slab's planes through the fused rotate + attenuate + x-transform kernel (planes z_first .. of the
    rotated volume).  With the slab's own sum as the total (a communicator of one rank adds nothing) the one call must equal the
    three-step form bit for bit, with and without the fused kernel; a single slab that is the whole view must equal the untiled view."""
    gt = synth.sphere_phantom(n)
    psf = synth.gaussian_psf(7, 9, kz, sigma=(1.3, 1.5, max(1.0, kz / 5)))
    dims = (n, n, n)
    with mvs.Context(0) as c:
        d_gt = _dev_volume(c, gt)
        d_a, d_b = c.dev_alloc(n * n * n * 4), c.dev_alloc(n * n * n * 4)
        try:
            for noise in (False, True):
                p = c.view_params(degrees=50, delta=0.01, inc=inc, snr=25.0 if noise else -1.0, seed=SEED, stream=5, conv_method=1)
                for r in range(nslabs):
                    z0, z1 = c.slab_range(n, nslabs, r)
                    got = {}
                    for fused in (0, 1):
                        c.set_option("fused_fftx", fused)
                        own = c.view_slab_convolve_dev(d_gt, dims, psf.copy(), p, z0, z1)
                        k = c.view_slab_finish_dev(dims, p, z0, z1, own, d_a)
                        three = c.download(d_a, (k, n, n))
                        k1 = c.view_slab_dev(d_gt, dims, psf.copy(), p, z0, z1, d_b)
                        assert k1 == k and k > 0
                        one = c.download(d_b, (k, n, n))
                        assert np.array_equal(one, three), (noise, r, fused)
                        got[fused] = one
                    assert np.array_equal(got[0], got[1]), (noise, r)       # the fused kernel leaves pass A's spectrum, bit for bit
                    c.set_option("fused_fftx", "auto")
                if nslabs == 1:
                    ref = c.simulate_view(gt, psf.copy(), p, want=("acq",))["acq"]
                    if noise:
                        assert (got[1] != ref).mean() < 0.005
                    else:
                        assert rel_to_max(got[1], ref) <= 1e-6
        finally:
            c.set_option("fused_fftx", "auto")
            for d in (d_gt, d_a, d_b):
                c.dev_free(d)


def test_view_slab_rejects_what_it_cannot_tile(ctx, synth):
    gt = synth.sphere_phantom(32)
    d = _dev_volume(ctx, gt)
    try:
        p = ctx.view_params(degrees=10, inc=1, snr=25.0)
        with pytest.raises(ValueError):
            ctx.view_slab_convolve_dev(d, (32, 32, 32), synth.gaussian_psf(5), p, 8, 8)                 # empty slab
        with pytest.raises(ValueError):
            ctx.view_slab_convolve_dev(d, (32, 32, 32), synth.gaussian_psf(5, 5, 71), p, 0, 16)         # PSF too deep
        with pytest.raises(ValueError):
            ctx.view_slab_convolve_dev(d, (32, 32, 32), synth.gaussian_psf(5), ctx.view_params(axis=1), 0, 16)
    finally:
        ctx.dev_free(d)


# ------------------------------------------------------------------------------------------------ BASELINE configs[3], [4]
def _window_volume(nz, ny, nx):
    """Compactly supported, non-separable enough: product of (1 - t^2)^2 windows plus a few isolated bright voxels."""
    def w(n, frac):
        t = (np.arange(n, dtype=np.float32) - (n - 1) / 2) / (frac * n / 2)
        return np.clip(1 - t * t, 0, None) ** 2
    vol = (w(nz, 0.55)[:, None, None] * w(ny, 0.6)[None, :, None]).astype(np.float32) * w(nx, 0.5)[None, None, :]
    rng = np.random.default_rng(77)
    for _ in range(64):
        z, y, x = (int(rng.integers(n // 3, 2 * n // 3)) for n in (nz, ny, nx))
        vol[z, y, x] += np.float32(5 * rng.random())
    return vol


def _large_view_properties(mvs, dims_xyz, kdims_zyx, inc, sigma, psf_raw=None, oracle_samples=False):
    nx, ny, nz = dims_xyz
    synth = importlib.import_module("multiview-simulation_amd.synthetic")
    gt = _window_volume(nz, ny, nx)
    nzo = (nz - 1) // inc + 1
    with mvs.Context(0) as c:
        d_gt = _dev_volume(c, gt)
        d_acq = c.dev_alloc(nzo * ny * nx * 4)
        d_acq2 = c.dev_alloc(nzo * ny * nx * 4)
        try:
            # 0 degrees, no attenuation, delta PSF, no noise: the view is the adjusted ground truth, strided in z
            delta = np.zeros(kdims_zyx, np.float32)
            delta[tuple(k // 2 for k in kdims_zyx)] = 3.0
            p0 = c.view_params(degrees=0, delta=0.0, inc=inc, snr=-1.0, seed=SEED, stream=0, conv_method=1)
            corr = c.simulate_view_dev(d_gt, dims_xyz, delta, p0, d_acq, want_corr=True)
            got = c.download(d_acq, (nzo, ny, nx))
            mean = gt.sum(dtype=np.float64) / gt.size
            assert abs(corr * mean - (1.0 - 1e-4)) < 1e-5          # Tools.adjustImage: (target - minValue) / mean
            want = (gt[::inc] * np.float32(corr)).astype(np.float32) + np.float32(1e-4)
            assert rel_to_max(got, want) <= CONV_TOL
            del want, got
            # a real view: integer counts, mean count ~ avgIntensity * mul, deterministic, stream-separated
            psf = psf_raw if psf_raw is not None else synth.gaussian_psf(kdims_zyx[2], kdims_zyx[1], kdims_zyx[0], sigma=sigma)
            assert psf.shape == tuple(kdims_zyx)
            p1 = c.view_params(degrees=60, delta=REF_DELTA, inc=inc, snr=25.0, seed=SEED, stream=3, conv_method=1)
            c.simulate_view_dev(d_gt, dims_xyz, psf.copy(), p1, d_acq)
            a = c.download(d_acq, (nzo, ny, nx))
            assert a.min() >= 0 and np.array_equal(a, np.round(a))
            # adjustImage sets the mean of the full convolved volume to 1; the strided planes sample it
            assert abs(a.sum(dtype=np.float64) / a.size / 124.99999999999997 - 1) < 0.05
            c.simulate_view_dev(d_gt, dims_xyz, psf.copy(), p1, d_acq2)
            assert np.array_equal(c.download(d_acq2, (nzo, ny, nx)), a)
            p2 = c.view_params(degrees=60, delta=REF_DELTA, inc=inc, snr=25.0, seed=SEED, stream=4, conv_method=1)
            c.simulate_view_dev(d_gt, dims_xyz, psf.copy(), p2, d_acq2)
            b = c.download(d_acq2, (nzo, ny, nx))
            assert not np.array_equal(a, b) and abs(a.sum(dtype=np.float64) / b.sum(dtype=np.float64) - 1) < 1e-3
            del b
            if oracle_samples:
                _large_view_oracle_samples(c, gt, d_gt, dims_xyz, psf, inc, 60, a, 3, d_acq2)
                # the same volume on a low background with bright voxels next to the faces: no empty plane (the unflagged passes), and the
                # mirror boundaries of the convolution act on content -- x and z at the z faces, x and y in the middle planes
                gt += np.float32(0.03)
                for zz, yy, xx in ((0, ny // 2, 1), (1, ny // 2 - 3, nx - 2), (nz - 1, ny // 2 + 2, 0), (nz // 2, 0, 2), (nz // 2 + 1, ny - 1, nx - 1)):
                    gt[zz, yy, xx] += np.float32(4.0)
                c.upload(d_gt, gt)
                c.simulate_view_dev(d_gt, dims_xyz, psf.copy(), p1, d_acq)
                _large_view_oracle_samples(c, gt, d_gt, dims_xyz, psf, inc, 60, c.download(d_acq, (nzo, ny, nx)), 3, d_acq2)
        finally:
            for d in (d_gt, d_acq, d_acq2):
                c.dev_free(d)


def _large_view_oracle_samples(c, gt, d_gt, dims_xyz, psf, inc, degrees, counts, counts_stream, d_acq):
    """Oracle-checked voxels of a FULL-SIZE view (the way test_config4_as_stated... does it for configs[4]).
    The same view without noise, `rot` and `att` kept on the device (the fused kernel writes them beside its spectrum rows):
      rot, att   WHOLE planes at both faces and in the middle, bit for bit against the reference's loops restated over those planes
                 (orc_rotate_around_axis_planes = SimulateMultiViewDataset.java:119-132 over the planes' voxels; attenuate3d :335-359 walks y
                 inside a plane of constant z, so the planes' columns are complete);
      con        the noise-free acquisition = Tools.adjustImage of the convolved planes k * inc (Tools.java:143-159, two roundings) at ~450
                 voxels -- blocks at both x faces x both y faces and the middle rows, random and the brightest voxels of planes at the z = 0
                 face, in the middle and at the last acquired plane -- against the exact fp64 direct sum over the downloaded `att` window
                 (orc_convolve_direct_at: SimulateMultiViewDataset.java:253-264 as FFTConvolution defines it), <= 1e-5 of the range: a wrong tap
                 weight or a wrong mirror at 1024-long lines fails here;
      counts     two acquired planes in the bright middle of the volume, bit for bit on identical lambda: the oracle's counter sampler
                 (second implementation) on the downloaded noise-free planes with the FULL volume's source indices."""
    import oracle as orc
    nx, ny, nz = dims_xyz
    kz = psf.shape[0]
    assert kz % 2 == 1
    r = kz // 2
    nzo = (nz - 1) // inc + 1
    plane = nx * ny
    d_rot, d_att = c.dev_alloc(plane * nz * 4), c.dev_alloc(plane * nz * 4)
    try:
        pn = c.view_params(degrees=degrees, delta=REF_DELTA, inc=inc, snr=-1.0, seed=SEED, stream=0, conv_method=1)
        corr = c.simulate_view_dev(d_gt, dims_xyz, psf.copy(), pn, d_acq, rot_dptr=d_rot, att_dptr=d_att, want_corr=True)
        nf = c.download(d_acq, (nzo, ny, nx))
        scale = float(nf.max())
        assert scale > 0 and corr > 0
        rng = np.random.default_rng(11)
        for z in sorted({0, 1, nz // 2, nz - 1, int(rng.integers(2, nz - 2))}):
            want_rot = orc.rotate_around_axis_planes(gt, 0, degrees, z, 1)
            assert np.array_equal(c.download(d_rot + z * plane * 4, (1, ny, nx)), want_rot), f"rot plane {z}"
            assert np.array_equal(c.download(d_att + z * plane * 4, (1, ny, nx)), orc.attenuate3d(want_rot, REF_DELTA)), f"att plane {z}"
        psf_n = psf.copy()
        orc.norm_image(psf_n)
        zm = (nz // 2) // inc * inc
        zt = (nzo - 1) * inc
        checked = 0
        for zlo, zhi, zs in ((0, inc + r + 1, (0, inc)), (zm - r, zm + inc + r + 1, (zm, zm + inc)), (zt - r, nz, (zt,))):
            win = c.download(d_att + zlo * plane * 4, (zhi - zlo, ny, nx))
            for z in zs:
                got_plane = nf[z // inc]
                bright = np.argsort(got_plane.ravel())[-16:]
                edge_y = np.concatenate([np.arange(3), np.arange(ny // 2 - 1, ny // 2 + 2), np.arange(ny - 3, ny)])       # 9 rows: both y faces, the middle
                edge_x = np.concatenate([np.arange(3), np.arange(nx - 3, nx)])                                          # 6 columns: both x faces
                ys = np.concatenate([np.repeat(edge_y, edge_x.size), rng.integers(0, ny, 24), bright // nx])
                xs = np.concatenate([np.tile(edge_x, edge_y.size), rng.integers(0, nx, 24), bright % nx])
                pos = np.unique(xs + nx * ys)
                want = orc.convolve_direct_at(win, psf_n, pos + plane * (z - zlo))
                want = (want.astype(np.float64) * corr).astype(np.float32) + np.float32(1e-4)       # Tools.adjustImage, two roundings
                err = float(np.abs(got_plane.ravel()[pos] - want).max())
                assert err <= CONV_TOL * scale, (z, err, scale)
                checked += pos.size
        assert checked >= 300
        # counts on identical lambda: the two acquired planes zm, zm + inc
        k0 = zm // inc
        lam_win = np.zeros((inc + 1, ny, nx), np.float32)
        lam_win[0], lam_win[inc] = nf[k0], nf[k0 + 1]
        assert float(lam_win.max()) * 124.99999999999997 > 50.0                                      # the PTRS regime is populated
        want_counts = orc.extract_slices_counter_window(lam_win, inc, 25.0, SEED, counts_stream, zm)
        assert np.array_equal(counts[k0:k0 + 2], want_counts)
        # ... and at the LAST acquired planes, whose counters are the view's largest (configs[4] at inc 1: 511 * 2^22 .. 2^31 - 1)
        kl = max(nzo - 2, 0)
        want_last = np.stack([orc.poisson_counter_array(nf[k], orc.poisson_mul(25.0), SEED, counts_stream, k * inc * plane)
                              for k in range(kl, nzo)])
        assert np.array_equal(counts[kl:nzo], want_last)
    finally:
        c.dev_free(d_rot)
        c.dev_free(d_att)


def test_config1_512_cubed_fused_view_with_rotation(mvs):
    """BASELINE configs[1]/[2] per view at full size: 512^3, 31^3 PSF, the FUSED view with a real rotation (60 degrees)."""
    _large_view_properties(mvs, (512, 512, 512), (31, 31, 31), 1, (2.0, 2.2, 6.0), oracle_samples=True)


def test_config3_1024_cubed_anisotropic_psf_inc4(mvs):
    """BASELINE configs[3] as SURVEY 8(d) states it: 1024^3 volume, 31 x 31 x 63 Gaussian PSF with sigma = (2, 2.2, 12), 4x
    axial down-sampling -- one view fits one GPU, so the view runs untiled here (the slab-tiled form of the same PSF depth:
    test_view_slab_tiling_at_size_with_the_config3_psf)."""
    _large_view_properties(mvs, (1024, 1024, 1024), (63, 31, 31), 4, (2.0, 2.2, 12.0), oracle_samples=True)


def test_view_slab_tiling_at_size_with_the_config3_psf(mvs, synth):
    """configs[3]'s z-slab tiling at size: a 512 x 512 x 256 view with the 63-deep anisotropic PSF (31 x 31 x 63, sigma
    2 / 2.2 / 12), inc 4, cut into 4 slabs of 64 planes (one context per slab, as one GPU per rank would have it).  Every slab
    recomputes a 31-plane halo of rotation and attenuation, the mirror boundary acts at the global faces only, the one
    exchanged double is the adjustImage sum: the stitched noise-free acquisition equals the untiled view's to 1e-6, the
    Poisson counts (global counters) differ only where that 1e-6 moves a voxel across an integer step."""
    nx, ny, nz, inc, nslabs = 512, 512, 256, 4, 4
    gt = np.ascontiguousarray(synth.sphere_phantom(512)[128:384])
    psf = synth.gaussian_psf(31, 31, 63, sigma=(2.0, 2.2, 12.0))
    dims = (nx, ny, nz)
    nzo = (nz - 1) // inc + 1
    with mvs.Context(0) as whole:
        p = whole.view_params(degrees=50, delta=0.01, inc=inc, snr=25.0, seed=SEED, stream=5, conv_method=1)
        pn = whole.view_params(degrees=50, delta=0.01, inc=inc, snr=-1.0, conv_method=1)
        ref = whole.simulate_view(gt, psf.copy(), p, want=("acq",))["acq"]
        ref_noise_free = whole.simulate_view(gt, psf.copy(), pn, want=("acq",))["acq"]
    ctxs = [mvs.Context(0) for _ in range(nslabs)]
    try:
        ranges = [ctxs[0].slab_range(nz, nslabs, r) for r in range(nslabs)]
        assert [b - a for a, b in ranges] == [64] * 4
        d_gt = [_dev_volume(c, gt) for c in ctxs]
        sums = [c.view_slab_convolve_dev(d, dims, psf.copy(), p, z0, z1) for c, d, (z0, z1) in zip(ctxs, d_gt, ranges)]
        total = float(np.sum(np.array(sums, dtype=np.float64)))
        for pp, want in ((pn, ref_noise_free), (p, ref)):
            parts = []
            for c, (z0, z1) in zip(ctxs, ranges):
                d_acq = c.dev_alloc(((z1 - z0) // inc + 2) * ny * nx * 4)
                try:
                    k = c.view_slab_finish_dev(dims, pp, z0, z1, total, d_acq)
                    parts.append(c.download(d_acq, (k, ny, nx)))
                finally:
                    c.dev_free(d_acq)
            got = np.concatenate(parts, axis=0)
            assert got.shape == (nzo, ny, nx)
            if pp is pn:
                assert rel_to_max(got, want) <= 1e-6
            else:
                assert np.array_equal(got, np.round(got)) and (got != want).mean() < 0.005
                assert abs(got.mean() / want.mean() - 1) < 1e-3
        for c, d in zip(ctxs, d_gt):
            c.dev_free(d)
    finally:
        for c in ctxs:
            c.close()


def test_host_streaming_entry_points_at_512_cubed(ctx, synth):
    """configs[4] names host-pinned streaming: the z-slab host-buffer entry point (mvsim_simulate_view_zslabs: ground truth
    in, acquisition out as lists of page-locked z slabs -- the convention for volumes beyond one Java array) and the
    pipelined entry point (mvsim_simulate_view_async / mvsim_wait) at 512^3, against the synchronous single-buffer call."""
    n = 512
    gt = synth.sphere_phantom(n)
    psf = synth.gaussian_psf(31, sigma=(2.0, 2.2, 6.0))
    p = ctx.view_params(degrees=60, inc=3, snr=25.0, seed=SEED, stream=2, conv_method=1)
    ref = ctx.simulate_view(gt, psf.copy(), p)
    cuts = [0, 100, 101, 300, 512]
    slabs = []
    for a, b in zip(cuts, cuts[1:]):
        h = ctx.pinned_empty((b - a, n, n))
        h[...] = gt[a:b]
        slabs.append(h)
    acq, corr = ctx.simulate_view_zslabs(slabs, psf.copy(), p, [60, 1, 110])
    assert abs(corr - ref["corr"]) <= 1e-12 * corr
    assert np.array_equal(np.concatenate(acq, axis=0), ref["acq"])
    del acq, slabs
    g = ctx.pinned_empty(gt.shape)
    g[...] = gt
    params = [ctx.view_params(degrees=15 + 45 * v, inc=3, snr=25.0, seed=SEED, stream=v, conv_method=1) for v in range(3)]
    outs = [{"acq": ctx.pinned_empty(ref["acq"].shape)} for _ in range(3)]
    tickets = [ctx.simulate_view_async(g, psf.copy(), params[v], outs[v]) for v in range(2)]
    ctx.wait(tickets[0])
    tickets.append(ctx.simulate_view_async(g, psf.copy(), params[2], outs[2]))
    for t in tickets[1:]:
        ctx.wait(t)
    for v in range(3):
        assert np.array_equal(outs[v]["acq"], ctx.simulate_view(gt, psf.copy(), params[v])["acq"]), v


def test_config4_as_stated_stencil_through_pinned_zslabs(mvs, orc):
    """BASELINE configs[4] as it is worded: a 2048 x 2048 x 512 volume -- 2^31 voxels, one more than a Java array (and the reference's
    ArrayImgFactory, SimulateMultiViewDataset.java:109) can hold --, the measured-like non-separable 63^3 PSF, the LDS-tiled DIRECT
    STENCIL (conv_method 2: 1.07 Pflop, ~14 s), ground truth in and acquisition out as lists of PAGE-LOCKED z slabs through
    mvsim_simulate_view_zslabs.  Checked against the FFT passes through the same entry point on every acquired voxel, and against the
    oracle's exact fp64 direct sum (orc_convolve_direct_at) at sampled voxels in two z windows: the z = 0 face, where the mirror
    boundary acts in all three axes, and the middle of the volume."""
    synth = importlib.import_module("multiview-simulation_amd.synthetic")
    nx, ny, nz, inc, slab = 2048, 2048, 512, 3, 64
    nzo = (nz - 1) // inc + 1
    psf = synth.hourglass_psf(63)
    # the window volume of _window_volume, built slab by slab straight into page-locked memory
    def w(n, frac):
        t = (np.arange(n, dtype=np.float32) - (n - 1) / 2) / (frac * n / 2)
        return np.clip(1 - t * t, 0, None) ** 2
    wz, plane = w(nz, 0.55), (w(ny, 0.6)[:, None] * w(nx, 0.5)[None, :]).astype(np.float32)
    with mvs.Context(0) as c:
        slabs = []
        for z0 in range(0, nz, slab):
            h = c.pinned_empty((slab, ny, nx))
            np.multiply(wz[z0:z0 + slab, None, None], plane[None], out=h)
            slabs.append(h)
        slabs[4][10, 1000, 1100] += np.float32(3.0)                      # an isolated bright voxel in the middle window
        out_nz = [64, 64, nzo - 128]
        ps = c.view_params(degrees=60, delta=REF_DELTA, inc=inc, snr=-1.0, seed=SEED, stream=0, conv_method=2)
        pf = c.view_params(degrees=60, delta=REF_DELTA, inc=inc, snr=-1.0, seed=SEED, stream=0, conv_method=1)
        import time
        t0 = time.perf_counter()
        acq_s, corr_s = c.simulate_view_zslabs(slabs, psf.copy(), ps, out_nz, pinned=True)
        t_stencil = time.perf_counter() - t0
        t0 = time.perf_counter()
        acq_f, corr_f = c.simulate_view_zslabs(slabs, psf.copy(), pf, out_nz, pinned=True)
        t_fft = time.perf_counter() - t0
        print(f"configs[4] through page-locked z slabs: direct stencil {t_stencil:.2f} s, FFT passes {t_fft:.3f} s (host to host)")
        assert abs(corr_s / corr_f - 1) <= 1e-6
        scale = max(float(a.max()) for a in acq_f)
        assert scale > 0
        for a, b in zip(acq_s, acq_f):                                    # every acquired voxel
            for k0 in range(0, a.shape[0], 16):
                assert float(np.abs(a[k0:k0 + 16] - b[k0:k0 + 16]).max()) <= CONV_TOL * scale
        # the attenuated volume of the same view, device-resident, for the oracle: only the planes the sampled voxels' taps reach
        d_gt, d_att, d_acq = c.dev_alloc(nx * ny * nz * 4), c.dev_alloc(nx * ny * nz * 4), c.dev_alloc(nx * ny * nzo * 4)
        try:
            for i, h in enumerate(slabs):
                c.upload(d_gt + i * slab * ny * nx * 4, h)
            corr = c.simulate_view_dev(d_gt, (nx, ny, nz), psf.copy(), pf, d_acq, att_dptr=d_att, want_corr=True)
            assert abs(corr / corr_f - 1) <= 1e-6
            pn = psf.copy()
            orc.norm_image(pn)
            acq_all = np.concatenate([a.reshape(-1, ny, nx) for a in acq_s], axis=0)
            rng = np.random.default_rng(4)
            for zlo, zhi, zs in ((0, 35, (0, 3)), (218, 285, (249, 252))):     # 63 taps, centre 31: plane z reads z - 31 .. z + 31
                win = c.download(d_att + zlo * ny * nx * 4, (zhi - zlo, ny, nx))
                ys = np.concatenate([np.arange(3), rng.integers(0, ny, 60), [1000]])
                xs = np.concatenate([np.arange(3), rng.integers(0, nx, 60), [1100]])
                for z in zs:
                    idx = np.unique(xs + nx * (ys + ny * (z - zlo)))
                    want = orc.convolve_direct_at(win, pn, idx)
                    want = (want.astype(np.float64) * corr).astype(np.float32) + np.float32(1e-4)      # Tools.adjustImage, two roundings
                    got = acq_all[z // inc].ravel()[idx - nx * ny * (z - zlo)]
                    assert float(np.abs(got - want).max()) <= CONV_TOL * scale, (z, float(np.abs(got - want).max()), scale)
        finally:
            for d in (d_gt, d_att, d_acq):
                c.dev_free(d)


def test_config4_2048x2048x512_psf63(mvs):
    """BASELINE configs[4]: 2048 x 2048 x 512 volume, non-separable 63^3 PSF (the tilted hour-glass of SURVEY 8d; padded
    2240 x 2160 on the hand-written FFT path), resident in HBM."""
    synth = importlib.import_module("multiview-simulation_amd.synthetic")
    _large_view_properties(mvs, (2048, 2048, 512), (63, 63, 63), 1, None, psf_raw=synth.hourglass_psf(63), oracle_samples=True)


# ------------------------------------------------------------------------------------------------ RCCL entry points
def test_rccl_entry_points_single_rank(mvs, synth):
    """Every mvsim_comm_* entry point executes on the one GPU (RCCL supports nranks = 1): the scatter + all-gather
    form of the ground-truth broadcast (a count that does not divide into aligned chunks, so the tail broadcast runs
    too), the ring form, the float all-reduce and the one-double all-reduce."""
    with mvs.Context(0) as c:
        assert c.comm_size is None
        with pytest.raises(ValueError):
            c.comm_init(1, 0, b"short")                                   # no communicator, no size
        assert c.comm_size is None
        c.comm_init(1, 0, mvs.Context.comm_unique_id())
        assert c.comm_size == 1                                           # what TiledView.run_on_device asks before it launches
        vol = np.random.default_rng(8).random(100003, dtype=np.float32)
        d = _dev_volume(c, vol)
        try:
            c.comm_broadcast_volume(d, vol.size, 0)
            c.synchronize()
            assert np.array_equal(c.download(d, vol.shape), vol)
            c.set_option("broadcast", "ring")
            c.comm_broadcast_volume(d, vol.size, 0)
            c.set_option("broadcast", "peer_copy")                        # copy-engine form: with one rank its barriers and the map
            with pytest.raises(ValueError, match="not registered"):
                c.comm_broadcast_volume(d, vol.size, 0)                   # never an implicit registration keyed by address
            c.comm_register_volume(d, vol.size)                           # the explicit collective
            c.comm_broadcast_volume(d, vol.size, 0)
            c.comm_register_volume(d, vol.size)                           # registering again replaces the mapping
            c.comm_broadcast_volume(d, vol.size, 0)
            c.synchronize()
            assert np.array_equal(c.download(d, vol.shape), vol)
            c.comm_unregister_volume(d)
            with pytest.raises(ValueError, match="not registered"):
                c.comm_broadcast_volume(d, vol.size, 0)
            d2 = c.dev_alloc(vol.nbytes)
            c.comm_register_volume(d2, vol.size)
            c.dev_free(d2)                                                # freeing the buffer drops its registration
            d3 = c.dev_alloc(vol.nbytes)                                  # (the allocator may hand the same address back)
            with pytest.raises(ValueError, match="not registered"):
                c.comm_broadcast_volume(d3, vol.size, 0)
            c.dev_free(d3)
            c.set_option("broadcast", "pipelined")                        # one rank: an empty schedule (tests/test_host_logic.py walks the real ones)
            c.comm_broadcast_volume(d, vol.size, 0)
            c.synchronize()
            assert np.array_equal(c.download(d, vol.shape), vol)
            c.set_option("broadcast", "scatter_allgather")
            c.comm_allreduce_sum(d, vol.size)
            c.synchronize()
            assert np.array_equal(c.download(d, vol.shape), vol)          # sum over one rank
            assert c.comm_allreduce_sum_f64(1.25) == 1.25
            with pytest.raises(ValueError):
                c.comm_broadcast_volume(d, vol.size, 3)                   # root out of range
        finally:
            c.dev_free(d)
        c.comm_destroy()
        assert c.comm_size is None
        with pytest.raises(ValueError):
            c.comm_broadcast_volume(1, 1, 0)                              # communicator gone


def test_group_single_process_views(mvs, synth):
    """mvsim_group_*: one process, one context per device, ncclCommInitAll, ground truth broadcast, view v on device
    v % ndev -- the acquisitions equal those of the per-context entry point (same kernels, same counters)."""
    gt = synth.sphere_phantom(40)
    psfs = [synth.gaussian_psf(7, sigma=(1.1, 1.2, 1.8 + 0.1 * v)) for v in range(3)]
    with mvs.Context(0) as c:
        params = [c.view_params(degrees=15 + 120 * v, inc=2, snr=25.0, seed=SEED, stream=v) for v in range(3)]
        want = [c.simulate_view(gt, psfs[v].copy(), params[v])["acq"] for v in range(3)]
    with mvs.Group(1) as g:
        assert len(g) == 1
        g.broadcast_volume(gt)
        raw = [q.copy() for q in psfs]
        got = g.simulate_views(raw, params)
        assert abs(float(raw[0].astype(np.float64).sum()) - 1.0) < 1e-6    # PSFs normalised in place (Q5)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        mvs.Group(2, devices=[0, 0])


def test_rccl_two_processes_two_gpus(mvs, tmp_path):
    """Two ranks, one process per GPU, through the C ABI only (no torch): broadcast (RCCL scatter + all-gather, RCCL ring, and the
    copy-engine form over IPC-mapped buffers), all-reduce, f64 all-reduce.  Needs two GPUs: skipped on the one-GPU box, runs on the driver's multi-GPU node."""
    import ctypes
    import subprocess
    import sys
    n = ctypes.c_int(0)
    mvs._lib.load().mvsim_device_count(ctypes.byref(n))
    if n.value < 2:
        pytest.skip(f"{n.value} GPU visible: the two-rank RCCL run needs two")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_rccl_worker.py")
    uid = str(tmp_path / "uid.bin")
    procs = [subprocess.Popen([sys.executable, worker, str(r), "2", uid], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"rank {r} ok" in o, o


# ------------------------------------------------------------------------------------------------ boundary: round 2 additions
class _PlainRandom:
    """A java.util.Random look-alike that is NOT this package's JavaRandom (what SimulateTileStitching.java:93,108 hands
    to `simulate`): only nextInt(bound) / nextDouble() are offered."""

    def __init__(self, mvs, seed):
        self._j = mvs.JavaRandom(seed)

    def nextInt(self, bound):
        return self._j.nextInt(bound)

    def nextDouble(self):
        return self._j.nextDouble()


def test_draw_spheres_accepts_any_random(mvs, orc):
    """drawSpheres with a caller-supplied generator that is not the package's own: the walk over the large sphere runs
    on the host with THAT generator, the compositing on the GPU (mvsim_splat_spheres) -- same image and same generator
    state as the oracle's drawSpheres."""
    S = mvs.SimulateMultiViewDataset
    img = np.zeros((140, 132, 150), np.float32)
    r = _PlainRandom(mvs, 77)
    S.drawSpheres(img, 0.0, 1.0, 1, True, r)
    ref = np.zeros_like(img)
    ro = orc.JRandom(77)
    n = orc.draw_spheres(ref, 0.0, 1.0, 1, True, ro)
    assert n > 0 and np.array_equal(img, ref)
    assert r._j._s == int(ro.st.s)
    with pytest.raises(ValueError):                                     # a sphere that leaves the image: the reference throws
        mvs.default_context().splat_spheres(img, [(2, 50, 50, 5, 1.0)])


def test_async_pipelined_views_equal_synchronous_views(ctx, synth):
    """mvsim_simulate_view_async / mvsim_wait: six views of one ground truth through the two staging sets (page-locked
    buffers, uploads skipped while the ground truth is unchanged, re-upload on a new generation, intermediates on
    request) give exactly the voxels of the synchronous entry point."""
    gt = synth.sphere_phantom(48)
    g = ctx.pinned_empty(gt.shape)
    g[...] = gt
    psfs = [synth.gaussian_psf(7, sigma=(1.1, 1.2, 1.6 + 0.1 * v)) for v in range(6)]
    params = [ctx.view_params(degrees=15 + 60 * v, inc=2, snr=25.0, seed=SEED, stream=v) for v in range(6)]
    want = [ctx.simulate_view(gt, psfs[v].copy(), params[v], want=("con", "acq")) for v in range(6)]
    outs = [{"acq": ctx.pinned_empty(want[0]["acq"].shape)} for _ in range(6)]
    outs[3]["con"] = ctx.pinned_empty(gt.shape)
    raws = [q.copy() for q in psfs]
    tickets = []
    for v in range(6):
        tickets.append(ctx.simulate_view_async(g, raws[v], params[v], outs[v]))
        if v >= 1:
            corr = ctx.wait(tickets[v - 1])                             # the caller's loop: submit v, collect v - 1
            assert abs(corr - want[v - 1]["corr"]) <= 1e-12 * corr
            assert np.array_equal(outs[v - 1]["acq"], want[v - 1]["acq"])
    ctx.wait(tickets[5])
    assert np.array_equal(outs[5]["acq"], want[5]["acq"]) and np.array_equal(outs[3]["con"], want[3]["con"])
    assert ctx.wait(tickets[4]) == pytest.approx(want[4]["corr"], rel=1e-12)     # waiting again is harmless
    # new contents behind the same pointer: a new generation forces the upload
    g[...] = gt[::-1]
    o2 = {"acq": ctx.pinned_empty(want[0]["acq"].shape)}
    ctx.wait(ctx.simulate_view_async(g, psfs[0].copy(), params[0], o2, gt_generation=1))
    assert np.array_equal(o2["acq"], ctx.simulate_view(gt[::-1], psfs[0].copy(), params[0])["acq"])
    with pytest.raises(ValueError):
        ctx.wait(10_000)


def test_async_acquisitions_cross_pcie_as_uint16_counts(mvs, synth):
    """Tools.poissonProcess stores Poisson COUNTS as floats (Tools.java:84): mvsim_simulate_view_async packs a sampled view's
    acquisition to uint16 on the device, downloads half the bytes and widens them on the host (mvsim_wait).  Identical arrays to the
    float32 transfer -- for unaligned output buffers and odd sizes too; a view whose counts exceed 65 535 (SNR 700: lambda ~ 10^5) is
    fetched as float32 after all, automatically; a view without noise (snr < 0) never takes the 16-bit path.  (The volume is the
    phantom on a pedestal: adjustImage sets the MEAN to 1, so the bright voxels of a small, mostly empty phantom alone would reach
    counts beyond 65 535 at SNR 25 already -- the automatic fallback, which the SNR 700 case exercises.)"""
    gt = (synth.sphere_phantom(61) + np.float32(0.5)).astype(np.float32)
    psf = synth.gaussian_psf(7, sigma=(1.1, 1.2, 1.6))
    with mvs.Context(0) as c:
        g = c.pinned_empty(gt.shape)
        g[...] = gt
        for snr, u16_expected, fallback_expected in ((25.0, True, False), (700.0, True, True), (-1.0, False, False)):
            p = c.view_params(degrees=40, inc=2, snr=snr, seed=SEED, stream=2)
            nzo = (61 - 1) // 2 + 1
            c.set_option("acq_transfer", "f32")
            want = c.pinned_empty((nzo, 61, 61))
            c.wait(c.simulate_view_async(g, psf.copy(), p, {"acq": want}))
            before = c.transfer_stats()
            assert before == c.transfer_stats()                       # float32 transfers are not counted
            c.set_option("acq_transfer", "auto")
            c.set_option("host_threads", 3)
            backing = np.zeros(nzo * 61 * 61 + 3, np.float32)
            got = backing[1:-2].reshape(nzo, 61, 61)                  # 4-byte aligned only: the widening's scalar head and tail
            tickets = [c.simulate_view_async(g, psf.copy(), p, {"acq": got})]
            got2 = c.pinned_empty((nzo, 61, 61))
            tickets.append(c.simulate_view_async(g, psf.copy(), p, {"acq": got2}))     # two outstanding views: both staging sets
            for t in tickets:
                c.wait(t)
            after = c.transfer_stats()
            assert np.array_equal(got, want) and np.array_equal(got2, want), snr
            assert (after[0] - before[0] == 2) == u16_expected and (after[1] - before[1] == 2) == fallback_expected, (snr, before, after)
            if snr == 700.0:
                assert want.max() > 65535
            if snr == 25.0:
                assert 0 < want.max() < 65535 and np.all(want == np.round(want))


def test_synchronous_counts_cross_pcie_as_uint16(mvs):
    """The synchronous host-buffer entry points (down_counts) send sampled outputs of 2^20 values and more over PCIe as uint16 counts
    too: the result equals the float32 transfer (acq_transfer=f32) bit for bit -- at the threshold, five values past it (the widening's
    tail), and with one lambda of 10^5 among them (a count beyond 65 535: the automatic float32 fallback) --, mvsim_get_transfer_stats
    moves by (1, 0) or (1, 1), and 2^20 - 1 values never take the path.  mvsim_release_caches frees the staging pair; the next call
    builds it again, with the same result, and the statistics go on from where they were."""
    snr = float(np.sqrt(5.0))                                     # poissonMul = (snr / sqrt 5)^2 = 1: the values ARE the lambdas
    n = 1 << 20
    lam = (4.0 + 2.0 * np.random.default_rng(20).random(n + 5)).astype(np.float32)
    bright = lam[:n].copy()
    bright[n // 2] = 1.0e5
    vol = lam[:n].reshape(64, 128, 128)                           # extract_slices at inc 1: exactly 2^20 outputs
    with mvs.Context(0) as c:
        def sample(x, transfer):
            c.set_option("acq_transfer", transfer)
            if x.ndim == 3:
                return c.extract_slices(x, 1, snr, SEED, stream=3)
            y = x.copy()
            c.poisson_process(y, snr, SEED, stream=3)
            return y

        def check(name, x, moved):
            start = c.transfer_stats()
            want = sample(x, "f32")
            before = c.transfer_stats()
            got = sample(x, "auto")
            after = c.transfer_stats()
            print(name, "stats", start, before, after, "max count", float(want.max()))
            assert start == before, name                          # float32 transfers are not counted
            assert got.shape == want.shape and np.array_equal(got, want), name
            assert (after[0] - before[0], after[1] - before[1]) == moved, (name, before, after)
            return got

        first = check("2^20", lam[:n], (1, 0))
        assert 0 < first.max() < 65535 and np.all(first == np.round(first))
        check("2^20 + 5", lam, (1, 0))
        assert check("one lambda of 1e5", bright, (1, 1)).max() > 65535
        check("extract_slices 128 x 128 x 64", vol, (1, 0))
        check("2^20 - 1", lam[:n - 1], (0, 0))
        c.release_caches()
        again = check("2^20 after release_caches", lam[:n], (1, 0))
        assert np.array_equal(again, first)


def test_simulate_views_with_host_buffers(mvs, synth):
    """mvsim_simulate_views: the view loop of `main` (SimulateMultiViewDataset.java:567-585) in ONE call with host buffers -- ground
    truth up once, the views stacked, the acquisitions back together as 16-bit counts -- equals one mvsim_simulate_view call per view,
    also with a different spacing per view (then the views run side by side instead of stacked) and for a view without noise."""
    gt = (synth.sphere_phantom(57) + np.float32(0.4)).astype(np.float32)
    psfs = [synth.gaussian_psf(9, sigma=(1.2, 1.4, 2.0 + 0.1 * v)) for v in range(5)]
    with mvs.Context(0) as c:
        for incs, snrs in (([3] * 5, [25.0] * 5), ([1, 2, 3, 1, 2], [25.0] * 5), ([2] * 5, [25.0, -1.0, 25.0, 25.0, 900.0])):
            params = [c.view_params(degrees=15 + 50 * v, inc=incs[v], snr=snrs[v], seed=SEED + v, stream=v, conv_method=1) for v in range(5)]
            want = [c.simulate_view(gt, psfs[v].copy(), params[v])["acq"] for v in range(5)]
            before = c.transfer_stats()
            mine = [p.copy() for p in psfs]
            got = c.simulate_views(gt, mine, params)
            after = c.transfer_stats()
            for v in range(5):
                assert got[v].shape == want[v].shape and np.array_equal(got[v], want[v]), (incs, snrs, v)
                assert abs(float(mine[v].astype(np.float64).sum()) - 1.0) < 1e-6
            sampled = sum(1 for x in snrs if x >= 0)
            assert after[0] - before[0] == sampled and after[1] - before[1] == sum(1 for x in snrs if x > 500)
        assert c.simulate_views(gt, [], []) == []


def test_async_ground_truth_cache_is_dropped_when_the_staging_buffer_changes(mvs, synth):
    """the upload of a ground truth is skipped only while the staging set really holds it -- a view of another size
    (the staging buffer moves or is laid out differently) and a host block that went back to the allocator both invalidate
    the (pointer, generation) pair, whatever generation the caller keeps passing."""
    with mvs.Context(0) as c:
        small, big = synth.sphere_phantom(40), synth.sphere_phantom(56)
        psf = synth.gaussian_psf(7, sigma=(1.1, 1.2, 1.6))
        p = c.view_params(degrees=33, inc=2, snr=25.0, seed=SEED, stream=1)
        hs, hb = c.pinned_empty(small.shape), c.pinned_empty(big.shape)
        hs[...] = small
        hb[...] = big
        want_s = c.simulate_view(small, psf.copy(), p)["acq"]
        want_b = c.simulate_view(big, psf.copy(), p)["acq"]
        for src, want in ((hs, want_s), (hs, want_s), (hb, want_b), (hb, want_b), (hs, want_s), (hb, want_b), (hs, want_s)):
            out = {"acq": c.pinned_empty(want.shape)}
            c.wait(c.simulate_view_async(src, psf.copy(), p, out, gt_generation=0))
            assert np.array_equal(out["acq"], want)


def test_view_from_z_slab_host_buffers(ctx, synth):
    """mvsim_simulate_view_zslabs: ground truth and acquisition as lists of z slabs (the host convention for volumes
    beyond 2^31-1 voxels) -- same voxels as the single-buffer entry point."""
    gt = synth.sphere_phantom(40)
    psf = synth.gaussian_psf(7, sigma=(1.1, 1.2, 1.8))
    p = ctx.view_params(degrees=40, inc=3, snr=25.0, seed=SEED, stream=1)
    ref = ctx.simulate_view(gt, psf.copy(), p)
    acq, corr = ctx.simulate_view_zslabs([gt[:7], gt[7:30], gt[30:]], psf.copy(), p, [5, 1, 8])
    assert abs(corr - ref["corr"]) <= 1e-12 * corr
    assert np.array_equal(np.concatenate(acq, axis=0), ref["acq"])
    with pytest.raises(ValueError):
        ctx.simulate_view_zslabs([gt[:7], gt[7:30]], psf.copy(), p, [14])          # slabs do not add up to the volume


def test_stage_operators_from_z_slab_host_buffers(ctx, synth):
    """mvsim_{rotate_around_axis,attenuate3d,convolve,extract_slices}_zslabs: the per-stage operators the reference's call
    sites use (SimulateMultiViewDataset.java:570-585), with volumes handed over as lists of z slabs -- what the Java facade
    does beyond 2^29 voxels (one direct buffer holds 2 GiB, an ArrayImg four times that).  Same voxels as the single-buffer
    operators, for ragged slab lists on both sides; slab lists that do not add up are rejected."""
    gt = synth.sphere_phantom(48)
    cut = lambda a, edges: [a[lo:hi] for lo, hi in zip(edges, edges[1:])]
    rot = ctx.stage_zslabs("rotate", cut(gt, [0, 5, 6, 30, 48]), [20, 28], axis=0, degrees=33)
    assert np.array_equal(np.concatenate(rot), ctx.rotate_around_axis(gt, 0, 33))
    att = ctx.stage_zslabs("attenuate", cut(gt, [0, 47, 48]), [1, 47], delta=0.01)
    assert np.array_equal(np.concatenate(att), ctx.attenuate3d(gt, 0.01))
    psf = synth.gaussian_psf(7, sigma=(1.1, 1.2, 1.8))
    p1, p2 = psf.copy(), psf.copy()
    con = ctx.stage_zslabs("convolve", cut(gt, [0, 16, 32, 48]), [48], psf=p1, method=1)
    assert np.array_equal(np.concatenate(con), ctx.convolve(gt, p2, method=1)) and np.array_equal(p1, p2)
    ext = ctx.stage_zslabs("extract", cut(gt, [0, 24, 48]), [3, 13], inc=3, snr=25.0, seed=SEED, stream=2)
    assert np.array_equal(np.concatenate(ext), ctx.extract_slices(gt, 3, 25.0, SEED, 2))
    with pytest.raises(ValueError):
        ctx.stage_zslabs("rotate", cut(gt, [0, 24, 47]), [48], axis=0, degrees=10)       # input one plane short
    with pytest.raises(ValueError):
        ctx.stage_zslabs("extract", cut(gt, [0, 48]), [17], inc=3, snr=-1.0, seed=0)     # (48 - 1) / 3 + 1 = 16 planes


@pytest.mark.parametrize("shape,kshape", [((32, 32, 32), (9, 7, 7)), ((24, 40, 36), (5, 8, 6)), ((17, 23, 19), (7, 3, 5)),
                                          ((64, 48, 48), (31, 5, 5)), ((40, 30, 30), (3, 3, 3))])
def test_early_sum_from_the_spectrum_matches_pass_e(ctx, synth, options, shape, kshape):
    """adjustImage needs the sum of the convolved volume BEFORE the last pass can adjust on the fly; it is taken from the
    spectrum side (epilogue of the z pass: a weighted sum of the half spectrum) instead of from the voxels pass E
    produces.  Both estimate the same quantity from the same float32 spectrum; they must agree to ~1e-7, which moves
    isolated float roundings of the adjusted volume by one ulp and (rarely) a count."""
    rng = np.random.default_rng(sum(shape))
    gt = rng.random(shape, dtype=np.float32) * (rng.random(shape) < 0.3)
    psf = rng.random(kshape, dtype=np.float32) + 0.05
    p = ctx.view_params(degrees=20, inc=1, snr=25.0, seed=SEED, stream=1, conv_method=1)
    options(early_sum=1)
    a = ctx.simulate_view(gt, psf.copy(), p, want=("con", "acq"))
    options(early_sum=0)
    b = ctx.simulate_view(gt, psf.copy(), p, want=("con", "acq"))
    assert abs(a["corr"] - b["corr"]) <= 3e-7 * b["corr"], (a["corr"], b["corr"])
    assert np.max(np.abs(a["con"] - b["con"]) / b["con"]) <= 2.4e-7              # at most one ulp of float per voxel
    assert (a["acq"] != b["acq"]).mean() < 2e-3


@pytest.mark.parametrize("inc", [2, 3, 4, 7])
def test_compact_planes_view_equals_full_view(ctx, synth, options, inc):
    """With the sum known before the last two passes of the convolution (early sum), a view that does not return the
    adjusted volume only produces the planes k * inc that extractSlices reads.  With every plane still convolved
    (zconv_strided=0) the acquisition must equal the one of a view that materialises the whole volume (same planes through
    the same per-plane transforms, same RNG counters)."""
    gt = synth.sphere_phantom(40)
    psf = synth.gaussian_psf(7, 9, 11, sigma=(1.2, 1.4, 2.2))
    options(zconv_strided=0)
    for snr in (25.0, -1.0):
        p = ctx.view_params(degrees=35, inc=inc, snr=snr, seed=SEED, stream=4, conv_method=1)
        full = ctx.simulate_view(gt, psf.copy(), p, want=("con", "acq"))          # con requested: every plane is produced
        compact = ctx.simulate_view(gt, psf.copy(), p, want=("acq",))
        assert compact["acq"].shape == ((40 - 1) // inc + 1, 40, 40)
        assert np.array_equal(compact["acq"], full["acq"])
        assert compact["corr"] == full["corr"]
        if snr < 0:
            assert np.array_equal(compact["acq"], full["con"][::inc])


@pytest.mark.parametrize("shape,kshape", [((40, 40, 40), (7, 9, 11)), ((36, 44, 61), (5, 5, 31)), ((48, 48, 130), (9, 9, 63)),
                                          ((24, 24, 7), (3, 3, 5)), ((32, 32, 300), (3, 5, 64)), ((32, 32, 33), (3, 3, 1))])
@pytest.mark.parametrize("inc", [2, 3, 4])
def test_strided_z_pass_of_compact_views(ctx, synth, options, shape, kshape, inc):
    """Default for compact views (inc 2..4): the direct z pass convolves the planes k * inc alone, in polyphase order, and takes
    adjustImage's sum over ALL planes from its input rows (k_zconv_strided).  Same taps, other summation order: the adjusted
    planes agree with a full view's to float rounding, the factor to 1e-6, the counts except where a rounding moves one;
    and against the oracle's exact direct sum like every other form of the convolution."""
    nx, ny, nz = shape
    options(exp=2)                         # the strided kernel wherever its geometry allows, not only where the cost rule picks it
    rng = np.random.default_rng(nz * 7 + inc)
    gt = (rng.random((nz, ny, nx), dtype=np.float32) * (rng.random((nz, ny, nx)) < 0.4)).astype(np.float32)
    psf = (rng.random(kshape[::-1], dtype=np.float32) + 0.05).astype(np.float32)
    for snr in (-1.0, 25.0):
        p = ctx.view_params(degrees=20, inc=inc, snr=snr, seed=SEED, stream=3, conv_method=1)
        full = ctx.simulate_view(gt, psf.copy(), p, want=("con", "acq"))
        compact = ctx.simulate_view(gt, psf.copy(), p, want=("acq",))
        assert compact["acq"].shape == ((nz - 1) // inc + 1, ny, nx)
        assert abs(compact["corr"] - full["corr"]) <= 1e-6 * full["corr"], (compact["corr"], full["corr"])
        if snr < 0:
            ref = full["con"][::inc]
            assert np.max(np.abs(compact["acq"] - ref)) <= 3e-6 * float(ref.max())
        else:
            assert (compact["acq"] != full["acq"]).mean() < 2e-3
    options(zconv_strided=0)
    old = ctx.simulate_view(gt, psf.copy(), p, want=("acq",))
    assert np.array_equal(old["acq"], full["acq"])


@pytest.mark.parametrize("inc,want_con", [(1, False), (1, True), (3, False), (3, True)])
def test_fused_tail_option_gives_the_same_view(ctx, synth, options, inc, want_con):
    """Option fuse_tail (off by default: measured neutral): pass E of the convolution adjusts, extracts and runs
    phase 1 of the Poisson sampler in its epilogue instead of writing the convolved volume.  Same adjusted voxels, same
    RNG counters: identical acquisition, with and without noise, with and without the volume being returned."""
    gt = synth.sphere_phantom(48)
    psf = synth.gaussian_psf(9, 7, 11, sigma=(1.3, 1.2, 2.4))
    want = ("con", "acq") if want_con else ("acq",)
    for snr in (25.0, -1.0):
        p = ctx.view_params(degrees=70, inc=inc, snr=snr, seed=SEED, stream=6, conv_method=1)
        options(fuse_tail=0)
        a = ctx.simulate_view(gt, psf.copy(), p, want=want)
        options(fuse_tail=1)
        b = ctx.simulate_view(gt, psf.copy(), p, want=want)
        assert a["corr"] == b["corr"]
        for k in want:
            assert np.array_equal(a[k], b[k]), (k, snr)


@pytest.mark.parametrize("shape", [(4, 64, 64), (3, 200, 130), (5, 70, 70), (2, 300, 33), (6, 16, 16)])
@pytest.mark.parametrize("delta", [0.0, 0.01, 0.3])
def test_attenuate_prefix_scan_variant(ctx, orc, options, shape, delta):
    """Option attenuate=scan: the sweep as a wavefront-level prefix scan along y (products of the per-voxel factors) instead
    of one serial fp64 walk per column.  Same quantity, re-associated roundings: the float outputs equal the oracle's
    except for isolated one-ulp differences."""
    v = np.random.default_rng(2).random(shape, dtype=np.float32) * 4
    options(attenuate="scan")
    got = ctx.attenuate3d(v, delta)
    want = orc.attenuate3d(v, delta)
    diff = got != want
    assert diff.mean() < 1e-4, diff.mean()
    if diff.any():
        assert np.max(np.abs(got[diff] - want[diff]) / np.maximum(np.abs(want[diff]), 1e-30)) <= 1.2e-7
    if delta == 0.0:
        nz, ny, nx = shape
        assert np.array_equal(got[:, ny - nx:, :], v[:, ny - nx:, :]) and not got[:, :ny - nx, :].any()


def test_hipgraph_replay_of_views(mvs, synth):
    """Option graph: the launches of a view are captured into a hipGraph (second call with the same pointers and
    parameters) and replayed from the third call on; the PSF upload stays outside the graph.  Same voxels as the eager
    path, for several views interleaved (one graph each), after a workspace has grown (stale graphs are dropped), and
    with the PSF changing from call to call."""
    gt = synth.sphere_phantom(48)
    with mvs.Context(0) as c:
        d_gt = _dev_volume(c, gt)
        params = [c.view_params(degrees=20 + 70 * v, inc=1 + v, snr=25.0, seed=SEED, stream=v, conv_method=1) for v in range(3)]
        nzo = [(48 - 1) // p.inc + 1 for p in params]
        d_acq = [c.dev_alloc(k * 48 * 48 * 4) for k in nzo]
        psfs = [synth.gaussian_psf(9, sigma=(1.2, 1.3, 2.0 + 0.3 * r)) for r in range(4)]
        want = [[None] * 4 for _ in range(3)]
        for v in range(3):
            for r in range(4):
                c.simulate_view_dev(d_gt, (48, 48, 48), psfs[r].copy(), params[v], d_acq[v])
                want[v][r] = c.download(d_acq[v], (nzo[v], 48, 48))
        c.set_option("graph", 1)
        for r in range(4):                                  # round 0 eager, round 1 captures, rounds 2, 3 replay
            for v in range(3):
                c.simulate_view_dev(d_gt, (48, 48, 48), psfs[r].copy(), params[v], d_acq[v])
                assert np.array_equal(c.download(d_acq[v], (nzo[v], 48, 48)), want[v][r]), (v, r)
        # a larger view makes workspaces grow: the captured graphs (raw workspace addresses inside) must not be replayed
        big = synth.sphere_phantom(64)
        d_big = _dev_volume(c, big)
        d_big_acq = c.dev_alloc(big.nbytes)
        p_big = c.view_params(degrees=33, inc=1, snr=25.0, seed=SEED, stream=9, conv_method=1)
        c.simulate_view_dev(d_big, (64, 64, 64), psfs[0].copy(), p_big, d_big_acq)
        for v in range(3):
            c.simulate_view_dev(d_gt, (48, 48, 48), psfs[1].copy(), params[v], d_acq[v])
            assert np.array_equal(c.download(d_acq[v], (nzo[v], 48, 48)), want[v][1])
        corr = c.simulate_view_dev(d_gt, (48, 48, 48), psfs[1].copy(), params[0], d_acq[0], want_corr=True)
        assert corr > 0
        for d in [d_gt, d_big, d_big_acq] + d_acq:
            c.dev_free(d)


def test_main_loop_iteration_device_resident(mvs, orc, synth):
    """mvsim_simulate_iteration_dev = one pass through the body of `main`'s view loop (SimulateMultiViewDataset.java:567-613) without
    leaving HBM: the view, makeIsotropic, and the rotate-backs of the isotropic view, of computeWeightImage and of the PSF -- against
    the oracle's stage functions chained the same way (noise-free, so that every voxel can be compared: the view's convolution is
    float32-FFT accurate, everything behind it is bit-exact on identical input)."""
    nx, ny, nz, inc, deg, back = 40, 44, 36, 3, 60, -45
    gt = np.ascontiguousarray(synth.sphere_phantom(44)[4:40, :, 2:42])
    assert gt.shape == (nz, ny, nx)
    psf = synth.gaussian_psf(7, 7, 9, sigma=(1.2, 1.4, 2.5))
    want = orc.simulate_view(gt, psf.copy(), deg, inc=inc, snr=-1.0, seed=SEED, stream=0)
    pn = psf.copy()
    orc.norm_image(pn)
    nzo = orc.extract_nz(nz, inc)
    niso = (nzo - 1) * inc + 1
    with mvs.Context(0) as c:
        d_gt = _dev_volume(c, gt)
        bufs = {k: c.dev_alloc(n * 4) for k, n in (("acq", nx * ny * nzo), ("iso", nx * ny * niso), ("view", nx * ny * niso),
                                                     ("w", nx * ny * nz), ("psf", psf.size))}
        try:
            p = c.view_params(degrees=deg, inc=inc, snr=-1.0, seed=SEED, stream=0, conv_method=1)
            for _ in range(2):                                          # second pass: the cached weight image
                praw = psf.copy()
                c.simulate_iteration_dev(d_gt, (nx, ny, nz), praw, p, back, bufs["acq"], iso_dptr=bufs["iso"], view_dptr=bufs["view"],
                                         view_weights_dptr=bufs["w"], view_psf_dptr=bufs["psf"])
            acq = c.download(bufs["acq"], (nzo, ny, nx))
            iso = c.download(bufs["iso"], (niso, ny, nx))
            view = c.download(bufs["view"], (niso, ny, nx))
            vw = c.download(bufs["w"], (nz, ny, nx))
            vpsf = c.download(bufs["psf"], psf.shape)
            # a view without the optional outputs leaves the same acquisition
            c.simulate_iteration_dev(d_gt, (nx, ny, nz), psf.copy(), p, back, bufs["acq"], view_dptr=bufs["view"])
            assert np.array_equal(c.download(bufs["view"], (niso, ny, nx)), view)
        finally:
            for d in [d_gt] + list(bufs.values()):
                c.dev_free(d)
    assert np.array_equal(praw, pn)                                     # the PSF comes back normalised (Q5)
    scale = float(np.abs(want["acq"]).max())
    assert rel_to_max(acq, want["acq"]) <= CONV_TOL
    # behind the view everything is bit-exact on identical input: feed the oracle what the GPU produced
    assert np.array_equal(iso, orc.make_isotropic(acq, inc))
    assert np.array_equal(view, orc.rotate_around_axis(iso, 0, back))
    assert np.abs(view - orc.rotate_around_axis(orc.make_isotropic(want["acq"], inc), 0, back)).max() <= 2 * CONV_TOL * scale
    w = orc.compute_weight_image((nz, ny, nx))
    assert np.abs(vw - orc.rotate_around_axis(w, 0, back)).max() <= 2e-7
    assert np.array_equal(vpsf, orc.rotate_around_axis(pn, 0, back))


@pytest.mark.parametrize("shape,kshape", [((64, 80, 72), (9, 7, 5)), ((100, 128, 96), (31, 15, 11)), ((40, 48, 44), (39, 5, 5)),
                                          ((200, 96, 64), (63, 9, 7))])
def test_inline_fft_z_pass(mvs, orc, synth, shape, kshape):
    """fft_zpass=inline (k_fft_lines<CONVZ>): the z pass as FFT -> product -> inverse FFT on the UNPADDED spectrum -- mirrored halo
    planes through the index map, the PSF's z spectrum computed per tile and kept in registers, adjustImage's sum from its epilogue.
    What auto selects for deep PSFs on z lengths whose tiles fit twice per CU (configs[4]: 2048 x 2048 x 512, 63 taps).  Against the
    oracle's exact direct sum, and the fused view against the direct z pass (same sum, same compact planes)."""
    nz, ny, nx = shape
    rng = np.random.default_rng(5)
    v = synth.sphere_phantom(nx, ny, nz) + 0.01 * rng.random(shape, dtype=np.float32)
    psf = (synth.gaussian_psf(kshape[2], kshape[1], kshape[0], sigma=(kshape[2] / 6, kshape[1] / 6, kshape[0] / 5)) *
           (1 + 0.3 * rng.random(kshape, dtype=np.float32))).astype(np.float32)
    pn = psf.copy()
    orc.norm_image(pn)
    out = {}
    for zp in ("direct", "inline"):
        with mvs.Context(0) as c:
            c.set_option("fft_zpass", zp)
            con = c.convolve(v, psf.copy(), method=1)
            views = [c.simulate_view(v, psf.copy(), c.view_params(degrees=40, inc=inc, snr=snr, seed=SEED, stream=2, conv_method=1), want=("acq",))
                     for inc, snr in ((3, -1.0), (1, 25.0))]
            out[zp] = (con, views)
    scale = float(np.abs(out["direct"][0]).max())
    idx = np.unique(np.concatenate([np.arange(300), v.size - 1 - np.arange(300), rng.integers(0, v.size, 1500)]))
    want = orc.convolve_direct_at(v, pn, idx)
    for zp in ("direct", "inline"):
        assert float(np.abs(out[zp][0].ravel()[idx] - want).max()) <= CONV_TOL * scale, zp
    assert rel_to_max(out["inline"][0], out["direct"][0]) <= CONV_TOL
    (a0, a1), (b0, b1) = out["direct"][1], out["inline"][1]
    assert abs(a0["corr"] / b0["corr"] - 1) <= 1e-6                      # the sum from the epilogue of either z pass
    assert rel_to_max(b0["acq"], a0["acq"]) <= CONV_TOL
    assert np.mean(a1["acq"] != b1["acq"]) < 5e-3                        # counts: only where 1e-6 of lambda crosses a decision


@pytest.mark.parametrize("zrange,kshape,inc", [((100, 180), (31, 15, 15), 1), ((0, 40), (31, 15, 15), 3), ((230, 256), (63, 9, 9), 1),
                                               ((0, 256), (15, 15, 15), 1), ((128, 129), (15, 31, 31), 4)])
def test_empty_planes_are_skipped_exactly(mvs, synth, zrange, kshape, inc):
    """Option skip_empty (default): the fused rotate kernel flags the planes that hold a non-zero attenuated voxel, pass B skips the
    others, the z pass neither loads them nor computes z blocks that reach nothing else, passes D and E skip the planes whose taps reach
    only empty planes -- their spectra are exactly zero.  A specimen that occupies a slab of z (at a face, in the middle, a single plane,
    the whole volume), deep and shallow PSFs, compact planes: acquisition, adjusted volume and factor identical to skip_empty = 0."""
    nx, ny, nz = 512, 512, 256                                          # 2^26 voxels: the fused kernel runs (rotation about x keeps z slabs thin)
    rng = np.random.default_rng(9)
    gt = np.zeros((nz, ny, nx), np.float32)
    z0, z1 = zrange
    gt[z0:z1, 200:312, 64:448] = rng.random((z1 - z0, 112, 384), dtype=np.float32)
    psf = synth.gaussian_psf(kshape[2], kshape[1], kshape[0], sigma=(kshape[2] / 6, kshape[1] / 6, kshape[0] / 5))
    out = {}
    for skip in (0, 1):
        with mvs.Context(0) as c:
            c.set_option("skip_empty", skip)
            c.set_option("fft_zpass", "direct")
            d_gt = _dev_volume(c, gt)
            nzo = (nz - 1) // inc + 1
            d_acq, d_con, d_acq2 = c.dev_alloc(nx * ny * nzo * 4), c.dev_alloc(gt.nbytes), c.dev_alloc(nx * ny * nzo * 4)
            try:
                p = c.view_params(degrees=3, inc=inc, snr=25.0, seed=SEED, stream=1, conv_method=1)     # 3 degrees: the slab stays a slab
                corr = c.simulate_view_dev(d_gt, (nx, ny, nz), psf.copy(), p, d_acq, con_dptr=d_con, want_corr=True)
                c.simulate_view_dev(d_gt, (nx, ny, nz), psf.copy(), p, d_acq2)                         # compact planes when inc > 1
                out[skip] = (corr, c.download(d_acq, (nzo, ny, nx)), c.download(d_con, gt.shape), c.download(d_acq2, (nzo, ny, nx)))
            finally:
                for d in (d_gt, d_acq, d_con, d_acq2):
                    c.dev_free(d)
    a, b = out[0], out[1]
    assert a[0] == b[0]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert a[1].max() > 0


def test_overlap_options_keep_the_results(mvs, synth):
    """The library's two overlaps (psf_overlap, tail_overlap: DESIGN 4.5) against the serial order, with and without the fused rotate
    kernel: back-to-back views into distinct and shared outputs, a view that reads the previous view's output, a stage operator and
    a download right behind a view, a view whose requested `att` is the pending tail's output.  (Round 4's other co-scheduling forms
    -- guest waves, CU masks, a late-joined tail, kx panels -- were measured neutral or slower, profiles/r04_coschedule.txt, and left
    the library in round 5; the code is in the history at b8f3482.)"""
    nx, ny, nz = 512, 512, 64                                           # 2^24 voxels: the size from which the overlaps act
    gt = np.ascontiguousarray(synth.sphere_phantom(512)[224:288])
    psfs = [synth.gaussian_psf(15, sigma=(1.5, 1.7, 3.0 + 0.2 * v)) for v in range(4)]
    dim = (nx, ny, nz)

    def run(c):
        d_gt = _dev_volume(c, gt)
        acq = [c.dev_alloc(gt.nbytes) for _ in range(3)]
        params = [c.view_params(degrees=15 + 45 * v, inc=1, snr=25.0, seed=SEED, stream=v, conv_method=1) for v in range(4)]
        out = []
        for v in range(3):
            c.simulate_view_dev(d_gt, dim, psfs[v].copy(), params[v], acq[v])
        out += [c.download(a, gt.shape) for a in acq]
        for v in range(3):
            c.simulate_view_dev(d_gt, dim, psfs[v].copy(), params[v], acq[0])
        out.append(c.download(acq[0], gt.shape))
        c.simulate_view_dev(d_gt, dim, psfs[0].copy(), params[0], acq[1])
        c.simulate_view_dev(acq[1], dim, psfs[1].copy(), params[1], acq[2])        # reads what the previous tail has yet to write
        c.rotate_around_axis_dev(acq[2], dim, 0, 30, acq[0])
        out += [c.download(acq[2], gt.shape), c.download(acq[0], gt.shape)]
        c.simulate_view_dev(d_gt, dim, psfs[3].copy(), params[3], acq[1], att_dptr=acq[2])
        c.simulate_view_dev(d_gt, dim, psfs[2].copy(), params[2], acq[0], att_dptr=acq[1])  # `att` is the previous tail's output
        c.simulate_view_dev(d_gt, dim, psfs[1].copy(), params[1], acq[2])
        c.synchronize()
        out += [c.download(a, gt.shape) for a in acq]
        for d in [d_gt] + acq:
            c.dev_free(d)
        return out

    with mvs.Context(0) as c:
        c.set_option("tail_overlap", 0)
        c.set_option("psf_overlap", 0)
        want = run(c)
    assert want[0].mean() > 1.0
    variants = [
        {"tail_overlap": 1, "psf_overlap": 1},                                       # defaults: fused kernel from 131072 columns up
        {"tail_overlap": 1, "psf_overlap": 1, "fused_fftx": 0},                      # separate rotate kernel: the tail runs beside it
        {"tail_overlap": "any", "psf_overlap": 0, "fused_fftx": 0},
        {"tail_overlap": 1, "psf_overlap": 1, "fused_fftx": 1, "skip_empty": 0},
    ]
    for opts in variants:
        with mvs.Context(0) as c:
            for k, v in opts.items():
                c.set_option(k, v)
            got = run(c)
        for i, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, b), (opts, i)


def test_tail_overlap_keeps_stream_order_semantics(mvs, synth):
    """Option tail_overlap (the default from round 3 on; device views of >= 2^24 voxels on the context's own stream): the extract +
    Poisson tail of view v runs on a stream of its own beside the rotate+attenuate of view v+1.  Same voxels as the
    serial order for back-to-back views into distinct and into shared outputs, for a view whose INPUT is the previous
    view's output (the pending tail must be joined first), around a stage operator, a download and a caller's stream."""
    n = 256
    gt = synth.sphere_phantom(n)
    psfs = [synth.gaussian_psf(15, sigma=(1.5, 1.7, 3.0 + 0.2 * v)) for v in range(4)]

    def run(c):
        d_gt = _dev_volume(c, gt)
        acq = [c.dev_alloc(gt.nbytes) for _ in range(3)]
        params = [c.view_params(degrees=15 + 45 * v, inc=1, snr=25.0, seed=SEED, stream=v, conv_method=1) for v in range(4)]
        out = []
        for v in range(3):                                              # distinct outputs, nothing in between
            c.simulate_view_dev(d_gt, (n, n, n), psfs[v].copy(), params[v], acq[v])
        out += [c.download(a, (n, n, n)) for a in acq]
        for v in range(3):                                              # the same output three times: the last one stays
            c.simulate_view_dev(d_gt, (n, n, n), psfs[v].copy(), params[v], acq[0])
        out.append(c.download(acq[0], (n, n, n)))
        c.simulate_view_dev(d_gt, (n, n, n), psfs[0].copy(), params[0], acq[1])
        c.simulate_view_dev(acq[1], (n, n, n), psfs[1].copy(), params[1], acq[2])      # reads what the pending tail writes
        c.rotate_around_axis_dev(acq[2], (n, n, n), 0, 30, acq[0])      # a stage operator right behind a view
        out += [c.download(acq[2], (n, n, n)), c.download(acq[0], (n, n, n))]
        c.simulate_view_dev(d_gt, (n, n, n), psfs[3].copy(), params[3], acq[1], att_dptr=acq[2])
        c.simulate_view_dev(d_gt, (n, n, n), psfs[2].copy(), params[2], acq[0], att_dptr=acq[1])  # writes the pending tail's output
        out += [c.download(acq[0], (n, n, n)), c.download(acq[1], (n, n, n))]
        for d in [d_gt] + acq:
            c.dev_free(d)
        return out

    with mvs.Context(0) as c:
        c.set_option("tail_overlap", 0)
        want = run(c)
    with mvs.Context(0) as c:
        c.set_option("tail_overlap", 1)
        c.set_option("psf_overlap", 1)
        got = run(c)
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), i
    # a caller's stream: off unless opted in; with "any", mvsim_join orders the tail in front of the caller's next work
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")                                 # the runtime libmvsim.so itself is linked against
    stream = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
    with mvs.Context(0) as c:
        c.set_stream(stream.value)
        c.set_option("tail_overlap", "any")
        d_gt = _dev_volume(c, gt)
        acq, mine = c.dev_alloc(gt.nbytes), c.dev_alloc(gt.nbytes)
        p = c.view_params(degrees=15, inc=1, snr=25.0, seed=SEED, stream=0, conv_method=1)
        for _ in range(2):
            c.simulate_view_dev(d_gt, (n, n, n), psfs[0].copy(), p, acq)
        c.join()
        # the caller's own work on its stream: a device-to-device copy of the acquisition (hipMemcpyDeviceToDevice = 3)
        assert hip.hipMemcpyAsync(ctypes.c_void_p(mine), ctypes.c_void_p(acq), ctypes.c_size_t(gt.nbytes), 3, stream) == 0
        assert hip.hipStreamSynchronize(stream) == 0
        assert np.array_equal(c.download(mine, (n, n, n)), want[0])
        for d in (d_gt, acq, mine):
            c.dev_free(d)
    assert hip.hipStreamDestroy(stream) == 0


def test_bench_rehearses_the_multi_gpu_data_path(tmp_path):
    """bench.py --rehearse-multi: the control flow of N > 1 on the one GPU -- a second ground-truth buffer, torch-owned view
    and broadcast streams, the C ABI's own RCCL communicator (one rank) and one mvsim_comm_broadcast_volume per step issued a
    dataset ahead, in both broadcast forms and with the tail overlap on a caller's stream.  The line it prints is a rehearsal,
    not a result; what is checked is that the path runs and leaves the ground truth and the acquisitions intact (the
    script's own assertion) and that the line says which collective ran."""
    import json
    import subprocess
    import sys
    bench = os.path.join(ROOT, "bench.py")
    # one form per run (--no-broadcast-ab: the line times --broadcast's form and nothing else), then the default: the line's own form and
    # the other forms back to back in one invocation, the fastest reported (multi_gpu.broadcast_ab)
    for extra in (["--broadcast", "scatter_allgather", "--no-broadcast-ab"], ["--broadcast", "ring", "--serial", "--no-broadcast-ab"],
                  ["--broadcast", "peer_copy", "--no-broadcast-ab"], ["--broadcast", "pipelined", "--no-broadcast-ab"], []):
        r = subprocess.run([sys.executable, bench, "--rehearse-multi", "--size", "256", "--psf", "15", "--steps", "2", "--warmup", "1",
                            "--no-cpu-baseline", "--full"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
        d = json.loads(line)
        assert "rehearsal" in d and d["value"] > 0 and "mvsim_comm_broadcast_volume" in d["config"]["collective"]
        if extra:
            assert extra[1] in d["config"]["collective"] and "broadcast_ab" not in d["multi_gpu"]
        else:
            ab = d["multi_gpu"]["broadcast_ab"]
            assert sorted(ab) == ["peer_copy", "pipelined", "scatter_allgather"] and all(rec["ms_per_step"] > 0 for rec in ab.values())
            chosen = d["multi_gpu"]["broadcast_chosen"]
            assert chosen in d["config"]["collective"] and abs(d["ms_per_step"] - ab[chosen]["ms_per_step"]) < 1e-3
            assert ab[chosen]["ms_per_step"] == min(rec["ms_per_step"] for rec in ab.values())
        assert d["config"]["rccl"]["libmvsim"]["version_code"] > 0 and d["config"]["rccl"]["libmvsim"]["path"]
        assert ("off" in d["config"]["overlap"]) == ("--serial" in extra)
        # what makes a scaling run attributable: per-step broadcast / view times and every rank's own clock
        mg = d["multi_gpu"]
        assert mg["broadcast_ms"] >= 0 and mg["views_ms"] > 0 and len(mg["per_rank"]) == 1 and mg["ms_per_step_max"] >= mg["ms_per_step_min"] > 0
        # the other legs of the N > 1 data path, at twice the edge (1024^3 for the line of record, 512^3 here): views sharded v % N
        # with their own broadcast, and BASELINE configs[3] -- every view cut into N z slabs, the sum reduced by the C ABI's collective
        big, tiled = d["size_512"], d["tiled_512"]
        assert big["value"] > 0 and big["multi_gpu"]["views_ms"] > 0 and "512^3" in big["workload"]
        # (the slab sum is reduced on the device inside mvsim_view_slab_dev since round 6; ranks that share a GPU fall back to the host form)
        assert tiled["value"] > 0 and "31x31x63" in tiled["workload"]
        assert "mvsim_view_slab_dev" in tiled["reduction"] or "mvsim_comm_allreduce_sum_f64" in tiled["reduction"]
        # (one asynchronous call per view: the whole slab shows up in the wait behind it, finish_ms_per_view)
        assert len(tiled["per_rank"]) == 1 and tiled["per_rank"][0]["planes_owned"] == 512 and "mvsim_view_slab_dev" in tiled["path"]
        assert tiled["per_rank"][0]["slab_convolve_ms_per_view"] + tiled["per_rank"][0]["finish_ms_per_view"] > 0


@pytest.mark.parametrize("shape,kshape,degrees,inc", [((40, 64, 64), (9, 5, 7), 33, 1),       # one wave per row batch
                                                      ((50, 160, 128), (11, 7, 5), -52, 3),   # Ny > Nx: rows the attenuation never visits
                                                      ((48, 200, 192), (31, 9, 15), 60, 2),   # three waves: rows wrap round the waves
                                                      ((64, 256, 256), (15, 15, 15), 15, 1),
                                                      ((33, 100, 100), (5, 5, 5), 90, 1),     # Nx not a multiple of 64 (inactive lanes)
                                                      ((20, 700, 640), (7, 9, 31), 25, 1),    # ten waves: two batches per transform round
                                                      ((12, 1024, 1024), (5, 5, 15), -40, 2)])  # sixteen waves, 128-row geometry chunks
def test_fused_rotate_attenuate_x_transform_is_bit_identical(mvs, synth, shape, kshape, degrees, inc):
    """rotate + attenuate + pass A of the convolution as one kernel (rotate_fft.hip, option fused_fftx): the attenuated volume
    no longer crosses HBM, and nothing else changes -- the spectrum it leaves is pass A's bit for bit, so rot, att, the
    adjusted convolved volume and the counts are IDENTICAL to the separate kernels', with and without the intermediates
    requested (the kernel's store-nothing instance)."""
    rng = np.random.default_rng(77)
    gt = synth.sphere_phantom(shape[2], shape[1], shape[0]) + (rng.random(shape, dtype=np.float32) < 0.02).astype(np.float32)
    psf = rng.random(kshape, dtype=np.float32) + 0.05
    res = {}
    for mode in (0, 1):
        with mvs.Context(0) as c:
            c.set_option("fused_fftx", mode)
            p = c.view_params(degrees=degrees, inc=inc, snr=25.0, seed=SEED, stream=3, conv_method=1)
            full = c.simulate_view(gt, psf.copy(), p, want=("rot", "att", "con", "acq"))
            only = c.simulate_view(gt, psf.copy(), p, want=("acq",))
            res[mode] = (full, only)
    for k in ("rot", "att", "con", "acq"):
        assert np.array_equal(res[0][0][k], res[1][0][k]), k
    assert np.array_equal(res[0][1]["acq"], res[1][1]["acq"])
    assert float(res[1][0]["acq"].max()) > 0


@pytest.mark.parametrize("shape,kshape,degrees,inc,fused", [((8, 600, 600), (5, 9, 7), 20, 1, 0),      # y lines of 640 points, separate kernels
                                                           ((8, 700, 700), (7, 9, 31), 25, 1, 1),     # 720 points, fused kernel: mirrored halo rows from their mirror images
                                                           ((6, 1030, 1030), (5, 15, 9), -35, 2, 0),  # 1080 points, compact planes in pass D
                                                           ((3, 2060, 2060), (3, 63, 5), 60, 1, 0)])  # 2160 points: one block per CU
def test_paired_y_tiles_of_long_lines_are_bit_identical(mvs, synth, orc, shape, kshape, degrees, inc, fused):
    """Round 6: on lines of more than 576 points the y passes move 8-column tiles (64-byte rows), and the two tiles of a 128-byte line
    now go to ONE XCD, one behind the other in its dispatch order (k_fft_lines; in grid order both XCDs' L2s fetched the whole line:
    profiles/r06_fetch_calibration.txt).  Only which block takes which tile changes: the adjusted convolved volume and the counts are
    identical to the grid order (option exp bit 4), and meet the convolution's contract against the oracle."""
    rng = np.random.default_rng(91)
    gt = synth.sphere_phantom(shape[2], shape[1], shape[0]) + (rng.random(shape, dtype=np.float32) < 0.03).astype(np.float32)
    psf = rng.random(kshape, dtype=np.float32) + 0.05
    res = {}
    # (exp bit 8: the whole-length 8-column tiles also where the library would split the line into two half-length transforms -- the
    # 1080- and 2160-point cases, test_split_y_lines_agree_with_the_single_transform; bit 4: those tiles in plain grid order)
    for exp in (8, 12):
        with mvs.Context(0) as c:
            c.set_option("exp", exp)
            c.set_option("fused_fftx", fused)
            p = c.view_params(degrees=degrees, inc=inc, snr=25.0, seed=SEED, stream=2, conv_method=1)
            res[exp] = (c.simulate_view(gt, psf.copy(), p, want=("att", "con", "acq")), c.simulate_view(gt, psf.copy(), p, want=("acq",)))
    assert float(res[8][0]["att"].max()) > 0 and not np.isnan(res[8][0]["con"]).any()
    for k in ("att", "con", "acq"):
        assert np.array_equal(res[8][0][k], res[12][0][k]), k
    assert np.array_equal(res[8][1]["acq"], res[12][1]["acq"])
    res[0] = res[8]
    want = orc.convolve_fft(res[0][0]["att"], psf.copy())
    got = res[0][0]["con"]
    # con is the ADJUSTED volume: undo Tools.adjustImage's scale and offset (approximately) before comparing
    scale = float((got.astype(np.float64) - 1e-4).sum() / want.astype(np.float64).sum())
    assert rel_to_max((got - np.float32(1e-4)) / np.float32(scale), want) <= 5 * CONV_TOL
    assert float(res[0][0]["acq"].max()) > 0


@pytest.mark.parametrize("shape,kshape,degrees,inc,fused", [((4, 2010, 2010), (3, 31, 5), 20, 1, 0),     # y lines of 2048 points = 2 x 1024, separate kernels
                                                           ((3, 2000, 2000), (3, 31, 7), -25, 1, 1),    # 2048 = 2 x 1024, fused kernel (16 waves): mirrored halo rows
                                                           ((6, 2060, 2060), (5, 63, 5), 60, 3, 0),     # 2160 = 2 x 1080 (configs[4]'s lines), compact planes in pass D
                                                           ((3, 2200, 2200), (3, 31, 5), 10, 1, 0)])    # 2240 = 2 x 1120: two tiles of 81 KB per CU
def test_split_y_lines_agree_with_the_single_transform(mvs, synth, orc, shape, kshape, degrees, inc, fused):
    """Round 6: y lines of 2048 / 2160 / 2240 points (whose 8-line tile leaves a CU room for one block only) are transformed as TWO
    half-length transforms (k_fft_lines_split: the first radix-2 stage in registers as the rows arrive, then e and o through a
    half-length tile one after the other -- two blocks per CU).  Another factorisation of the same transform: the adjusted convolved volume agrees with the one-block
    form (option exp=8) to rounding, far inside the convolution's contract, which both meet against the oracle; the counts follow
    their lambdas (a count moves where a rounding moves a lambda across a decision of the sampler: ~1e-4 of the voxels)."""
    rng = np.random.default_rng(92)
    gt = synth.sphere_phantom(shape[2], shape[1], shape[0]) + (rng.random(shape, dtype=np.float32) < 0.03).astype(np.float32)
    psf = rng.random(kshape, dtype=np.float32) + 0.05
    res = {}
    for exp in (0, 8):
        with mvs.Context(0) as c:
            c.set_option("exp", exp)
            c.set_option("fused_fftx", fused)
            p = c.view_params(degrees=degrees, inc=inc, snr=25.0, seed=SEED, stream=2, conv_method=1)
            res[exp] = c.simulate_view(gt, psf.copy(), p, want=("att", "con", "acq"))
    assert float(res[0]["att"].max()) > 0 and not np.isnan(res[0]["con"]).any()
    assert np.array_equal(res[0]["att"], res[8]["att"])
    assert rel_to_max(res[0]["con"], res[8]["con"]) <= 2e-6
    assert np.mean(res[0]["acq"] != res[8]["acq"]) < 1e-3            # (where a rejection flips, the count is another draw altogether)
    want = orc.convolve_fft(res[0]["att"], psf.copy())
    for exp in (0, 8):
        got = res[exp]["con"]
        scale = float((got.astype(np.float64) - 1e-4).sum() / want.astype(np.float64).sum())
        assert rel_to_max((got - np.float32(1e-4)) / np.float32(scale), want) <= 5 * CONV_TOL, exp


def test_split_y_lines_in_place_behind_the_padded_z_transform(mvs, synth, orc):
    """k_fft_lines_split where the y passes run IN PLACE on a z-padded spectrum (option fft_zpass=fft: the formulation for PSFs deeper
    than 64 taps): a block reads every row of its tile before it stores the first, so rows 2k / 2k + 1 may overwrite rows n / n + L/2;
    the planes of the z gap are skipped by the outer index map.  Against the one-block form (exp=8) and the oracle."""
    shape, kshape = (5, 2010, 2010), (5, 31, 7)
    rng = np.random.default_rng(93)
    v = (synth.sphere_phantom(shape[2], shape[1], shape[0]) + (rng.random(shape, dtype=np.float32) < 0.03)).astype(np.float32)
    psf = rng.random(kshape, dtype=np.float32) + 0.05
    res = {}
    for exp in (0, 8):
        with mvs.Context(0) as c:
            c.set_option("exp", exp)
            c.set_option("fft_zpass", "fft")
            res[exp] = c.convolve(v, psf.copy(), method=1)
    want = orc.convolve_fft(v, psf.copy())
    assert rel_to_max(res[0], res[8]) <= 2e-6
    for exp in (0, 8):
        assert rel_to_max(res[exp], want) <= CONV_TOL, exp


def test_bench_line_carries_the_contract_keys():
    """bench.py --full's one JSON line (small volume, so that the test stays short): the contract keys, `value` on the library
    defaults with a serial leg beside it, a roofline whose fused-byte fractions never exceed 1 and that says where the x
    transform ran, a two-mode CPU baseline labelled as a port; and with --conv-method 2 the direct stencil against the fp32
    vector peak."""
    import json
    import subprocess
    import sys
    bench = os.path.join(ROOT, "bench.py")
    r = subprocess.run([sys.executable, bench, "--size", "256", "--psf", "15", "--steps", "2", "--warmup", "1", "--cpu-slab", "8",
                        "--no-end-to-end", "--no-two-streams", "--full"], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, MVSIM_OPTIONS="fused_fftx=1"))       # (auto takes the fused kernel from 131072 columns up)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline", "serial"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["vs_baseline"] is None and d["higher_is_better"] is True and "workload" in d["config"]
    rl = d["roofline"]
    assert rl["bound"] == "hbm" and rl["unit"] == "GB/s" and rl["peak"] == 8000.0 and abs(rl["frac"] - rl["achieved"] / rl["peak"]) < 1e-9
    assert rl["x_transform_in_rotate_kernel"] is True and rl["stage_ms"]["pass_a_ms"] == 0.0
    for st in rl["stages"].values():
        assert 0 < st["frac_fused"] <= 1.0 and st["fused_bytes"] <= st["algorithmic_bytes"]
    assert 0 < rl["whole_view"]["frac_fused"] <= 1.0
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and set(cb["modes"]) == {"as_reference", "all_cores"} and cb["value"] == cb["modes"]["as_reference"]["value"]
    assert cb["modes"]["as_reference"]["extrapolated_fraction_of_seconds"] == 0.0 and "not the JVM" in cb["what"]
    r = subprocess.run([sys.executable, bench, "--conv-method", "2", "--size", "128", "--psf", "15", "--steps", "1", "--warmup", "1", "--serial",
                        "--no-cpu-baseline"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    rl = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["roofline"]
    assert rl["bound"] == "fp32" and rl["unit"] == "TFLOP/s" and rl["peak"] == 157.3 and 0 < rl["frac"] < 1
    assert rl["flop"] == 2.0 * 15 ** 3 * 128 ** 3 and rl["stencil_geometry"]["blocks_per_cu"] == 2


def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """bench.py without --full: the line of record and nothing beside it (no serial leg, roofline, CPU baseline or other record), over
    exactly --steps timed steps; --dump-outputs writes the acquisitions of the last timed step as float32 .npy files, and two runs with
    the same arguments write the same arrays.  Views larger than their share of the dump's budget are written as a fixed sample."""
    import json
    import subprocess
    import sys
    bench = os.path.join(ROOT, "bench.py")

    def run(size, steps, out_dir):
        r = subprocess.run([sys.executable, bench, "--size", str(size), "--psf", "15", "--steps", str(steps), "--warmup", "1",
                            "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    dumps = []
    for k in range(2):
        d = run(64, 3, tmp_path / f"whole{k}")
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in d, key
        assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["higher_is_better"] is True and d["value_dense"] is None
        assert abs(d["value"] - 8 * 64 ** 3 / d["ms_per_step"] / 1e3) <= 1e-9 * d["value"]
        for key in ("serial", "roofline", "cpu_baseline", "no_empty_space", "poisson_queue", "main_iteration", "two_streams",
                    "end_to_end", "size_1024", "small_views"):
            assert key not in d, key
        files = sorted(os.listdir(tmp_path / f"whole{k}"))
        assert files == sorted(f"acq_view{v}.npy" for v in range(8))
        arrs = {f: np.load(tmp_path / f"whole{k}" / f) for f in files}
        for a in arrs.values():
            assert a.dtype == np.float32 and a.shape == (64, 64, 64) and float(a.max()) > 0      # 2^18 voxels: whole views
        dumps.append(arrs)
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f], dumps[1][f]), f
    run(128, 1, tmp_path / "sampled")                 # 2^21 voxels a view, 2^20 of them written
    paths = [tmp_path / "sampled" / f"acq_view{v}.npy" for v in range(8)]
    assert sum(os.path.getsize(p) for p in paths) <= 64 << 20
    for p in paths:
        a = np.load(p)
        assert a.dtype == np.float32 and a.shape == (1 << 20,) and float(a.max()) > 0


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher around it: bench.py starts the two ranks itself (children with RANK /
    WORLD_SIZE / MASTER_* set, before anything touches the GPU in the parent) and rank 0's line says n_gpus 2 with both
    ranks seen by an all-reduce.  Two ranks share the one GPU of this box, so the process group is gloo and the ground truth
    travels through torch.distributed.broadcast (RCCL cannot place two ranks on one device); on an 8-GPU node the same
    command line with the default backend runs one rank per GPU over RCCL."""
    import json
    import subprocess
    import sys
    bench = os.path.join(ROOT, "bench.py")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, bench, "--gpus", "2", "--backend", "gloo", "--size", "256", "--psf", "15", "--steps", "2",
                        "--warmup", "1", "--no-cpu-baseline", "--full"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["config"]["ranks_seen"]["torch"] == 2
    assert d["config"]["launcher"].startswith("self-launched") and d["config"]["views_this_gpu"] == 4
    assert "torch.distributed.broadcast (gloo)" in d["config"]["collective"]
    assert d["roofline"]["stages"]["convolve"]["ms"] > 0
    # configs[3]'s tiled leg with two real ranks: each owns half of the planes and recomputes the PSF's halo beside them
    tiled = d["tiled_512"]
    assert len(tiled["per_rank"]) == 2 and all(r["planes_owned"] == 256 and r["planes_rotated"] > 256 for r in tiled["per_rank"])
    assert 0 < tiled["per_rank"][0]["halo_recompute_share"] < 0.2 and "torch.distributed.all_reduce" in tiled["reduction"]
    assert len(d["size_512"]["multi_gpu"]["per_rank"]) == 2 and d["size_512"]["value"] > 0


def test_tiled_view_two_gloo_ranks_on_one_gpu():
    """BASELINE configs[3]'s rank-level path (multiview-simulation_amd/tiling.py through examples/tiled_view.py) with two real
    processes sharing this box's GPU: each rank rotates, attenuates and convolves its z slab of a 256^3 view (31 x 31 x 63 taps would
    not leave two slabs their halo at this size: 15 x 15 x 41), the one double of adjustImage's sum is all-reduced between them, and
    the stitched acquisition equals the untiled view (the script's own --check).  On gloo the double travels through
    torch.distributed; with the default backend (one rank per GPU) it goes through mvsim_comm_allreduce_sum_f64."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29546", os.path.join(ROOT, "examples", "tiled_view.py"), "--size", "256", "--psf", "15", "15", "41",
                        "--inc", "4", "--backend", "gloo", "--check"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "rank 0: planes [0,128)" in r.stdout and "rank 1: planes [128,256)" in r.stdout and "of the counts differ" in r.stdout


def test_example_simulate_dataset_runs(tmp_path):
    """examples/simulate_dataset.py -- the whole driver of SimulateMultiViewDataset.main (:524-663) on the GPU path through the
    package's mirror of the reference's static methods -- runs and writes every image `main` writes."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "simulate_dataset.py"), "--size", "48", "--views", "3", "--psf", "9",
                        "--out", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    z = np.load(tmp_path / "dataset.npz")
    for name in ("rendered", "groundtruth", "rot_view_0", "att_view_0", "con_view_0", "acq_view_0", "iso_view_0", "aligned_view_0",
                 "aligned_view_psf_0", "aligned_view_weights0", "sum_weights"):
        assert name in z.files, name
    assert z["acq_view_0"].shape == (16, 48, 48) and z["acq_view_0"].max() > 0 and np.all(z["acq_view_0"] == np.round(z["acq_view_0"]))
    assert z["sum_weights"].max() <= 3.0 + 1e-5 and z["iso_view_0"].shape == (46, 48, 48)


def test_simulate_views_dev_equals_sequential_views(mvs, synth):
    """mvsim_simulate_views_dev (the view loop of `main`, SimulateMultiViewDataset.java:567-585, for views that cannot fill the chip
    one at a time): V views of one ground truth in one call.  STACKED (view_batch: one launch per stage for all views, the view index
    in the grids) or, where the views do not allow that (an adjusted volume requested), on LANES (view_lanes child contexts side by
    side) -- every acquisition and every requested adjusted volume bit-identical to V sequential mvsim_simulate_view_dev calls: even
    and odd plane sizes (the sampler's 16-byte and group-by-group forms), inc 1..3 (whole and compact planes, the strided z pass), more
    views than lanes; a second batch of another geometry through the same context; overlapping outputs rejected."""
    with mvs.Context(0) as c:
        for (n, k, inc, nv) in ((64, 9, 1, 8), (97, 11, 3, 7), (128, 15, 2, 5), (50, 7, 1, 3)):
            gt = synth.sphere_phantom(n)
            nzo = (n - 1) // inc + 1
            psfs = [synth.gaussian_psf(k, sigma=(1.2, 1.4, 2.0 + 0.1 * v)) for v in range(nv)]
            d_gt = _dev_volume(c, gt)
            acq = [c.dev_alloc(nzo * n * n * 4) for _ in range(nv)]
            con = [c.dev_alloc(gt.nbytes) for _ in range(nv)]
            params = [c.view_params(degrees=15 + 50 * v, inc=inc, snr=25.0, seed=SEED, stream=v, conv_method=1) for v in range(nv)]
            try:
                for v in range(nv):
                    c.simulate_view_dev(d_gt, (n, n, n), psfs[v].copy(), params[v], acq[v])
                want = [c.download(a, (nzo, n, n)) for a in acq]
                for v in range(nv):
                    c.simulate_view_dev(d_gt, (n, n, n), psfs[v].copy(), params[v], acq[v], con_dptr=con[v])
                want_con = [c.download(x, gt.shape) for x in con]
                assert want[0].max() > 0
                for batch, lanes, with_con in ((1, "auto", False), ("auto", "auto", False), (0, 1, False), (0, 2, False), (0, 3, True), (1, 8, True)):
                    for a in acq:
                        c.upload(a, np.full((nzo, n, n), -1.0, np.float32))
                    c.set_option("view_batch", batch)
                    c.set_option("view_lanes", lanes)
                    mine = [p.copy() for p in psfs]
                    c.simulate_views_dev(d_gt, (n, n, n), mine, params, acq, con_dptrs=[con[v] if v % 2 else 0 for v in range(nv)] if with_con else None)
                    for v in range(nv):
                        got = c.download(acq[v], (nzo, n, n))
                        if with_con:
                            # (a materialised adjusted volume changes nothing in the counts of a whole-plane view; compact views take
                            # another z pass -- compare those with their own kind)
                            if v % 2:
                                assert np.array_equal(c.download(con[v], gt.shape), want_con[v]), (n, batch, lanes, v)
                            if inc == 1:
                                assert np.array_equal(got, want[v]), (n, batch, lanes, v)
                        else:
                            assert np.array_equal(got, want[v]), (n, batch, lanes, v)
                        assert abs(float(mine[v].astype(np.float64).sum()) - 1.0) < 1e-6      # normalised in place (Q5)
                with pytest.raises(ValueError, match="overlap"):
                    c.simulate_views_dev(d_gt, (n, n, n), [p.copy() for p in psfs[:2]], params[:2], [acq[0], acq[0]])
                with pytest.raises(ValueError, match="overlap"):
                    c.simulate_views_dev(d_gt, (n, n, n), [p.copy() for p in psfs[:2]], params[:2], [acq[0], d_gt])
            finally:
                for d in [d_gt] + acq + con:
                    c.dev_free(d)


def test_stacked_views_that_share_one_psf_buffer(mvs, synth):
    """`mvsim_simulate_views_dev(..., [psf] * V, ...)` -- every view names the SAME PSF memory.  Sequential calls normalise that
    buffer V times, one after the other (Tools.normImage in place, SMVD:255; after the first pass the sum is 1 up to rounding, so the
    later passes move single ulps), and the stacked path does the same, in view order, instead of normalising it from V host threads at
    once: acquisitions and the buffer itself are bit-identical to the sequential calls, run after run."""
    n, k, nv = 64, 9, 8
    gt = synth.sphere_phantom(n)
    raw = synth.gaussian_psf(k, sigma=(1.2, 1.4, 2.2))
    with mvs.Context(0) as c:
        d_gt = _dev_volume(c, gt)
        acq = [c.dev_alloc(gt.nbytes) for _ in range(nv)]
        params = [c.view_params(degrees=15 + 45 * v, inc=1, snr=25.0, seed=SEED, stream=v, conv_method=1) for v in range(nv)]
        try:
            shared = raw.copy()
            for v in range(nv):
                c.simulate_view_dev(d_gt, (n, n, n), shared, params[v], acq[v])
            want = [c.download(a, gt.shape) for a in acq]
            want_psf = shared.copy()
            for rep in range(3):
                for a in acq:
                    c.upload(a, np.full(gt.shape, -1.0, np.float32))
                c.set_option("view_batch", 1)
                mine = raw.copy()
                c.simulate_views_dev(d_gt, (n, n, n), [mine] * nv, params, acq)
                assert np.array_equal(mine, want_psf), rep
                for v in range(nv):
                    assert np.array_equal(c.download(acq[v], gt.shape), want[v]), (rep, v)
        finally:
            for d in [d_gt] + acq:
                c.dev_free(d)


@pytest.mark.parametrize("seed", range(12))
def test_random_geometries_against_oracle(mvs, orc, seed):
    """Random volume shapes (Nx <= Ny, odd and even, not multiples of the 16-row / 16-column tiles), PSF shapes, angles,
    spacings and the three ways a view can leave the convolution (whole planes, acquired planes only, materialised volume):
    rot/att bit-exact, con within 1e-5 of the oracle's FFTConvolution recipe, counts bit-exact on identical lambda.  A fresh
    context per case, so that workspaces of one geometry are never reused by the next by accident."""
    rng = np.random.default_rng(9000 + seed)
    nx = int(rng.integers(12, 72))
    ny = int(rng.integers(nx, 96))
    nz = int(rng.integers(10, 80))
    kd = [int(min(2 * rng.integers(0, 11) + 1, 2 * ((d - 1) // 2) - 1 if d > 3 else 1)) for d in (nx, ny, nz)]
    kd = [max(1, k) for k in kd]
    gt = (rng.random((nz, ny, nx), dtype=np.float32) ** 3) * (rng.random() < 0.8) + rng.random((nz, ny, nx), dtype=np.float32) * 0.05
    psf = rng.random((kd[2], kd[1], kd[0]), dtype=np.float32) + 0.05
    degrees = int(rng.integers(-170, 171))
    inc = int(rng.integers(1, 5))
    with mvs.Context(0) as c:
        # ... and the sampler's work queue in every size: full (the default), a sixteenth of it, an eighth, five sixteenths -- the small
        # ones refuse voxels on these volumes (two thirds of the cases have no empty voxel), which the third kernel then samples
        c.set_option("poisson_queue_share", (16, 1, 2, 5)[seed % 4])
        got, _ = _view_against_oracle(c, orc, gt.astype(np.float32), psf, degrees=degrees, inc=inc, stream=seed)
        # the same view without materialised intermediates (compact planes when inc > 1) gives the same acquisition as the
        # one that wrote `con` -- up to the count flips of the two summation orders of adjustImage's mean
        p = c.view_params(degrees=degrees, delta=REF_DELTA, inc=inc, snr=25.0, seed=SEED, stream=seed, conv_method=1)
        only = c.simulate_view(gt.astype(np.float32), psf.copy(), p)
        assert only["acq"].shape == got["acq"].shape
        assert np.mean(only["acq"] != got["acq"]) < 2e-3


def test_graph_capture_with_the_side_stream_options(mvs, synth):
    """hipGraph replay of a view whose capture forks to the context's side stream (psf_overlap: PSF spectrum beside passes
    A and B, joined before the z pass) -- and with tail_overlap asked for as well, which graph mode switches off: the same
    voxels as the plain serial order, eager (first call), captured (second) and replayed (third, fourth)."""
    n = 256
    gt = synth.sphere_phantom(n)
    psf = synth.gaussian_psf(15, sigma=(1.5, 1.7, 3.0))
    outs = {}
    for name, opts in (("plain", {}), ("graph+psf", {"graph": 1, "psf_overlap": 1}),
                       ("graph+psf+tail", {"graph": 1, "psf_overlap": 1, "tail_overlap": 1}), ("psf+tail", {"psf_overlap": 1, "tail_overlap": 1})):
        with mvs.Context(0) as c:
            for k, v in opts.items():
                c.set_option(k, v)
            d_gt = _dev_volume(c, gt)
            d_acq = c.dev_alloc(gt.nbytes)
            p = c.view_params(degrees=35, inc=1, snr=25.0, seed=SEED, stream=1, conv_method=1)
            for _ in range(4):
                c.simulate_view_dev(d_gt, (n, n, n), psf.copy(), p, d_acq)
            outs[name] = c.download(d_acq, (n, n, n))
            c.dev_free(d_gt)
            c.dev_free(d_acq)
    for k, v in outs.items():
        assert np.array_equal(v, outs["plain"]), k


@pytest.mark.parametrize("tool,kwargs", [
    ("fuzz_strided_zpass", dict(n_cases=50, seed=11)),            # k_zconv_strided forced wherever its geometry allows, any plane size
    ("fuzz_strided_zpass", dict(n_cases=25, seed=12, EXP=3)),     # ... with the z pass's tiles in plain grid order as well
    ("fuzz_fused_rotate", dict(count=30, seed=2025)),             # fused rotate + attenuate + x transform against the separate kernels, bit for bit
    ("fuzz_stencil", dict(count=30, seed=100, oracle_limit=4e8)), # direct stencil against the oracle's exact sum (small cases) / the FFT passes
])
def test_seeded_fuzzers(tool, kwargs):
    """The three random-geometry stress tools of tools/ as seeded test cases (they used to be one-off runs: 1 900 cases in round 4): each
    returns its number of failing cases."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        mod = importlib.import_module(tool)
        assert mod.run(verbose=False, **kwargs) == 0
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))

