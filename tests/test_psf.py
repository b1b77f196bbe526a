"""The PSF extraction on the GPU against the restatement of tests/psf_reference.py, bit for bit (NaNs compared as NaNs), through the C
ABI: the PSF, the record, the status bytes and the stages' own outputs over every chunk edge, PSF and image size, source type, stride,
matrix (from the host and from device memory) and parameter -- and the loop closed on the device: rendered views detected, registered,
their PSFs extracted in one frame and handed to the deconvolution.  Guard bytes behind every output stay intact and no input is
written."""
import numpy as np
import pytest

from . import dog_reference as D
from . import fuse_reference as FR
from . import psf_reference as R
from . import register_reference as REG
from .test_psf_host import matrices, same_record, singular_matrices
from .test_register import Arena, as_list
from .test_register_host import LOOP_BEADS, LOOP_INTERVAL, loop_cloud

pytestmark = pytest.mark.gpu
F64 = np.float64
BIG = (40, 33, 17)                                          # x, y, z


def volume(dim_xyz, seed=0, u16=False):
    rng = np.random.default_rng(seed + 17 * dim_xyz[0])
    v = rng.uniform(0, 60000, dim_xyz[::-1]) if u16 else rng.uniform(-3, 900, dim_xyz[::-1])
    return v.astype(np.uint16 if u16 else np.float32)


def beads(dim, kdim, n, seed=0):
    """n positions: two thirds where the whole window is inside (where there is such a place), the rest anywhere around the box."""
    rng = np.random.default_rng(seed)
    half = np.array([k // 2 for k in kdim], F64)
    lo, hi = half, np.array(dim, F64) - 1 - half
    pos = rng.uniform(-2, np.array(dim, F64) + 1, (n, 3))
    if np.all(lo <= hi):
        inside = lo + rng.uniform(0, 1, (n, 3)) * (hi - lo)
        pick = rng.uniform(size=n) < 0.67
        pos[pick] = inside[pick]
    return pos


def taps_of(kdim):
    return int(kdim[0]) * int(kdim[1]) * int(kdim[2])


def run(ctx, mvs, img, pos, m=None, use=None, kdim=(3, 3, 3), sep=(0, 0, 0), subtract_min=1, normalize=1, stride=24, m_dev=False, count=None,
        spare=0, want_status=True, stages=False):
    """mvsim_extract_psf_dev (or, with ``stages``, the three stage calls one after the other): (psf, record, status bytes or None, totals or
    None).  ``count``: the value of *n_dev (default: the length of the list); the capacity is the list's length + spare."""
    pos = np.asarray(pos, F64).reshape(-1, 3)
    u16 = img.dtype == np.uint16
    p = mvs.psf_params(kdim=kdim, min_separation=sep, subtract_min=subtract_min, normalize=normalize,
                       src_type=mvs._lib.MVSIM_SRC_U16 if u16 else mvs._lib.MVSIM_SRC_F32)
    cap, taps = max(1, len(pos) + spare), taps_of(kdim)
    n_dev = len(pos) if count is None else count
    n = min(max(n_dev, 0), cap)
    singular = R.invert(m) is None
    with Arena(ctx) as A:
        src = A.put(img)
        lst = A.put(as_list(np.vstack([pos, np.full((cap - len(pos), 3), 1e9)]), stride))      # spare entries: far outside
        cnt = A.put(np.array([n_dev], np.int64))
        use_d = A.put(np.asarray(use, np.uint8)) if use is not None else 0
        md = A.put(np.asarray(m, F64).reshape(12)) if m_dev else 0
        mh = None if m_dev else m
        out, rec, st, tot = A.out(4 * taps), A.out(72), A.out(cap), A.out(8 * taps)
        dim = img.shape[::-1]
        if stages:
            ctx.psf_select_dev(lst, stride, cnt, cap, dim, st, rec, use_d, mh, md, p)
            ctx.psf_gather_dev(src, dim, lst, stride, cnt, cap, st, tot, mh, md, p)
            ctx.psf_finish_dev(tot, out, rec, p)
        else:
            ctx.extract_psf_dev(src, dim, lst, stride, cnt, cap, out, rec, st if want_status else 0, use_d, mh, md, p)
        got = (A.get(out, 4 * taps, 4 * taps).view(np.float32).reshape(kdim[::-1]), A.get(rec, 72, 72).view(R.RESULT_DTYPE)[0],
               A.get(st, cap, n if want_status and not singular else 0) if want_status else None,
               A.get(tot, 8 * taps, 8 * taps if stages else 0).view(F64).reshape(kdim[::-1] if stages else (0,)))
        A.check_inputs()
    return got


def check(ctx, mvs, img, pos, m=None, use=None, kdim=(3, 3, 3), sep=(0, 0, 0), subtract_min=1, normalize=1, count=None, spare=0, **kw):
    """The whole call against the restatement; returns the restatement's (psf, record, status, totals)."""
    pos = np.asarray(pos, F64).reshape(-1, 3)
    n = len(pos) if count is None else min(max(count, 0), len(pos) + spare)
    listed = np.vstack([pos, np.full((max(0, n - len(pos)), 3), 1e9)])[:n]
    want = R.extract(img, listed, m, None if use is None else np.asarray(use)[:n], kdim, sep, subtract_min, normalize)
    got = run(ctx, mvs, img, pos, m, use, kdim, sep, subtract_min, normalize, count=count, spare=spare, **kw)
    assert R.same_bits(got[0], want[0]), "PSF"
    assert same_record(got[1], want[1]), (got[1], want[1])
    if got[2] is not None and want[2] is not None:
        assert np.array_equal(got[2], want[2]), "status bytes"
    if got[3].size:
        assert R.same_bits(got[3], want[3]), "totals"
    return want


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------------
def test_one_voxel(ctx, mvs):
    """kdim 1 x 1 x 1 on a 1 x 1 x 1 image with the bead at the origin."""
    for u16 in (False, True):
        img = np.full((1, 1, 1), 7, np.uint16 if u16 else np.float32)
        psf, rec, st, _ = check(ctx, mvs, img, [[0.0, 0.0, 0.0]], kdim=(1, 1, 1), subtract_min=0, normalize=0)
        assert psf[0, 0, 0] == 7.0 and rec["n_used"] == 1 and list(st) == [0]
        psf, rec, _, _ = check(ctx, mvs, img, [[0.0, 0.0, 0.0]], kdim=(1, 1, 1), stages=True)
        assert rec["flags"] == R.FLAT and psf[0, 0, 0] == 0.0


@pytest.mark.parametrize("u16", [False, True], ids=["float", "uint16"])
@pytest.mark.parametrize("kdim", [(3, 1, 5), (7, 7, 7), (15, 15, 15), (63, 3, 1)])
def test_psf_and_image_sizes(ctx, mvs, kdim, u16):
    used = 0
    for dim in ((5, 4, 3), BIG, (70, 9, 6)):
        img = volume(dim, u16=u16)
        for stages in (False, True):
            want = check(ctx, mvs, img, beads(dim, kdim, 12, seed=kdim[0]), kdim=kdim, stages=stages)
            used += int(want[1]["n_used"])
    assert used > 0


def test_identity_returns_the_window(ctx, mvs):
    img = volume(BIG, seed=1)
    for m in (None, FR.identity()):
        psf, rec, _, tot = run(ctx, mvs, img, [[20.0, 11.0, 8.0]], m, kdim=(5, 3, 7), subtract_min=0, normalize=0, stages=True)
        assert R.same_bits(psf, img[5:12, 10:13, 18:23]) and R.same_bits(tot, img[5:12, 10:13, 18:23].astype(F64)) and rec["n_used"] == 1


# ---- the list -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 513])
def test_bead_counts_at_the_chunk_edges(ctx, mvs, n):
    img = volume(BIG, seed=2)
    pos = beads(BIG, (3, 1, 5), n, seed=n)
    want = check(ctx, mvs, img, pos, kdim=(3, 1, 5), sep=(1.5, 1.5, 1.5), stages=True)
    check(ctx, mvs, img, pos, kdim=(3, 1, 5), sep=(1.5, 1.5, 1.5))
    if n == 0:
        assert want[1]["flags"] == R.NO_BEADS and not want[0].any()
    if n >= 255:
        assert want[1]["n_used"] > 30 and want[1]["n_crowded"] > 0 and want[1]["n_outside"] > 0


def test_masks(ctx, mvs):
    img = volume(BIG, seed=3)
    pos = beads(BIG, (3, 3, 3), 300, seed=3)
    use = (np.random.default_rng(3).uniform(size=300) > 0.4).astype(np.uint8)
    use[5] = 200                                            # any non-zero byte is "use"
    want = check(ctx, mvs, img, pos, use=use, sep=(1, 1, 1))
    assert want[1]["n_masked"] > 50 and want[1]["n_used"] > 50
    want = check(ctx, mvs, img, pos, use=np.zeros(300, np.uint8), sep=(2, 2, 2))
    assert want[1]["flags"] == R.NO_BEADS and want[1]["n_masked"] + want[1]["n_nonfinite"] == 300 and not want[0].any()


def test_corners_on_the_faces(ctx, mvs):
    """A corner tap exactly on 0 and on N - 1 is inside; one ulp beyond is OUTSIDE (dim y = 31: 29 + 1 stays in N - 1's binade)."""
    img = volume((40, 31, 17), seed=4)
    pos = np.array([[2.0, 1.0, 3.0], [37.0, 29.0, 13.0], [np.nextafter(2.0, 0), 1, 3], [2, 1, np.nextafter(3.0, 0)], [np.nextafter(37.0, 99), 29, 13],
                    [37, np.nextafter(29.0, 99), 13], [20.25, 15.5, 8.75]])
    for m in (None, FR.identity()):
        want = check(ctx, mvs, img, pos, m, kdim=(5, 3, 7))
        assert list(want[2]) == [0, 0, 3, 3, 3, 3, 0]


def test_non_finite_points_and_duplicates(ctx, mvs):
    img = volume(BIG, seed=5)
    pos = beads(BIG, (3, 3, 3), 70, seed=5)
    pos[3], pos[17, 1], pos[40, 2] = np.nan, np.inf, -np.inf
    pos[50] = pos[51] = (20.5, 16.25, 8.0)
    pos[60], pos[61] = (10.0, 10.0, 8.0), (14.0, 10.0, 8.0)    # exactly min_separation apart: not crowded by each other
    want = check(ctx, mvs, img, pos, sep=(4.0, 4.0, 4.0), stages=True)
    assert want[1]["n_nonfinite"] == 3 and want[2][50] == want[2][51] == R.CROWDED


@pytest.mark.parametrize("stride", [24, 40])
def test_strides(ctx, mvs, stride):
    img = volume(BIG, seed=6)
    pos = beads(BIG, (3, 5, 3), 40, seed=6)
    a = check(ctx, mvs, img, pos, kdim=(3, 5, 3), sep=(3, 3, 3), stride=stride)
    b = check(ctx, mvs, img, pos, kdim=(3, 5, 3), sep=(3, 3, 3), stride=stride, stages=True)
    assert R.same_bits(a[0], b[0]) and a[1]["n_used"] > 5


def test_count_above_the_capacity_and_negative(ctx, mvs):
    img = volume(BIG, seed=7)
    pos = beads(BIG, (3, 3, 3), 30, seed=7)
    full = check(ctx, mvs, img, pos, count=1000)            # clipped to the capacity
    assert full[1]["n_listed"] == 30
    assert check(ctx, mvs, img, pos, count=-5)[1]["flags"] == R.NO_BEADS
    part = check(ctx, mvs, img, pos, count=12, spare=7, stages=True)
    assert part[1]["n_listed"] == 12
    check(ctx, mvs, img, pos, count=35, spare=7)            # the spare entries are listed too: far outside


# ---- matrices -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k in matrices() if k != "none"])
def test_matrices_from_the_host_and_from_device_memory(ctx, mvs, name):
    m = matrices()[name]
    img = volume(BIG, seed=8)
    pos = beads(BIG, (5, 5, 3), 60, seed=8)
    host = check(ctx, mvs, img, pos, m, kdim=(5, 5, 3), sep=(2, 2, 2), stages=True)
    for stages in (False, True):
        dev = run(ctx, mvs, img, pos, m, kdim=(5, 5, 3), sep=(2, 2, 2), m_dev=True, stages=stages)
        assert R.same_bits(dev[0], host[0]) and same_record(dev[1], host[1]) and np.array_equal(dev[2], host[2])
    assert host[1]["n_used"] > 5
    shifted = np.array(m, F64)
    shifted[:, 3] = np.nan                                  # only the linear part is used
    assert R.same_bits(run(ctx, mvs, img, pos, shifted, kdim=(5, 5, 3), sep=(2, 2, 2))[0], host[0])


@pytest.mark.parametrize("name", list(singular_matrices()))
def test_singular_matrices(ctx, mvs, name):
    m = singular_matrices()[name]
    img = volume(BIG, seed=9)
    pos = beads(BIG, (3, 3, 3), 20, seed=9)
    for kw in ({}, {"m_dev": True}, {"stages": True}, {"stages": True, "m_dev": True}, {"want_status": False}):
        psf, rec, st, tot = run(ctx, mvs, img, pos, m, **kw)
        want = R.extract(img, pos, m, None, (3, 3, 3), (0, 0, 0))
        assert R.same_bits(psf, want[0]) and same_record(rec, want[1]) and rec["flags"] == R.SINGULAR and rec["n_listed"] == 20
        assert not psf.any() and not np.signbit(psf).any() and (st is None or len(st) == 0)
        if tot.size:
            assert R.same_bits(tot, want[3])


# ---- voxels and parameters ------------------------------------------------------------------------------------------------------------------
def test_non_finite_voxels_inside_a_window(ctx, mvs):
    img = volume(BIG, seed=10)
    pos = np.array([[10.25, 10.5, 8.0], [25.0, 20.0, 8.5], [30.5, 9.0, 7.0]])
    for value, at in ((np.nan, (8, 10, 10)), (np.inf, (8, 20, 25)), (-np.inf, (7, 9, 30))):
        bad = img.copy()
        bad[at] = value
        for sub in (1, 0):
            want = check(ctx, mvs, bad, pos, kdim=(5, 5, 5), subtract_min=sub, stages=True)
            assert not np.isfinite(want[0]).all() and want[1]["flags"] == R.FLAT
    both = img.copy()
    both[8, 10, 10], both[8, 20, 25] = np.inf, -np.inf
    assert np.isnan(check(ctx, mvs, both, pos, kdim=(5, 5, 5))[0]).any()


def test_constant_image_is_flat(ctx, mvs):
    img = np.full(BIG[::-1], 12.5, np.float32)
    want = check(ctx, mvs, img, beads(BIG, (3, 3, 3), 20, seed=11))
    assert want[1]["flags"] == R.FLAT and not want[0].any() and want[1]["minimum"] == 12.5 and want[1]["sum"] == 0.0
    want = check(ctx, mvs, img, beads(BIG, (3, 3, 3), 20, seed=11), subtract_min=0)
    assert want[1]["flags"] == 0 and np.all(want[0] == np.float32(1.0 / 27.0))


@pytest.mark.parametrize("subtract_min,normalize", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_subtract_min_and_normalize(ctx, mvs, subtract_min, normalize):
    img = volume(BIG, seed=12)
    pos = beads(BIG, (5, 3, 7), 300, seed=12)
    want = check(ctx, mvs, img, pos, kdim=(5, 3, 7), subtract_min=subtract_min, normalize=normalize, stages=True)
    check(ctx, mvs, img, pos, kdim=(5, 3, 7), subtract_min=subtract_min, normalize=normalize, want_status=False)
    assert want[1]["n_used"] > 100 and want[1]["flags"] == 0
    if normalize:
        assert abs(float(want[0].astype(F64).sum()) - 1.0) < 1e-5


# ---- the use-mask from a registration's candidates --------------------------------------------------------------------------------------------
def test_use_from_matches(ctx, mvs):
    rng = np.random.default_rng(13)
    cand = np.zeros(300, REG.MATCH_DTYPE)
    cand["a"], cand["b"] = rng.integers(-3, 70, 300), rng.integers(-3, 70, 300)
    cand["a"][7], cand["b"][9] = 2 ** 31 - 1, -2 ** 31
    mask = rng.integers(0, 3, 300).astype(np.uint8)          # 2 is not "inlier"
    for n_cand, cap, use_mask, side, n_points in ((300, 300, True, 0, 64), (300, 300, True, 1, 64), (300, 300, False, 0, 64), (1000, 257, True, 1, 31),
                                                  (-4, 300, False, 0, 64), (100, 300, True, 1, 1)):
        with Arena(ctx) as A:
            c, cnt, mk = A.put(cand), A.put(np.array([n_cand], np.int64)), A.put(mask)
            use = A.out(n_points)
            ctx.psf_use_from_matches_dev(c, cnt, cap, mk if use_mask else 0, side, n_points, use)
            got = A.get(use, n_points, n_points)
            A.check_inputs()
        pairs = list(zip(cand["a"].tolist(), cand["b"].tolist()))
        assert np.array_equal(got, R.use_from_matches(pairs, n_cand, cap, mask if use_mask else None, side, n_points)), (n_cand, cap, side)


# ---- the host entry, repeatability ------------------------------------------------------------------------------------------------------------
def test_host_entry_equals_the_device_entry(ctx, mvs):
    img = volume(BIG, seed=14)
    pos = beads(BIG, (5, 5, 3), 300, seed=14)
    use = (np.random.default_rng(14).uniform(size=300) > 0.3).astype(np.uint8)
    m = matrices()["rot_z"]
    p = mvs.psf_params(kdim=(5, 5, 3), min_separation=2.0)
    dev = run(ctx, mvs, img, pos, m, use, kdim=(5, 5, 3), sep=(2, 2, 2))
    psf, rec, st = ctx.extract_psf(img, pos, m, use, p, status=True)
    assert R.same_bits(psf, dev[0]) and same_record(rec, dev[1]) and np.array_equal(st, dev[2])
    want = R.extract(img, pos, m, use, (5, 5, 3), (2.0, 2.0, 2.0))
    assert R.same_bits(psf, want[0]) and same_record(rec, want[1]) and rec["n_used"] > 20
    psf2, rec2 = mvs.PsfExtraction(ctx=ctx, kdim=(5, 5, 3), min_separation=2.0).extract(img, as_list(pos, 40), m, use)
    assert R.same_bits(psf2, psf) and same_record(rec2, rec)
    u16 = np.abs(img).astype(np.uint16)
    got, _ = ctx.extract_psf(u16, pos, None, None, mvs.psf_params(kdim=3, min_separation=0, src_type=mvs._lib.MVSIM_SRC_U16))
    assert R.same_bits(got, R.extract(u16, pos, None, None, (3, 3, 3), (0, 0, 0))[0])
    empty, rec0 = ctx.extract_psf(img, np.zeros((0, 3)), None, None, p)
    assert rec0["flags"] == R.NO_BEADS and not empty.any()
    with pytest.raises(ValueError, match="overlaps"):
        with Arena(ctx) as A:
            src = A.put(img)
            ctx.extract_psf_dev(src, BIG, src, 24, src, 8, src + 4 * img.size - 4, src, params=p)


def test_second_call_and_call_after_release_caches(ctx, mvs):
    img = volume(BIG, seed=15)
    pos = beads(BIG, (7, 7, 7), 300, seed=15)
    first = run(ctx, mvs, img, pos, matrices()["shear"], kdim=(7, 7, 7), sep=(1, 1, 1))
    again = run(ctx, mvs, img, pos, matrices()["shear"], kdim=(7, 7, 7), sep=(1, 1, 1))
    assert R.same_bits(first[0], again[0]) and same_record(first[1], again[1])
    ctx.release_caches()
    after = run(ctx, mvs, img, pos, matrices()["shear"], kdim=(7, 7, 7), sep=(1, 1, 1), want_status=False)
    assert R.same_bits(first[0], after[0]) and same_record(first[1], after[1])


# ---- accuracy -------------------------------------------------------------------------------------------------------------------------------
ACC_DIM, ACC_KDIM = (96, 96, 72), (15, 15, 21)
ACC_INTERVAL = ((0, 0, 0), ACC_DIM)


def rendered(ctx, mvs, pts, mats, register=False):
    """The views of a cloud rendered and detected on the device, view 1 registered against view 0 and each view's PSF extracted in view
    0's frame (the registration's matrix read from device memory), nothing downloaded in between; then everything downloaded once."""
    det = mvs.DifferenceOfGaussian(threshold=5.0, ctx=ctx, capacity=256)
    item, cap = D.PEAK_DTYPE.itemsize, det.capacity
    nv, taps = ACC_DIM[0] * ACC_DIM[1] * ACC_DIM[2], taps_of(ACC_KDIM)
    p = mvs.psf_params(kdim=ACC_KDIM)
    out = []
    with Arena(ctx) as A:
        img = [A.out(4 * nv) for _ in mats]
        pk = [A.out(cap * item + 8) for _ in mats]
        res = A.out(160)
        psf, rec, st = [A.out(4 * taps) for _ in mats], [A.out(72) for _ in mats], [A.out(cap) for _ in mats]
        for m, im, at in zip(mats, img, pk):
            ctx.render_beads_dev(pts, ACC_INTERVAL, D.BEAD_SIGMA, [im], None, matrices=np.asarray(m)[None])
            ctx.detect_beads_dev(im, np.float32, ACC_DIM, cap, at, at + cap * item, params=det.params)
        if register:
            ctx.register_beads_dev(pk[1], item, pk[1] + cap * item, cap, pk[0], item, pk[0] + cap * item, cap, res, params=mvs.match_params())
        for v in range(len(mats)):
            ctx.extract_psf_dev(img[v], ACC_DIM, pk[v], item, pk[v] + cap * item, cap, psf[v], rec[v], st[v],
                                m_dptr=res if register and v == 1 else 0, params=p)
        for v in range(len(mats)):
            n = int(ctx.download(pk[v] + cap * item, (1,), np.int64)[0])
            out.append({"img": A.get(img[v], 4 * nv, 4 * nv).view(np.float32).reshape(ACC_DIM[::-1]), "peaks": ctx.download(pk[v], (n,), D.PEAK_DTYPE),
                        "psf": A.get(psf[v], 4 * taps, 4 * taps).view(np.float32).reshape(ACC_KDIM[::-1]),
                        "rec": A.get(rec[v], 72, 72).view(R.RESULT_DTYPE)[0], "status": A.get(st[v], cap, n)})
        reg = A.get(res, 160, 160).view(REG.REGISTRATION_DTYPE)[0] if register else None
    return out, reg


def test_psf_from_detected_beads_is_as_accurate_as_from_the_true_positions(ctx, mvs):
    """Gaussian beads of sigma (1, 1, 3) on a grid of pitch 22 with random sub-voxel offsets, every 15 x 15 x 21 window inside.  r_ref is
    the restatement at the TRUE positions against the analytic Gaussian -- the price of trilinear sampling alone --; the device's PSF
    from the DETECTED positions must stay within 2 r_ref.  Measured on the MI355X: r_ref 0.00639, detected 0.00632."""
    rng = np.random.default_rng(5)
    pts = np.array([[x, y, z] for z in (12, 34, 56) for y in (8, 30, 52, 74) for x in (8, 30, 52, 74)], F64) + rng.uniform(0, 1, (48, 3))
    sb = mvs.SimulateBeads([0], 0, len(pts), ((0, 0, 0), (95, 95, 71)), ACC_INTERVAL, D.BEAD_SIGMA)
    sb.points = pts
    assert np.array_equal(sb.matrices()[0], FR.identity())
    (view,), _ = rendered(ctx, mvs, pts, [sb.matrices()[0]])
    assert view["rec"]["n_used"] == len(pts) == len(view["peaks"]) and not view["status"].any() and view["rec"]["flags"] == 0
    analytic = R.gaussian(D.BEAD_SIGMA, ACC_KDIM)
    r_ref = R.rms_range(R.extract(view["img"], pts, None, None, ACC_KDIM)[0], analytic)
    got = R.rms_range(view["psf"], analytic)
    print(f"identity: r_ref {r_ref:.5f}, detected {got:.5f}")
    assert 0 < r_ref < 0.02 and got <= 2 * r_ref
    want = R.extract(view["img"], view["peaks"]["pos"], None, None, ACC_KDIM)
    assert R.same_bits(view["psf"], want[0]) and same_record(view["rec"], want[1])
    # the simulator's own entry point does the same chain
    psf, rec, ana = sb.extract_psf(0, detector=mvs.DifferenceOfGaussian(threshold=5.0, ctx=ctx, capacity=256), params=mvs.psf_params(kdim=ACC_KDIM))
    assert R.same_bits(psf, view["psf"]) and same_record(rec, view["rec"]) and np.allclose(ana, analytic, rtol=1e-12, atol=0)


def test_psf_of_a_rotated_view_in_the_reference_frame(ctx, mvs):
    """View B is the cloud under 45 degrees about x; its PSF is extracted in view A's frame through the REGISTERED matrix B -> A, read
    from device memory.  r_ref: the restatement at the true positions with the true matrix.  The two-step alternative -- extract in
    B's own frame, then transform_psf -- is printed for comparison.  Measured on the MI355X: r_ref 0.00660, registered 0.00656,
    two steps 0.00835."""
    rng = np.random.default_rng(5)
    mats = [FR.identity(), np.asarray(mvs.SimulateMultiViewDataset.axisRotation(ACC_DIM, 0, 45), F64).reshape(3, 4)]
    grid = np.array([[x, 48 + a, 36 + b] for a, b in ((0, 0), (-22, 0), (25, 0), (0, -23), (0, 22)) for x in (9, 31, 56, 85)], F64)
    in_b = grid + rng.uniform(0, 1, grid.shape)             # hand-placed in B's image; irregular pitches >= 22 keep the descriptors apart
    back = np.linalg.inv(np.vstack([mats[1], [0, 0, 0, 1]]))
    pts = in_b @ back[:3, :3].T + back[:3, 3]
    true = mvs.registration.true_transform(mats[1], mats[0], (0, 0, 0))
    views, reg = rendered(ctx, mvs, pts, mats, register=True)
    b = views[1]
    assert reg["flags"] == 0 and reg["n_inliers"] >= 12
    assert b["rec"]["n_used"] == len(pts) == len(b["peaks"]) and not b["status"].any() and b["rec"]["flags"] == 0
    analytic = R.gaussian(D.BEAD_SIGMA, ACC_KDIM, true)
    r_ref = R.rms_range(R.extract(b["img"], in_b, true, None, ACC_KDIM)[0], analytic)
    got = R.rms_range(b["psf"], analytic)
    own = R.extract(b["img"], b["peaks"]["pos"], None, None, ACC_KDIM)[0]
    two = R.rms_range(mvs.transform_psf(own, reg["m"], ctx=ctx), analytic)
    print(f"rotated: r_ref {r_ref:.5f}, registered {got:.5f}, two steps (extract, then transform_psf) {two:.5f}")
    assert 0 < r_ref < 0.02 and got <= 2 * r_ref
    want = R.extract(b["img"], b["peaks"]["pos"], reg["m"], None, ACC_KDIM)
    assert R.same_bits(b["psf"], want[0]) and same_record(b["rec"], want[1])


# ---- the closed loop ------------------------------------------------------------------------------------------------------------------------
LOOP_DIM = (128, 128, 96)


def test_extracted_psfs_feed_the_deconvolution(ctx, mvs):
    """The 40-bead cloud under the identity (A) and under 45 degrees about x (B): detect, register A -> B, the inliers as A's use-mask, both
    PSFs extracted in B's frame, the views aligned into B's frame with their weights, the weights normalised -- one stream, nothing
    downloaded in between.  The deconvolution takes its PSFs from the host, so they are fetched there; two iterations on the device must
    be finite and equal Context.deconvolve on the downloaded aligned arrays with the downloaded PSFs bit for bit."""
    pts, mats = loop_cloud(mvs)
    det = mvs.DifferenceOfGaussian(threshold=5.0, ctx=ctx, capacity=256)
    item, cap, nv = D.PEAK_DTYPE.itemsize, det.capacity, LOOP_DIM[0] * LOOP_DIM[1] * LOOP_DIM[2]
    kdim = (9, 9, 13)
    taps = taps_of(kdim)
    p = mvs.psf_params(kdim=kdim, min_separation=(9, 9, 13))
    crop_min, crop_dim, n = (40, 40, 24), (48, 48, 48), 48 ** 3
    params = mvs.decon_params(iterations=2)
    with Arena(ctx) as A:
        img = [A.out(4 * nv), A.out(4 * nv)]
        pk = [A.out(cap * item + 8), A.out(cap * item + 8)]
        res, cand, mask, use = A.out(160), A.out(24 * cap), A.out(cap), A.out(cap)
        psf, rec = [A.out(4 * taps), A.out(4 * taps)], [A.out(72), A.out(72)]
        al, wt, psi = [A.out(4 * n), A.out(4 * n)], [A.out(4 * n), A.out(4 * n)], A.out(4 * n)
        for m, im, at in zip(mats, img, pk):
            ctx.render_beads_dev(pts, LOOP_INTERVAL, D.BEAD_SIGMA, [im], None, matrices=np.asarray(m)[None])
            ctx.detect_beads_dev(im, np.float32, LOOP_DIM, cap, at, at + cap * item, params=det.params)
        ctx.register_beads_dev(pk[0], item, pk[0] + cap * item, cap, pk[1], item, pk[1] + cap * item, cap, res, cand, mask, params=mvs.match_params())
        ctx.psf_use_from_matches_dev(cand, res + 120, cap, mask, 0, cap, use)         # n_candidates of the record, read on the device
        ctx.extract_psf_dev(img[0], LOOP_DIM, pk[0], item, pk[0] + cap * item, cap, psf[0], rec[0], use_dptr=use, m_dptr=res, params=p)
        ctx.extract_psf_dev(img[1], LOOP_DIM, pk[1], item, pk[1] + cap * item, cap, psf[1], rec[1], params=p)
        ctx.align_views_dev(img, [LOOP_DIM] * 2, [None, FR.identity()], crop_min, crop_dim, al, wt, params=mvs.fuse_params(blend=6.0),
                            matrix_dptrs=[res, 0])
        ctx.normalize_weights_dev(wt, n, 1.0)
        psfs = [A.get(q, 4 * taps, 4 * taps).view(np.float32).reshape(kdim[::-1]) for q in psf]
        ctx.deconvolve_dev(al, crop_dim, psfs, psi, weight_dptrs=wt, params=params)
        got = A.get(psi, 4 * n, 4 * n).view(np.float32).reshape(48, 48, 48)
        got_al = [A.get(a, 4 * n, 4 * n).view(np.float32).reshape(48, 48, 48) for a in al]
        got_wt = [A.get(w, 4 * n, 4 * n).view(np.float32).reshape(48, 48, 48) for w in wt]
        recs = [A.get(r, 72, 72).view(R.RESULT_DTYPE)[0] for r in rec]
        reg = A.get(res, 160, 160).view(REG.REGISTRATION_DTYPE)[0]
        imgs = [A.get(im, 4 * nv, 4 * nv).view(np.float32).reshape(LOOP_DIM[::-1]) for im in img]
        found = [int(ctx.download(at + cap * item, (1,), np.int64)[0]) for at in pk]
        peaks = [ctx.download(at, (k,), D.PEAK_DTYPE) for at, k in zip(pk, found)]
        cands = A.get(cand, 24 * cap, 24 * min(int(reg["n_candidates"]), cap)).view(REG.MATCH_DTYPE)
        masks = A.get(mask, cap, len(cands))
        uses = A.get(use, cap, cap)
    assert reg["flags"] == 0 and found == [LOOP_BEADS, LOOP_BEADS]
    want_use = R.use_from_matches(list(zip(cands["a"].tolist(), cands["b"].tolist())), reg["n_candidates"], cap, masks, 0, cap)
    assert np.array_equal(uses, want_use) and uses.sum() == reg["n_inliers"]
    for v, (m, u) in enumerate(((reg["m"], want_use[:found[0]]), (None, None))):
        want = R.extract(imgs[v], peaks[v]["pos"], m, u, kdim, (9.0, 9.0, 13.0))
        assert R.same_bits(psfs[v], want[0]) and same_record(recs[v], want[1]) and recs[v]["flags"] == 0 and recs[v]["n_used"] >= 12, v
        assert abs(float(psfs[v].astype(F64).sum()) - 1.0) < 1e-5
    assert np.isfinite(got).all() and got.max() > 0
    assert R.same_bits(got, ctx.deconvolve(got_al, psfs, got_wt, params))
