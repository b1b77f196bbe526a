"""The bead detector on the GPU against the restatement of tests/dog_reference.py, bit for bit (NaNs compared as NaNs): the DoG volume
over every tile edge, alignment and source type, the peak list and its order, the sub-voxel fit with its flags, the whole call,
and the loop closed on the device -- rendered beads found where the simulator put them."""
import math

import numpy as np
import pytest

from . import dog_reference as R

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = -7


# ---- device helpers ---------------------------------------------------------------------------------------------------------------------
def run_dog(ctx, img, params, src_off=0, dst_off=0):
    """D of a host image through mvsim_dog_dev with both pointers offset by whole elements; checks that the source is not written
    and that nothing is written outside the destination."""
    a = np.ascontiguousarray(img)
    n, item = a.size, a.itemsize
    src, dst = ctx.dev_alloc((n + 2) * item), ctx.dev_alloc((n + 2) * 4)
    try:
        ctx.upload(src + src_off * item, a)
        ctx.upload(dst, np.full(n + 2, GUARD, F32))
        ctx.dog_dev(src + src_off * item, a.dtype, a.shape[::-1], dst + dst_off * 4, params)
        out = ctx.download(dst, (n + 2,), F32)
        back = ctx.download(src + src_off * item, a.shape, a.dtype)
    finally:
        ctx.dev_free(src)
        ctx.dev_free(dst)
    assert R.same_bits(back, a), "the source was written"
    outside = np.delete(out, np.s_[dst_off:dst_off + n])
    assert np.all(outside == GUARD), "written outside the destination"
    return out[dst_off:dst_off + n].reshape(a.shape)


class DevVolume:
    """A float volume on the device for the peak and localisation operators."""

    def __init__(self, ctx, D):
        self.ctx, self.D = ctx, np.ascontiguousarray(D, dtype=F32)
        self.dim = self.D.shape[::-1]
        self.ptr = ctx.dev_alloc(self.D.nbytes)
        ctx.upload(self.ptr, self.D)

    def close(self):
        self.ctx.dev_free(self.ptr)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def find(self, threshold, capacity):
        """(the list with one guard element behind it, n_found)"""
        ctx = self.ctx
        lst = ctx.dev_alloc(8 * (capacity + 1) + 8)
        try:
            ctx.upload(lst, np.full(capacity + 2, GUARD, np.int64))
            ctx.find_peaks_dev(self.ptr, self.dim, threshold, capacity, lst, lst + 8 * (capacity + 1))
            got = ctx.download(lst, (capacity + 2,), np.int64)
        finally:
            ctx.dev_free(lst)
        return got[:capacity + 1], int(got[capacity + 1])

    def localise(self, voxels, n_found, capacity, max_moves):
        """the records with one guard record behind them"""
        ctx = self.ctx
        item = R.PEAK_DTYPE.itemsize
        buf = ctx.dev_alloc(8 * (capacity + 1) + item * (capacity + 1))
        try:
            v = np.full(capacity + 1, GUARD, np.int64)
            v[:len(voxels)] = voxels
            v[capacity] = n_found
            ctx.upload(buf, v)
            pk = buf + 8 * (capacity + 1)
            ctx.upload(pk, np.full(item * (capacity + 1), 0xAB, np.uint8))
            ctx.localise_peaks_dev(self.ptr, self.dim, buf, buf + 8 * capacity, capacity, max_moves, pk)
            raw = ctx.download(pk, (item * (capacity + 1),), np.uint8)
        finally:
            ctx.dev_free(buf)
        assert np.all(raw[item * min(n_found, capacity):] == 0xAB), "records past min(n_found, capacity) were written"
        return raw[:item * min(n_found, capacity)].view(R.PEAK_DTYPE)


def check_peaks(ctx, D, threshold, capacity=None, max_moves=4, localise_at_most=400):
    """The list and the count against the restatement, then the fit of (at most localise_at_most of) the listed peaks."""
    want = R.find_peaks(D, threshold)
    cap = max(1, len(want)) if capacity is None else capacity
    with DevVolume(ctx, D) as dv:
        got, n = dv.find(threshold, cap)
        assert n == len(want)
        listed = min(n, cap)
        assert np.array_equal(got[:listed], want[:listed])
        assert np.all(got[listed:] == GUARD), "entries past min(n_found, capacity) were written"
        lcap = max(1, min(listed, localise_at_most))
        pk = dv.localise(want[:lcap], n, lcap, max_moves)
    ref = R.localise(D, want[:min(n, lcap)], max_moves)
    assert R.same_bits(pk, ref)
    return want, pk


# ---- D bit for bit ------------------------------------------------------------------------------------------------------------------------
def _shapes(mvs):
    g = mvs.dog_geometry()
    tx, ty, tz = g["tile_x"], g["tile_y"], g["tile_z"]
    fixed = [(3, 3, 3), (2, 5, 4), (5, 4, 3), (33, 9, 7), (67, 35, 19), (130, 70, 20)]
    edges = [(tx - 1, ty - 1, tz - 1), (tx, ty, tz), (tx + 1, ty + 1, tz + 1), (2 * tx - 1, 5, 4), (2 * tx + 1, 2 * ty + 1, 6),
             (2 * tx + 4, 3, 2 * tz + 1), (8, 2 * ty - 1, 2 * tz - 1)]
    return fixed + edges


SIGMA_SETS = {
    "default": (R.DEFAULT_SIGMA1, R.DEFAULT_SIGMA2),
    "mixed": ((1.0, 2.5, 0.7), (1.4, 3.0, 1.1)),
    "wide": ((1.8, 1.8, 1.8), (10.3, 2.3, 10.3)),          # radius 31: the mirror folds more than once on most shapes
}
SHAPE_IDS = range(13)


def _random_float(shape_zyx, rng):
    v = (rng.random(shape_zyx) * 100).astype(F32)
    flat = v.reshape(-1)
    special = [0.0, -0.0, 1e-40, -3e-42, np.nan, np.inf, -np.inf]
    if flat.size >= 64:
        at = rng.choice(flat.size, len(special), replace=False)
        flat[at] = special
    else:
        flat[:3] = [0.0, 1e-40, -3e-42]
    return v


@pytest.fixture(scope="module")
def volumes(mvs):
    """Per shape: the float and uint16 sources, drawn once."""
    out = []
    for i, (nx, ny, nz) in enumerate(_shapes(mvs)):
        rng = np.random.default_rng(100 + i)
        out.append({"f32": _random_float((nz, ny, nx), rng),
                    "u16": rng.integers(0, 65536, (nz, ny, nx)).astype(np.uint16),
                    "clean": (rng.random((nz, ny, nx)) * 100).astype(F32)})
    assert len(out) == len(SHAPE_IDS)
    return out


@pytest.mark.parametrize("sig", list(SIGMA_SETS))
@pytest.mark.parametrize("si", SHAPE_IDS)
def test_dog_equals_the_restatement(ctx, mvs, volumes, si, sig):
    s1, s2 = SIGMA_SETS[sig]
    params = mvs.dog_params(sigma1=s1, sigma2=s2)
    t1, t2 = [mvs.dog_taps(s) for s in s1], [mvs.dog_taps(s) for s in s2]
    vol = volumes[si]
    for kind, offsets in (("f32", ((0, 0), (1, 0), (0, 1))), ("u16", ((0, 0), (1, 1)))):
        want = R.dog(vol[kind], t1, t2)
        for src_off, dst_off in offsets:
            got = run_dog(ctx, vol[kind], params, src_off, dst_off)
            assert R.same_bits(got, want), (kind, src_off, dst_off, vol[kind].shape)


@pytest.mark.parametrize("si", SHAPE_IDS)
def test_peaks_of_the_dog_volumes_equal_the_restatement(ctx, mvs, volumes, si):
    """List, count and fit over the D of NaN-free random data (dense in peaks: every block of the peaks kernel holds some) and of
    the data with planted NaN and infinities."""
    for kind in ("clean", "f32"):
        D = R.dog_sigmas(volumes[si][kind], taps_of=mvs.dog_taps)
        want, _ = check_peaks(ctx, D, 0.05)
        if kind == "clean" and si == 5:
            per = mvs.dog_geometry()["peak_block_voxels"]
            assert len(set((want // per).tolist())) >= 3, "the peaks do not span three blocks"
            check_peaks(ctx, D, 0.05, capacity=len(want) // 2)             # the first capacity entries, the full count
            check_peaks(ctx, D, 0.05, capacity=1)
            check_peaks(ctx, D, 1e30)                                      # no peaks at all
            check_peaks(ctx, D, -math.inf, capacity=7)


# ---- hand-made volumes ----------------------------------------------------------------------------------------------------------------------
def _base(shape=(9, 10, 11)):
    return np.zeros(shape, F32)


def test_peak_rule_on_hand_made_volumes(ctx):
    cases = []
    cases.append(("constant", np.full((6, 7, 8), 3, F32), 1.0, 0))
    for axis_step in ((0, 0, 1), (0, 1, 0), (1, 0, 0), (1, 1, 1), (1, -1, 1)):
        for run in (2, 3):
            v = _base()
            for k in range(run):
                v[4 + k * axis_step[0], 4 + k * axis_step[1], 4 + k * axis_step[2]] = 5
            cases.append((f"plateau {axis_step} x{run}", v, 1.0, 1))
    for face in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (8, 4, 4), (4, 9, 4), (4, 4, 10)):
        v = _base()
        v[face] = 5
        cases.append((f"face {face}", v, 1.0, 0))
    for dz, dy, dx in ((0, 0, 1), (-1, 1, 0), (1, 1, 1)):
        v = _base()
        v[4, 4, 4] = 5
        v[4 + dz, 4 + dy, 4 + dx] = np.nan
        cases.append((f"nan at {(dz, dy, dx)}", v, 1.0, 0))
    v = _base()
    v[4, 4, 4] = np.nan
    cases.append(("nan itself", v, -1.0, 0))
    v = _base()
    v[4, 4, 4] = 5
    cases.append(("threshold equals the peak", v, 5.0, 0))
    cases.append(("threshold just below", v, float(np.nextafter(F32(5), F32(0))), 1))
    v = _base()
    v[2, 2, 2], v[2, 2, 4], v[6, 7, 8] = 5, 5, np.inf
    cases.append(("three peaks, one infinite", v, 1.0, 3))
    cases.append(("extent below 3", np.full((2, 5, 5), 1, F32), 0.0, 0))
    for name, vol, thr, expect in cases:
        want, _ = check_peaks(ctx, vol, thr)
        assert len(want) == expect, name


def test_peaks_span_blocks_in_index_order(ctx, mvs):
    """Isolated spikes in four blocks of the peaks kernel, several per block, at both ends of a block's range."""
    per = mvs.dog_geometry()["peak_block_voxels"]
    nx, ny = 32, 16
    nz = 4 * per // (nx * ny) + 2
    v = np.zeros((nz, ny, nx), F32)
    rng = np.random.default_rng(5)
    for z in range(1, nz - 1, 2):
        for y in range(1, ny - 1, 3):
            for x in rng.choice(np.arange(1, nx - 1, 2), 4, replace=False):
                v[z, y, x] = 1 + rng.random()
    want, _ = check_peaks(ctx, v, 0.5)
    assert np.all(np.bincount(want // per, minlength=4)[:4] >= 8), "fewer than 8 peaks in one of the first four blocks"
    check_peaks(ctx, v, 0.5, capacity=len(want) - 1)
    check_peaks(ctx, v, 0.5, capacity=1)


# ---- localisation -----------------------------------------------------------------------------------------------------------------------------
def test_half_voxel_beads_are_frozen(ctx, mvs):
    shape = (48, 24, 24)
    for k in range(11):
        p = np.array([[12.3, 12.7, 24.0 + 0.496 + 0.001 * k]])
        D = R.dog_sigmas(R.render_beads(shape, p), taps_of=mvs.dog_taps)
        want, pk = check_peaks(ctx, D, 5.0)
        assert len(want) == 1 and pk["flags"][0] & R.FROZEN
        assert R.nearest(p, pk["pos"])[0] <= 0.5


def test_max_moves_caps_a_fit_that_wants_two_moves(ctx, mvs):
    shape = (40, 40, 40)
    p = np.array([[20.2, 19.9, 20.1]])
    D = R.dog_sigmas(R.render_beads(shape, p, sigma=(3.0, 3.0, 3.0)), (2.0,) * 3, (2.6,) * 3, taps_of=mvs.dog_taps)
    start = np.array([22 + 40 * (20 + 40 * 20)], np.int64)                  # two voxels off along x
    flags = {}
    with DevVolume(ctx, D) as dv:
        for mm in (0, 1, 2, 4):
            got = dv.localise(start, 1, 1, mm)
            assert R.same_bits(got, R.localise(D, start, mm)), mm
            flags[mm] = int(got["flags"][0])
            if mm >= 2:
                assert R.nearest(p, got["pos"])[0] < 0.1 and got["voxel"][0] == 20 + 40 * (20 + 40 * 20)
    assert flags[0] & R.CAPPED and flags[1] & R.CAPPED and not flags[2] & R.CAPPED and not flags[4] & R.CAPPED


def test_singular_refused_and_outside_fits(ctx):
    # constant along z: the determinant is exactly zero
    y, x = np.mgrid[0:12, 0:14]
    plane = (100 * np.exp(-((x - 6.3) ** 2 + (y - 5.6) ** 2) / 8.0)).astype(F32)
    D = np.repeat(plane[None], 8, axis=0)
    vox = np.array([6 + 14 * (6 + 12 * 3)], np.int64)
    with DevVolume(ctx, D) as dv:
        got = dv.localise(vox, 1, 1, 4)
    assert R.same_bits(got, R.localise(D, vox, 4))
    assert got["flags"][0] == R.SINGULAR and tuple(got["pos"][0]) == (6.0, 6.0, 3.0) and got["voxel"][0] == vox[0]
    # a maximum between the face x = 0 and the voxel x = 1: the fit wants to leave the interior, the move is refused
    z, y, x = np.mgrid[0:9, 0:9, 0:9]
    D = (100 * np.exp(-((x - 0.3) ** 2 + (y - 4.1) ** 2 + (z - 4.2) ** 2) / 6.0)).astype(F32)
    vox = np.array([1 + 9 * (4 + 9 * 4)], np.int64)
    with DevVolume(ctx, D) as dv:
        got = dv.localise(vox, 1, 1, 4)
    assert R.same_bits(got, R.localise(D, vox, 4))
    assert got["voxel"][0] == vox[0] and got["pos"][0][0] < 0.5 and got["flags"][0] == 0
    # listed voxels that are no interior voxels are reported, not read around
    vox = np.array([0, 9 * 9 * 9 - 1, 9 * 9 * 9 + 5, -3, 4 + 9 * (4 + 9 * 8)], np.int64)
    with DevVolume(ctx, D) as dv:
        got = dv.localise(vox, len(vox), len(vox), 4)
    assert R.same_bits(got, R.localise(D, vox, 4)) and np.all(got["flags"] == R.OUTSIDE)


# ---- the whole call ---------------------------------------------------------------------------------------------------------------------------
def _chain(ctx, img, params, capacity):
    """The three stage operators chained on the device: (peaks, n_found)."""
    a = np.ascontiguousarray(img)
    n = a.size
    item = R.PEAK_DTYPE.itemsize
    src, dog = ctx.dev_alloc(a.nbytes), ctx.dev_alloc(4 * n)
    lst, pk = ctx.dev_alloc(8 * capacity + 8), ctx.dev_alloc(item * capacity)
    try:
        ctx.upload(src, a)
        ctx.dog_dev(src, a.dtype, a.shape[::-1], dog, params)
        ctx.find_peaks_dev(dog, a.shape[::-1], params.threshold, capacity, lst, lst + 8 * capacity)
        ctx.localise_peaks_dev(dog, a.shape[::-1], lst, lst + 8 * capacity, capacity, params.max_moves, pk)
        nf = int(ctx.download(lst + 8 * capacity, (1,), np.int64)[0])
        peaks = ctx.download(pk, (min(nf, capacity),), R.PEAK_DTYPE)
    finally:
        for p in (src, dog, lst, pk):
            ctx.dev_free(p)
    return peaks, nf


@pytest.mark.parametrize("kind", ["f32", "u16"])
def test_whole_call_equals_the_chained_operators(ctx, mvs, kind):
    rng = np.random.default_rng(21)
    shape = (40, 36, 44)
    pts = R.draw_positions(shape, 9, rng)
    img = R.add_poisson(R.render_beads(shape, pts), rng)
    img = img.astype(np.uint16) if kind == "u16" else img
    params = mvs.dog_params(threshold=5.0)
    want, D = R.detect(img, threshold=5.0, taps_of=mvs.dog_taps)
    assert len(want) == 9
    for cap in (64, 4):
        chained, n_chain = _chain(ctx, img, params, cap)
        src = ctx.dev_alloc(img.nbytes)
        try:
            ctx.upload(src, img)
            dev1, n1 = ctx.detect_beads_dev(src, img.dtype, shape[::-1], cap, params=params)
            dev2, n2 = ctx.detect_beads_dev(src, img.dtype, shape[::-1], cap, params=params)
            ctx.release_caches()
            dev3, n3 = ctx.detect_beads_dev(src, img.dtype, shape[::-1], cap, params=params)
        finally:
            ctx.dev_free(src)
        host, nh = ctx.detect_beads(img, cap, params)
        assert n_chain == n1 == n2 == n3 == nh == len(want)
        for got in (chained, dev1, dev2, dev3, host):
            assert R.same_bits(got, want[:cap])
    det = mvs.DifferenceOfGaussian(threshold=5.0, ctx=ctx)
    peaks, n = det.detect(img)
    assert n == 9 and R.same_bits(peaks, want)


def test_rendered_beads_are_found_where_the_simulator_put_them(ctx, mvs):
    """render_beads_dev of 12 beads in 56 x 40 x 48 under the identity and under 45 degrees about x (axisRotation), float and uint16,
    detected without a download: as many detections as beads, one within 0.5 voxel of every true position, and the list the
    restatement finds in the downloaded image."""
    shape, interval, sigma = (48, 40, 56), ((0, 0, 0), (56, 40, 48)), R.BEAD_SIGMA
    mats = [np.eye(3, 4), mvs.SimulateMultiViewDataset.axisRotation((56, 40, 48), 0, 45)]
    hi = np.array([55.0, 39.0, 47.0])

    def keeps_margin(p):
        return all(np.all(q >= 8) and np.all(q <= hi - 8) for q in (mvs.beads.apply_affine(m, p) for m in mats))

    pts = R.draw_positions(shape, 12, np.random.default_rng(3), accept=keeps_margin)
    det = mvs.DifferenceOfGaussian(threshold=5.0, ctx=ctx)
    n = 56 * 40 * 48
    worst = 0.0
    for m in mats:
        for u16 in (False, True):
            peaks, found, truth = mvs.detection.detect_rendered(ctx, pts, m, interval, sigma, det, u16)
            assert np.allclose(truth, mvs.beads.apply_affine(m, pts))
            dist = R.nearest(truth, peaks["pos"])
            worst = max(worst, float(dist.max()))
            assert found == len(peaks) == 12 and np.all(dist <= 0.5)
            # the same image downloaded, through the restatement
            img = ctx.dev_alloc(n * (2 if u16 else 4))
            try:
                ctx.render_beads_dev(pts, interval, sigma, None if u16 else [img], [img] if u16 else None, matrices=np.asarray(m)[None])
                host = ctx.download(img, shape, np.uint16 if u16 else F32)
            finally:
                ctx.dev_free(img)
            want, _ = R.detect(host, threshold=5.0, taps_of=mvs.dog_taps)
            assert R.same_bits(peaks, want)
    print(f"largest distance between a true bead position and its detection: {worst:.4f} voxel")
    # the simulators' own entry points render and detect the same way
    sb = mvs.SimulateBeads([0, 45], 0, 12, ((0, 0, 0), (55, 39, 47)), interval, sigma)
    sb.points = pts
    peaks, found, truth = sb.detect(1, det)
    assert found == 12 and np.all(R.nearest(truth, peaks["pos"]) <= 0.5)
