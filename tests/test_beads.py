"""Bead images on the GPU (beads.hip) against the sequential restatement of SimulateBeads.renderPoints (tests/beads_restatement.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import beads_restatement as R

pytestmark = pytest.mark.gpu

SIGMAS = [(1.0, 1.0, 3.0), (0.5, 0.7, 2.0), (0.3, 0.3, 0.3)]


def _cloud(rng, n, interval, spill=4.0):
    """Random beads over the interval and a little beyond it, plus beads on the faces, at exactly max - min and just outside."""
    mn, mx = interval
    lo = np.array(mn, dtype=np.float64) - spill
    hi = np.array(mx, dtype=np.float64) + spill
    pts = lo + rng.random((n, 3)) * (hi - lo)
    edge = []
    for d in range(3):
        for v in (mn[d], mx[d], mn[d] - 1e-9, mx[d] + 1e-9, mx[d] - 0.5, mn[d] + 0.5):
            p = (np.array(mn) + np.array(mx)) / 2.0
            p[d] = v
            edge.append(p)
    edge.append(np.array(mx, dtype=np.float64))
    edge.append(np.array(mn, dtype=np.float64))
    return np.concatenate([pts, np.array(edge)])


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("interval", [((0, 0, 0), (40, 33, 21)), ((5, -7, -3), (70, 20, 30)), ((-20, 3, 11), (13, 50, 27))])
def test_bit_exact_against_the_sequential_restatement(ctx, sigma, interval):
    rng = np.random.default_rng(hash((sigma, interval)) & 0xFFFF)
    pts = _cloud(rng, 300, interval)
    got = ctx.render_beads(pts, interval, sigma)["f32"][0]
    want, n = R.render(pts, interval, sigma)
    assert n < 1_000_000 and n > 1000
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_bead_order_is_honoured(ctx):
    rng = np.random.default_rng(5)
    interval = ((0, 0, 0), (48, 40, 36))
    pts = np.array([20.3, 17.8, 15.1]) + (rng.random((300, 3)) - 0.5) * 4.0
    sigma = (1.3, 0.9, 2.2)
    got = ctx.render_beads(pts, interval, sigma)["f32"][0]
    fwd, _ = R.render(pts, interval, sigma)
    rev, _ = R.render(pts[::-1], interval, sigma)
    assert np.array_equal(got.view(np.uint32), fwd.view(np.uint32))
    assert not np.array_equal(fwd, rev), "the forward and reverse sums must differ somewhere for this test to mean anything"


def test_deterministic_and_chunking_invisible(mvs):
    rng = np.random.default_rng(11)
    interval = ((-3, 0, 2), (90, 70, 50))
    pts = _cloud(rng, 4000, interval)
    mats = np.stack([mvs.SimulateMultiViewDataset.axisRotation((94, 71, 49), 0, a) for a in (0, 30, 60)])
    with mvs.Context(0) as c:
        a = c.render_beads(pts, interval, (1, 1, 3), matrices=mats, f32=True, u16=True)
        b = c.render_beads(pts, interval, (1, 1, 3), matrices=mats, f32=True, u16=True)
        c.set_option("beads_pair_cap", 4096)          # bead ranges of one view in sequence, continued from the float image
        d = c.render_beads(pts, interval, (1, 1, 3), matrices=mats, f32=True, u16=True)
        e = c.render_beads(pts, interval, (1, 1, 3), matrices=mats, f32=False, u16=True)   # the same through the scratch image
    for v in range(3):
        assert np.array_equal(a["f32"][v].view(np.uint32), b["f32"][v].view(np.uint32))
        assert np.array_equal(a["f32"][v].view(np.uint32), d["f32"][v].view(np.uint32))
        assert np.array_equal(a["u16"][v], b["u16"][v]) and np.array_equal(a["u16"][v], d["u16"][v])
        assert np.array_equal(a["u16"][v], e["u16"][v])
        assert np.array_equal(a["u16"][v], mvs.beads.to_unsigned_short(a["f32"][v]))


def test_simulate_beads_main_equals_the_restatement(mvs):
    """SimulateBeads.main (:207-224): angles 0/45/90/135 about x, 1000 points, 512 x 512 x 200, sigma (1, 1, 3)."""
    rng = ((0, 0, 0), (511, 511, 199))
    sb = mvs.SimulateBeads([0, 45, 90, 135], 0, 1000, rng, rng, [1, 1, 3])
    imgs = sb.getImgs()
    pts = mvs.SimulateBeads.randomPoints(1000, rng, mvs.JavaRandom(535))
    lists = mvs.SimulateBeads.transformPoints(pts, [0, 45, 90, 135], 0, rng)
    assert len(imgs) == 4
    for img, lst in zip(imgs, lists):
        want, n = R.render(lst, rng, (1, 1, 3))
        assert img.shape == (199, 511, 511)
        diff = img.view(np.uint32) != want.view(np.uint32)
        assert int(diff.sum()) <= max(1, n // 1_000_000)
        if diff.any():
            assert np.all(np.abs(img.view(np.int32)[diff].astype(np.int64) - want.view(np.int32)[diff]) <= 1)


def test_simulate_beads2_views_u16_and_normalize(mvs):
    rng = ((0, 0, 0), (96, 80, 40))
    sb = mvs.SimulateBeads2(400, [1, 1, 3], ((-20, -20, -10), (116, 100, 50)), rng)
    sb.addAngle(0, 1, 30.0)
    for t, s in enumerate(([0, 0, 0], [10.5, 0, 0])):
        sb.addTile(t, s)
    for ch, s in enumerate(([0, 0, 0], [0.25, -1.5, 0])):
        sb.addChannel(ch, s)
    for il, s in enumerate(([0, 0, 0], [0, 0, 2.0])):
        sb.addIllumination(il, s)
    for tile in (0, 1):
        for ch in (0, 1):
            for il in (0, 1):
                img = sb.getImg(0, 0, ch, tile, il)
                assert sb.getImg(0, 0, ch, tile, il) is img          # cached
                m = sb.transform(0, 0, ch, tile, il).m
                want, _ = R.render(R.apply(m, sb.points), rng, (1, 1, 3))
                assert np.array_equal(img.view(np.uint32), want.view(np.uint32))
                u16 = sb.getImage(0, 0, ch, tile, il)
                assert u16.dtype == np.uint16 and np.array_equal(u16, mvs.beads.to_unsigned_short(img))
                nf = sb.getFloatImage(0, 0, ch, tile, il, True)
                mn, mx = np.float32(img.min()), np.float32(img.max())
                assert np.array_equal(nf, ((img - mn) / (mx - mn)).astype(np.float32))
    # a voxel beyond 65535 wraps modulo 2^16 in the uint16 image
    pts = np.tile([[10.2, 11.7, 6.4]], (80, 1))
    with mvs.Context(0) as c:
        r = c.render_beads(pts, ((0, 0, 0), (24, 24, 14)), (1, 1, 1), f32=True, u16=True)
        f, u = r["f32"][0], r["u16"][0]
        assert f.max() > 65535
        assert np.array_equal(u, (np.floor(f.astype(np.float64) + 0.5).astype(np.int64) & 0xFFFF).astype(np.uint16))
        const = np.full((4, 5, 6), 3.0, dtype=np.float32)
        c.beads_normalize(const)
        assert np.isnan(const).all()


def test_stacked_views_equal_single_views_and_offsets_equal_lists(mvs, ctx):
    rng = np.random.default_rng(21)
    interval = ((0, 0, 0), (60, 52, 30))
    pts = _cloud(rng, 1500, interval)
    mats = np.stack([mvs.SimulateMultiViewDataset.axisRotation((61, 53, 31), 1, a) for a in range(0, 180, 30)])
    stacked = ctx.render_beads(pts, interval, (0.5, 0.7, 2), matrices=mats)["f32"]
    lists = [R.apply(m, pts) for m in mats]
    for v in range(6):
        single = ctx.render_beads(pts, interval, (0.5, 0.7, 2), matrices=mats[v:v + 1])["f32"][0]
        assert np.array_equal(stacked[v].view(np.uint32), single.view(np.uint32))
    lens = [len(l) - 100 * v for v, l in enumerate(lists)]
    cut = [l[:k] for l, k in zip(lists, lens)]
    offs = np.concatenate([[0], np.cumsum(lens)])
    by_offsets = ctx.render_beads(np.concatenate(cut), interval, (0.5, 0.7, 2), view_offsets=offs)["f32"]
    copies = [c.copy() for c in cut]
    by_lists = mvs.SimulateBeads.renderPoints(copies, interval, (0.5, 0.7, 2))
    for v in range(6):
        want, _ = R.render(cut[v], interval, (0.5, 0.7, 2))
        assert np.array_equal(by_offsets[v].view(np.uint32), want.view(np.uint32))
        assert np.array_equal(by_lists[v].view(np.uint32), want.view(np.uint32))
    # renderPoints adjusts the caller's points (isInsideAdjust)
    for v in range(6):
        assert np.array_equal(copies[v], mvs.beads._adjust(cut[v], *interval))


EDGE_INTERVAL = ((0, 0, 0), (40, 33, 21))      # 2 x 5 x 2 bricks of 32 x 8 x 16, none of them whole


def _all_zero(r):
    return all(not f.view(np.uint32).any() for f in r["f32"]) and all(not u.any() for u in r["u16"])


def test_empty_bead_list_gives_positive_zero_images(ctx):
    """No bead at all: the binner sorts its one padded slot, every brick's list is empty, every voxel is written +0.0f / 0."""
    r = ctx.render_beads(np.zeros((0, 3)), EDGE_INTERVAL, (1.0, 1.0, 3.0), f32=True, u16=True)
    assert r["f32"][0].shape == (21, 33, 40) and r["u16"][0].shape == (21, 33, 40)
    assert _all_zero(r)


def test_empty_view_between_two_views_of_one_call(ctx):
    """view_offsets with an empty view in the middle: a job without pairs between jobs with pairs, its keys a run of empty lists."""
    rng = np.random.default_rng(31)
    sigma = (1.0, 1.0, 3.0)
    pts = _cloud(rng, 200, EDGE_INTERVAL)
    k = 90
    r = ctx.render_beads(pts, EDGE_INTERVAL, sigma, view_offsets=[0, k, k, len(pts)], f32=True, u16=True)
    assert len(r["f32"]) == 3 and len(r["u16"]) == 3
    assert not r["f32"][1].view(np.uint32).any() and not r["u16"][1].any()
    for v, part in ((0, pts[:k]), (2, pts[k:])):
        single = ctx.render_beads(part, EDGE_INTERVAL, sigma, f32=True, u16=True)
        assert single["f32"][0].any()
        assert np.array_equal(r["f32"][v].view(np.uint32), single["f32"][0].view(np.uint32))
        assert np.array_equal(r["u16"][v], single["u16"][0])


def test_beads_that_all_lie_outside_the_interval_give_zero_images(ctx):
    """A non-empty list of which the cull keeps nothing: counts that scan to zero pairs, so the pad starts at slot 0."""
    rng = np.random.default_rng(32)
    mx = np.array(EDGE_INTERVAL[1], dtype=np.float64)
    far = mx + 5.0 + rng.random((150, 3)) * 30.0                          # beyond max on every axis
    near = np.array([[-1e-9, 10.0, 10.0], [20.0, 33.0 + 1e-9, 10.0], [20.0, 10.0, -0.5], [np.nan, 10.0, 10.0]])
    r = ctx.render_beads(np.concatenate([far, near, -far]), EDGE_INTERVAL, (1.0, 1.0, 3.0), f32=True, u16=True)
    assert _all_zero(r)


def test_large_dense_case_on_the_device(mvs, ctx):
    """10^6 beads, 2048 x 2048 x 512, 4 angles, float and uint16 images resident on the device."""
    nx, ny, nz = 2048, 2048, 512
    interval = ((0, 0, 0), (nx, ny, nz))
    sigma = (1.0, 1.0, 3.0)
    pts = mvs.SimulateBeads.randomPoints(1_000_000, interval, mvs.JavaRandom(535))
    mats = np.stack([mvs.SimulateMultiViewDataset.axisRotation((nx + 1, ny + 1, nz + 1), 0, a) for a in (0, 45, 90, 135)])
    nv = nx * ny * nz
    f_ptrs = [ctx.dev_alloc(4 * nv) for _ in range(4)]
    u_ptrs = [ctx.dev_alloc(2 * nv) for _ in range(4)]
    try:
        ctx.render_beads_dev(pts, interval, sigma, f_ptrs, u_ptrs, matrices=mats)
        ctx.synchronize()
        for v in (0, 3):
            lst = R.apply(mats[v], pts)
            for (x0, y0, z0) in ((0, 0, 0), (1000, 1500, 200), (nx - 64, ny - 64, nz - 64)):
                w0, w1 = (x0, y0, z0), (x0 + 64, y0 + 64, z0 + 64)
                near = np.all((lst >= np.array(w0) - 20) & (lst <= np.array(w1) + 20), axis=1)
                want, _ = R.render(lst[near], interval, sigma, window=(w0, w1))
                got = np.empty((64, ny, nx), dtype=np.float32)
                mvs._lib.check(ctx._L.mvsim_download(ctx._h, C.c_void_p(got.ctypes.data), C.c_void_p(f_ptrs[v] + 4 * z0 * nx * ny), 4 * 64 * nx * ny))
                win = got[:, y0:y0 + 64, x0:x0 + 64]
                assert np.array_equal(win.view(np.uint32), want.view(np.uint32)), (v, w0)
                gu = np.empty((64, ny, nx), dtype=np.uint16)
                mvs._lib.check(ctx._L.mvsim_download(ctx._h, C.c_void_p(gu.ctypes.data), C.c_void_p(u_ptrs[v] + 2 * z0 * nx * ny), 2 * 64 * nx * ny))
                assert np.array_equal(gu, mvs.beads.to_unsigned_short(got))
        # the sum of all voxels of view 0 against the fp64 sum of the contributions
        lst = R.apply(mats[0], pts)
        keep = np.all((lst >= 0) & (lst <= np.array([nx, ny, nz])), axis=1)
        loc = lst[keep]
        total = np.ones(len(loc))
        for d, (n_d, s) in enumerate(zip((nx, ny, nz), sigma)):
            size = R.kernel_diameter(s) * 2
            lo = np.floor(loc[:, d] + 0.5).astype(np.int64) - size // 2
            pos = lo[:, None] + np.arange(size)[None, :]
            x = loc[:, d][:, None] - pos
            e = np.exp(-(x * x) / (2 * s * s))
            e[(pos < 0) | (pos >= n_d)] = 0.0
            total *= e.sum(axis=1)
        analytic = 1000.0 * total.sum()
        acc = 0.0
        plane = np.empty((32, ny, nx), dtype=np.float32)
        for z0 in range(0, nz, 32):
            mvs._lib.check(ctx._L.mvsim_download(ctx._h, C.c_void_p(plane.ctypes.data), C.c_void_p(f_ptrs[0] + 4 * z0 * nx * ny), plane.nbytes))
            acc += float(plane.sum(dtype=np.float64))
        assert abs(acc - analytic) <= 1e-6 * analytic
    finally:
        for p in f_ptrs + u_ptrs:
            ctx.dev_free(p)
