"""The view fusion on the GPU against the restatement of tests/fuse_reference.py, bit for bit (NaNs compared as NaNs), through the C
ABI: fused and aligned output over every brick edge, source size, matrix, blend and view count, matrices read from device memory,
the host entry, repeatability -- and the loop closed on the device: rendered views detected, registered, fused, and aligned views fed
to the deconvolution.  Guard bytes behind every output stay intact and no input is written."""
import numpy as np
import pytest

from . import dog_reference as D
from . import fuse_reference as R
from . import register_reference as REG
from .test_register import Arena
from .test_register_host import LOOP_BEADS, LOOP_INTERVAL, loop_cloud

pytestmark = pytest.mark.gpu
F64 = np.float64
SOURCES = [(1, 1, 1), (2, 1, 3), (5, 4, 3), (40, 33, 17)]          # x, y, z


def volume(dim_xyz, seed=0, u16=False):
    rng = np.random.default_rng(seed + 17 * dim_xyz[0])
    v = rng.uniform(0, 60000, dim_xyz[::-1]) if u16 else rng.uniform(-3, 900, dim_xyz[::-1])
    return v.astype(np.uint16 if u16 else np.float32)


def n_of(dim):
    return int(dim[0]) * int(dim[1]) * int(dim[2])


def shape_of(dim):
    return (int(dim[2]), int(dim[1]), int(dim[0]))


def run_fused(ctx, mvs, views, mats, out_min, out_dim, blend=(8, 8, 8), background=0.0, dev_matrices=(), want_sum=True, want_status=True):
    """mvsim_fuse_views_dev: (fused, sum of weights, status); ``dev_matrices``: the views whose matrix is read from device memory."""
    u16 = views[0].dtype == np.uint16
    p = mvs.fuse_params(blend=blend, background=background, src_type=mvs._lib.MVSIM_SRC_U16 if u16 else mvs._lib.MVSIM_SRC_F32)
    n, V = n_of(out_dim), len(views)
    with Arena(ctx) as A:
        srcs = [A.put(v) for v in views]
        mdev = [A.put(np.asarray(mats[v], F64).reshape(12)) if v in dev_matrices else 0 for v in range(V)]
        host = [np.full((3, 4), 1e300) if v in dev_matrices else mats[v] for v in range(V)]       # ignored where m_dev is given
        out, sw, st = A.out(4 * n), A.out(4 * n), A.out(4 * V)
        ctx.fuse_views_dev(srcs, [v.shape[::-1] for v in views], host, out_min, out_dim, out, sw if want_sum else 0, st if want_status else 0,
                           params=p, matrix_dptrs=mdev)
        got = (A.get(out, 4 * n, 4 * n).view(np.float32).reshape(shape_of(out_dim)),
               A.get(sw, 4 * n, 4 * n if want_sum else 0).view(np.float32).reshape(shape_of(out_dim) if want_sum else (0,)),
               A.get(st, 4 * V, 4 * V if want_status else 0).view(np.int32))
        A.check_inputs()
    return got


def run_aligned(ctx, mvs, views, mats, out_min, out_dim, blend=(8, 8, 8), want_aligned=None, want_weights=None, dev_matrices=()):
    """mvsim_align_views_dev: ([aligned or None], [weight or None], status); want_*: per view, whether the output is asked for
    (want_weights = False: no weight table at all)."""
    u16 = views[0].dtype == np.uint16
    p = mvs.fuse_params(blend=blend, src_type=mvs._lib.MVSIM_SRC_U16 if u16 else mvs._lib.MVSIM_SRC_F32)
    n, V = n_of(out_dim), len(views)
    wa = [True] * V if want_aligned is None else want_aligned
    ww = [True] * V if want_weights is None else ([False] * V if want_weights is False else want_weights)
    with Arena(ctx) as A:
        srcs = [A.put(v) for v in views]
        mdev = [A.put(np.asarray(mats[v], F64).reshape(12)) if v in dev_matrices else 0 for v in range(V)]
        al, wt, st = [A.out(4 * n) for _ in range(V)], [A.out(4 * n) for _ in range(V)], A.out(4 * V)
        ctx.align_views_dev(srcs, [v.shape[::-1] for v in views], mats, out_min, out_dim, [a if k else 0 for a, k in zip(al, wa)],
                            None if want_weights is False else [w if k else 0 for w, k in zip(wt, ww)], st, params=p, matrix_dptrs=mdev)
        got_al = [A.get(a, 4 * n, 4 * n if k else 0).view(np.float32) for a, k in zip(al, wa)]
        got_wt = [A.get(w, 4 * n, 4 * n if k else 0).view(np.float32) for w, k in zip(wt, ww)]
        status = A.get(st, 4 * V, 4 * V).view(np.int32)
        A.check_inputs()
    s = shape_of(out_dim)
    return [a.reshape(s) if k else None for a, k in zip(got_al, wa)], [w.reshape(s) if k else None for w, k in zip(got_wt, ww)], status


def check(ctx, mvs, views, mats, out_min, out_dim, blend=(8, 8, 8), background=0.0, aligned=True, **kw):
    """Both modes against the restatement; returns the restatement's (fused, sum of weights, status)."""
    want = R.fuse(views, mats, out_min, out_dim, blend, background)
    got = run_fused(ctx, mvs, views, mats, out_min, out_dim, blend, background, **kw)
    assert R.same_bits(got[0], want[0]), "fused volume"
    assert R.same_bits(got[1], want[1]), "sum of weights"
    assert np.array_equal(got[2], want[2]), "status words"
    if aligned:
        wal, wwt, wst = R.align(views, mats, out_min, out_dim, blend)
        al, wt, st = run_aligned(ctx, mvs, views, mats, out_min, out_dim, blend, **kw)
        for v in range(len(views)):
            assert R.same_bits(al[v], wal[v]), f"aligned view {v}"
            assert R.same_bits(wt[v], wwt[v]), f"weights of view {v}"
        assert np.array_equal(st, wst)
    return want


def placed(views, out_min, out_dim, seed=0):
    """Matrices that put every view somewhere into the output interval: a small rotation about each axis in turn, then a shift of the
    view's centre onto a random point of the interval."""
    rng = np.random.default_rng(seed)
    mats = []
    for k, v in enumerate(views):
        c = (np.array(v.shape[::-1], F64) - 1) / 2
        m = R.rotation(k % 3, rng.uniform(-25, 25), c)
        m[:, 3] += np.array(out_min, F64) + rng.uniform(0.2, 0.8, 3) * np.array(out_dim, F64) - c
        mats.append(m)
    return mats


def oblique():
    c = (19.5, 16.0, 8.0)
    shear = R.identity()
    shear[0, 1], shear[1, 2], shear[2, 0], shear[:, 3] = 0.3, -0.2, 0.1, (1.5, 2.0, -0.75)
    return {"rot_x": R.rotation(0, 33, c), "rot_y": R.rotation(1, -21, c), "rot_z": R.rotation(2, 57, c),
            "scale": np.hstack([np.diag([1.7, 0.6, 2.3]), [[-3.0], [4.5], [0.25]]]), "shear": shear}


# ---- identity -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u16", [False, True], ids=["float", "uint16"])
def test_identity_returns_the_input(ctx, mvs, u16):
    for dim in SOURCES + [(70, 9, 6)]:
        src = volume(dim, u16=u16)
        fused, den, status = run_fused(ctx, mvs, [src], [R.identity()], (0, 0, 0), dim, blend=(0, 0, 0))
        assert R.same_bits(fused, src.astype(np.float32)) and np.all(den == 1.0) and status[0] == 0
        al, wt, _ = run_aligned(ctx, mvs, [src], [R.identity()], (0, 0, 0), dim, blend=(0, 0, 0))
        assert R.same_bits(al[0], src.astype(np.float32)) and np.all(wt[0] == 1.0)


# ---- the launch geometry --------------------------------------------------------------------------------------------------------------------
def edge_sizes(brick):
    return [1, brick - 1, brick, brick + 1, 2 * brick + 1]


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_output_extents_at_the_bricks_edges(ctx, mvs, axis):
    """Every source size in one call, views of different sizes; the output runs over 1, brick-1, brick, brick+1 and 2 brick+1 voxels
    along one axis and over brick+1 along the others."""
    brick = mvs.fusion_geometry()["brick"]
    views = [volume(d, seed=3) for d in SOURCES]
    for size in edge_sizes(brick[axis]):
        if size < 1:
            continue
        out_dim = [min(b + 1, 9) for b in brick]
        out_dim[axis] = size
        out_min = (-2, 3, -1)
        mats = placed(views, out_min, out_dim, seed=size)
        want = check(ctx, mvs, views, mats, out_min, out_dim, blend=(2.5, 2.5, 2.5), background=-1.0)
        assert size < 4 or (want[1] > 0).any(), "the case must see a view"
    out_dim = [2 * b + 1 for b in brick]                    # all three at once
    check(ctx, mvs, views, placed(views, (0, 0, 0), out_dim, seed=99), (0, 0, 0), out_dim, blend=(2.5, 2.5, 2.5))


def test_more_bricks_than_blocks(ctx, mvs):
    """More bricks than the launch has blocks: every block walks several bricks of its run, and the runs' ends are ragged."""
    g = mvs.fusion_geometry()
    bx, by, bz = g["brick"]
    side = int(np.ceil(np.sqrt(g["max_blocks"]))) + 1
    out_dim = (bx + 1, by * side - 1, bz * side + 1)
    assert 2 * side * side > g["max_blocks"] + 8
    views = [volume((40, 33, 17), seed=5), volume((5, 4, 3), seed=5)]
    stretch = [np.hstack([np.diag([1.5, out_dim[1] / 40.0, out_dim[2] / 20.0]), [[2.0], [3.0], [1.0]]]),
               np.hstack([np.diag([9.0, out_dim[1] / 3.5, out_dim[2] / 2.5]), [[0.0], [0.0], [5.0]]])]
    want = check(ctx, mvs, views, stretch, (0, 0, 0), out_dim, blend=(3.5, 3.5, 3.5), aligned=False)
    assert (want[1] > 0).mean() > 0.5


# ---- matrices -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rot_x", "rot_y", "rot_z", "scale", "shear"])
def test_oblique_matrices(ctx, mvs, name):
    m = oblique()[name]
    src = volume((40, 33, 17), seed=7)
    out_min, out_dim = R.bounds([m], [(40, 33, 17)])
    assert all(1 <= d <= 110 for d in out_dim)
    want = check(ctx, mvs, [src], [m], out_min, out_dim, blend=(3.5, 3.5, 3.5))
    assert 0.1 < (want[1] > 0).mean() < 1.0 or name == "scale"
    check(ctx, mvs, [src, volume((5, 4, 3))], [m, R.translation((7, 7, 3))], out_min, out_dim, blend=(0, 0, 0))


def test_positions_exactly_on_the_faces(ctx, mvs):
    """p lands exactly on 0 and on N - 1: integer translations over an interval that overhangs the view by two voxels on every side, and
    a scale by two, whose half-integer positions end exactly on the last voxel."""
    src = volume((5, 4, 3), seed=8)
    want = check(ctx, mvs, [src], [R.translation((3, -2, 1))], (1, -4, -1), (9, 8, 7), blend=(0, 0, 0), background=-9.0)
    assert R.same_bits(want[0][2:5, 2:6, 2:7], src) and (want[0] == -9.0).sum() == 9 * 8 * 7 - src.size
    double = np.hstack([np.diag([2.0, 2.0, 2.0]), np.zeros((3, 1))])
    want = check(ctx, mvs, [src], [double], (-1, -1, -1), (11, 9, 7), blend=(1.5, 1.5, 1.5))
    assert want[1][1 + 4, 1 + 6, 1 + 8] == 0.0 and want[1][1 + 2, 1 + 3, 1 + 4] > 0.0
    check(ctx, mvs, [volume((1, 1, 1))], [R.identity()], (-1, -1, -1), (3, 3, 3), blend=(0, 0, 0))
    check(ctx, mvs, [volume((1, 1, 1))], [R.identity()], (-1, -1, -1), (3, 3, 3), blend=(2, 2, 2))      # its only voxel has weight 0


def test_negative_partial_and_empty_intervals(ctx, mvs):
    views = [volume((40, 33, 17), seed=9), volume((40, 33, 17), seed=10)]
    mats = [R.identity(), R.rotation(0, 45, (19.5, 16.0, 8.0))]
    # far in the negative; an interval wider than a brick that only partly overlaps the views, so that whole bricks miss a view
    want = check(ctx, mvs, views, mats, (-30, -20, -10), (25, 15, 8), blend=(3.5, 3.5, 3.5))
    assert (want[1] == 0).all()
    want = check(ctx, mvs, views, mats, (-70, -9, -6), (200, 30, 20), blend=(3.5, 3.5, 3.5), background=2.0)
    assert 0.0 < (want[1] > 0).mean() < 0.3
    want = check(ctx, mvs, views, mats, (20, 10, 5), (150, 12, 30), blend=(3.5, 3.5, 3.5))
    assert 0.0 < (want[1] > 0).mean() < 0.5
    # no view reaches the interval: all background
    want = check(ctx, mvs, views, mats, (500, 500, 500), (70, 6, 6), background=12.5)
    assert np.all(want[0] == np.float32(12.5)) and np.all(want[1] == 0.0)


@pytest.mark.parametrize("blend", [(0, 0, 0), (3.5, 3.5, 3.5), (30, 30, 30), (0, 2.5, 7)], ids=["0", "3.5", "above-half", "per-axis"])
def test_blends(ctx, mvs, blend):
    views = [volume((40, 33, 17), seed=11), volume((5, 4, 3), seed=11), volume((2, 1, 3), seed=11)]
    mats = [R.rotation(2, 12, (19.5, 16, 8)), R.translation((10.25, 9.5, 4.75)), R.translation((20, 20, 7.5))]
    check(ctx, mvs, views, mats, (-3, -3, -2), (48, 40, 21), blend=blend)


@pytest.mark.parametrize("V", [1, 2, 4, R.MAX_VIEWS])
def test_view_counts(ctx, mvs, V):
    rng = np.random.default_rng(V)
    views = [volume(SOURCES[2 + v % 2], seed=v) for v in range(V)]
    mats = []
    for v, src in enumerate(views):
        m = R.rotation(v % 3, rng.uniform(-15, 15), (np.array(src.shape[::-1], F64) - 1) / 2)
        m[:, 3] += rng.uniform(0, 3, 3)
        mats.append(m)
    out_min, out_dim = (-4, -4, -4), (66, 44, 27)
    check(ctx, mvs, views, mats, out_min, out_dim, blend=(2, 2, 2))
    cover = sum(R.resample(src, m, out_min, out_dim, (2, 2, 2))[2].astype(int) for src, m in zip(views, mats))
    assert cover.max() >= min(V, 3), "the views must overlap"


def test_uint16_sources(ctx, mvs):
    views = [volume((40, 33, 17), seed=12, u16=True), volume((5, 4, 3), seed=12, u16=True)]
    check(ctx, mvs, views, [oblique()["rot_x"], R.translation((30.5, 3.25, 2))], (-5, -5, -5), (70, 44, 27), blend=(3.5, 3.5, 3.5))


def test_planted_non_finite_voxels(ctx, mvs):
    src = volume((40, 33, 17), seed=13)
    rng = np.random.default_rng(13)
    at = rng.permutation(src.size)[:60]
    src.reshape(-1)[at] = rng.choice([np.nan, np.inf, -np.inf], len(at)).astype(np.float32)
    other = volume((40, 33, 17), seed=14)
    for blend in ((0, 0, 0), (3.5, 3.5, 3.5)):
        want = check(ctx, mvs, [src, other], [R.rotation(0, 10, (19.5, 16, 8)), R.identity()], (-2, -2, -2), (44, 37, 21), blend=blend)
        assert np.isnan(want[0]).any() and np.isfinite(want[0]).any()
    want = check(ctx, mvs, [src], [R.identity()], (0, 0, 0), (40, 33, 17), blend=(0, 0, 0))      # u = 0, yet inf - inf is NaN
    assert np.isnan(want[0]).sum() > np.isnan(src).sum()


def test_singular_and_non_finite_matrices_leave_the_view_out(ctx, mvs):
    views = [volume((5, 4, 3), seed=v) for v in range(4)]
    flat = R.identity()
    flat[1, 1] = 0.0
    bad = R.identity()
    bad[2, 3] = np.nan
    mats = [R.identity(), flat, bad, R.translation((1, 1, 0))]
    want = check(ctx, mvs, views, mats, (0, 0, 0), (8, 8, 4), blend=(0, 0, 0))
    assert list(want[2]) == [0, R.SINGULAR, R.SINGULAR, 0]
    only = R.fuse([views[0], views[3]], [mats[0], mats[3]], (0, 0, 0), (8, 8, 4), (0, 0, 0))
    assert R.same_bits(want[0], only[0]) and R.same_bits(want[1], only[1])
    check(ctx, mvs, views, mats, (0, 0, 0), (8, 8, 4), dev_matrices=(0, 1, 2, 3))
    want = check(ctx, mvs, views[:1], [flat], (0, 0, 0), (70, 5, 5), background=3.0)
    assert np.all(want[0] == 3.0)
    # the status words are optional, and so is the sum of weights
    got = run_fused(ctx, mvs, views, mats, (0, 0, 0), (8, 8, 4), (0, 0, 0), want_sum=False, want_status=False)
    assert R.same_bits(got[0], only[0])


def test_aligned_mode_with_null_entries(ctx, mvs):
    views = [volume((40, 33, 17), seed=15), volume((5, 4, 3), seed=15), volume((2, 1, 3), seed=15)]
    mats = [oblique()["rot_z"], R.translation((10.25, 9.5, 4.75)), R.translation((1, 1, 1))]
    out_min, out_dim = (-6, -6, -3), (70, 50, 24)
    wal, wwt, _ = R.align(views, mats, out_min, out_dim, (3.5, 3.5, 3.5))
    for wa, ww in (([True, False, True], [False, True, True]), ([False, False, False], [True, False, False]), ([True, True, False], False)):
        al, wt, _ = run_aligned(ctx, mvs, views, mats, out_min, out_dim, (3.5, 3.5, 3.5), wa, ww)
        for v in range(3):
            assert (al[v] is None) == (not wa[v]) and (al[v] is None or R.same_bits(al[v], wal[v]))
            assert wt[v] is None or R.same_bits(wt[v], wwt[v])


def test_matrices_from_device_memory_give_the_same_bits(ctx, mvs):
    views = [volume((40, 33, 17), seed=16), volume((5, 4, 3), seed=16), volume((40, 33, 17), seed=17)]
    mats = [oblique()["rot_x"], R.translation((10.25, 9.5, 4.75)), oblique()["shear"]]
    want = check(ctx, mvs, views, mats, (-6, -6, -3), (70, 50, 24), blend=(3.5, 3.5, 3.5))
    for dev in ((0, 1, 2), (1,), (0, 2)):
        got = run_fused(ctx, mvs, views, mats, (-6, -6, -3), (70, 50, 24), (3.5, 3.5, 3.5), dev_matrices=dev)
        assert R.same_bits(got[0], want[0]) and R.same_bits(got[1], want[1]) and np.array_equal(got[2], want[2])
        check(ctx, mvs, views, mats, (-6, -6, -3), (70, 50, 24), blend=(3.5, 3.5, 3.5), dev_matrices=dev)


def test_host_entry_repeats_and_released_caches(ctx, mvs):
    views = [volume((40, 33, 17), seed=18), volume((5, 4, 3), seed=18)]
    mats = [oblique()["rot_y"], np.zeros((3, 4))]
    out_min, out_dim = (-6, -6, -3), (70, 50, 24)
    first = run_fused(ctx, mvs, views, mats, out_min, out_dim, (3.5, 3.5, 3.5), 1.5)
    want = R.fuse(views, mats, out_min, out_dim, (3.5, 3.5, 3.5), 1.5)
    assert all(R.same_bits(a, b) for a, b in zip(first, want))
    p = mvs.fuse_params(blend=3.5, background=1.5)
    host = ctx.fuse_views(views, mats, out_min, out_dim, p, sum_weights=True, status=True)
    assert all(R.same_bits(a, b) for a, b in zip(host, first)), "the host entry against the device entry"
    assert R.same_bits(ctx.fuse_views(views, mats, out_min, out_dim, p), first[0])
    f = mvs.ViewFusion(ctx=ctx, blend=3.5, background=1.5)
    assert R.same_bits(f.fuse(views, mats, (out_min, out_dim)), first[0])
    assert R.same_bits(f.fuse(views, mats), R.fuse(views, mats, (0, 0, 0), (40, 33, 17), (3.5, 3.5, 3.5), 1.5)[0]), "view 0's own interval"
    al, wt, st = ctx.align_views(views, mats, out_min, out_dim, p, status=True)
    wal, wwt, wst = R.align(views, mats, out_min, out_dim, (3.5, 3.5, 3.5))
    assert all(R.same_bits(a, b) for a, b in zip(al + wt, wal + wwt)) and np.array_equal(st, wst)
    al2, none = f.align(views, mats, (out_min, out_dim), weights=False)
    assert none is None and all(R.same_bits(a, b) for a, b in zip(al2, wal))
    u16 = [v.astype(np.uint16) for v in views]
    got = ctx.fuse_views(u16, mats, out_min, out_dim, mvs.fuse_params(blend=3.5, src_type=mvs._lib.MVSIM_SRC_U16))
    assert R.same_bits(got, R.fuse(u16, mats, out_min, out_dim, (3.5, 3.5, 3.5))[0])
    # a second call; a call after the caches were released
    assert all(R.same_bits(a, b) for a, b in zip(run_fused(ctx, mvs, views, mats, out_min, out_dim, (3.5, 3.5, 3.5), 1.5), first))
    ctx.release_caches()
    assert all(R.same_bits(a, b) for a, b in zip(run_fused(ctx, mvs, views, mats, out_min, out_dim, (3.5, 3.5, 3.5), 1.5), first))
    with pytest.raises(ValueError, match="overlaps"):
        with Arena(ctx) as A:
            src = A.put(views[0])
            ctx.fuse_views_dev([src], [(40, 33, 17)], [R.identity()], (0, 0, 0), (40, 33, 17), src + 4 * views[0].size - 4)


def test_weights_of_the_aligned_views_sum_to_the_fused_sum(ctx, mvs):
    """Where every view's weight is a float already (1, 0, or a dyadic ramp value), the float sum over the weight volumes is exact
    and must equal the fused call's sum of weights."""
    views = [volume((40, 33, 17), seed=19), volume((40, 33, 17), seed=20), volume((5, 4, 3), seed=19)]
    mats = [R.identity(), R.translation((3, -2, 1)), R.rotation(2, 30, (2, 1.5, 1))]
    out_min, out_dim = (-4, -4, -2), (50, 42, 22)
    for blend in ((0, 0, 0), (4, 4, 4)):
        _, den, _ = run_fused(ctx, mvs, views, mats, out_min, out_dim, blend)
        _, wt, _ = run_aligned(ctx, mvs, views, mats, out_min, out_dim, blend, want_aligned=[False] * 3)
        w64 = [R.resample(v, m, out_min, out_dim, blend)[1] for v, m in zip(views, mats)]
        exact = np.all([w.astype(np.float32).astype(F64) == w for w in w64], axis=0)
        total = wt[0].astype(F64) + wt[1].astype(F64) + wt[2].astype(F64)
        exact &= total.astype(np.float32).astype(F64) == total
        assert exact.mean() > (0.99 if blend[0] == 0 else 0.2)
        assert np.array_equal(total.astype(np.float32)[exact], den[exact])


# ---- the closed loop --------------------------------------------------------------------------------------------------------------------
LOOP_DIM = (128, 128, 96)


@pytest.fixture(scope="module")
def loop(ctx, mvs):
    """The two views of tests/test_register_host.py's cloud rendered, detected, registered A -> B and fused into B's interval on the
    device, nothing downloaded in between; then everything downloaded once, for the tests below to share."""
    pts, mats = loop_cloud(mvs)
    det = mvs.DifferenceOfGaussian(threshold=5.0, ctx=ctx, capacity=256)
    item, cap, n = D.PEAK_DTYPE.itemsize, det.capacity, n_of(LOOP_DIM)
    p = mvs.fuse_params()
    with Arena(ctx) as A:
        img = [A.out(4 * n), A.out(4 * n)]
        pk = [A.out(cap * item + 8), A.out(cap * item + 8)]
        res, out, sw, st = A.out(160), A.out(4 * n), A.out(4 * n), A.out(8)
        for m, im, at in zip(mats, img, pk):
            ctx.render_beads_dev(pts, LOOP_INTERVAL, D.BEAD_SIGMA, [im], None, matrices=np.asarray(m)[None])
            ctx.detect_beads_dev(im, np.float32, LOOP_DIM, cap, at, at + cap * item, params=det.params)
        ctx.register_beads_dev(pk[0], item, pk[0] + cap * item, cap, pk[1], item, pk[1] + cap * item, cap, res, params=mvs.match_params())
        ctx.fuse_views_dev(img, [LOOP_DIM] * 2, [None, R.identity()], (0, 0, 0), LOOP_DIM, out, sw, st, params=p, matrix_dptrs=[res, 0])
        got = {"fused": A.get(out, 4 * n, 4 * n).view(np.float32).reshape(shape_of(LOOP_DIM)),
               "sum": A.get(sw, 4 * n, 4 * n).view(np.float32).reshape(shape_of(LOOP_DIM)), "status": A.get(st, 8, 8).view(np.int32),
               "imgs": [A.get(im, 4 * n, 4 * n).view(np.float32).reshape(shape_of(LOOP_DIM)) for im in img],
               "reg": A.get(res, 160, 160).view(REG.REGISTRATION_DTYPE)[0]}
        found = [int(ctx.download(at + cap * item, (1,), np.int64)[0]) for at in pk]
        got["peaks"] = [ctx.download(at, (k,), D.PEAK_DTYPE) for at, k in zip(pk, found)]
    got["truth"] = mvs.registration.true_transform(mats[0], mats[1], LOOP_INTERVAL[0])
    got["det"] = det
    return got


def test_rendered_views_fuse_from_their_registration(loop):
    assert loop["reg"]["flags"] == 0 and list(loop["status"]) == [0, 0] and len(loop["peaks"][1]) == LOOP_BEADS
    want = R.fuse(loop["imgs"], [loop["reg"]["m"], R.identity()], (0, 0, 0), LOOP_DIM)
    assert R.same_bits(loop["fused"], want[0]) and R.same_bits(loop["sum"], want[1])
    assert np.isfinite(loop["fused"]).all() and loop["fused"].max() > 100.0


def test_fusion_with_the_registered_transform_is_as_accurate_as_with_the_true_one(ctx, mvs, loop):
    """View A aligned into B's frame and its beads detected there: the largest distance to the nearest detection of view B under the
    TRUE transform is r_ref (resampling and detection alone); under the REGISTERED transform it must stay within 2 r_ref."""
    dist = {}
    for name, m in (("true", loop["truth"]), ("registered", loop["reg"]["m"])):
        al, _ = ctx.align_views([loop["imgs"][0]], [m], (0, 0, 0), LOOP_DIM, mvs.fuse_params(blend=0.0), weights=False)
        peaks, n_found = loop["det"].detect(al[0])
        assert n_found >= LOOP_BEADS // 2
        d = np.linalg.norm(peaks["pos"][:, None] - loop["peaks"][1]["pos"][None], axis=2).min(axis=1)
        dist[name] = float(d.max())
    print(f"r_ref {dist['true']:.4f} voxel, registered {dist['registered']:.4f} voxel")
    assert dist["registered"] <= 2 * dist["true"]


def test_aligned_views_feed_the_deconvolution(ctx, mvs, loop):
    """48^3 crops of the two views aligned into one frame with their weights, the weights normalised, transformed Gaussian PSFs, two
    iterations: all on the device, finite, and equal to Context.deconvolve on the downloaded aligned arrays."""
    crop = [im[24:72, 40:88, 40:88].copy() for im in loop["imgs"]]
    shift = np.eye(4)
    shift[:3, 3] = (40, 40, 24)
    back = np.eye(4)
    back[:3, 3] = (-40, -40, -24)
    m_a = (back @ np.vstack([loop["reg"]["m"].reshape(3, 4), [0, 0, 0, 1]]) @ shift)[:3]
    mats = [m_a, R.identity()]
    ax = np.arange(9) - 4.0
    g = [np.exp(-ax * ax / (2 * s * s)) for s in (1.0, 1.0, 2.0)]
    psf = (g[2][:, None, None] * g[1][None, :, None] * g[0][None, None, :]).astype(np.float32)
    psfs = [mvs.transform_psf(psf, m, (11, 11, 11), ctx=ctx) for m in mats]
    assert R.same_bits(psfs[1][1:-1, 1:-1, 1:-1], psf) and psfs[0].sum() > 0.8 * psf.sum()
    dim, n = (48, 48, 48), 48 ** 3
    params = mvs.decon_params(iterations=2)
    with Arena(ctx) as A:
        srcs = [A.put(c) for c in crop]
        al, wt, psi = [A.out(4 * n), A.out(4 * n)], [A.out(4 * n), A.out(4 * n)], A.out(4 * n)
        ctx.align_views_dev(srcs, [dim] * 2, mats, (0, 0, 0), dim, al, wt, params=mvs.fuse_params(blend=6.0))
        got_al = [A.get(a, 4 * n, 4 * n).view(np.float32).reshape(48, 48, 48) for a in al]
        raw_wt = [A.get(w, 4 * n, 4 * n).view(np.float32).reshape(48, 48, 48) for w in wt]
        ctx.normalize_weights_dev(wt, n, 1.0)
        ctx.deconvolve_dev(al, dim, psfs, psi, weight_dptrs=wt, params=params)
        got = A.get(psi, 4 * n, 4 * n).view(np.float32).reshape(48, 48, 48)
        norm_wt = [A.get(w, 4 * n, 4 * n).view(np.float32).reshape(48, 48, 48) for w in wt]
        A.check_inputs()
    wal, wwt, _ = R.align(crop, mats, (0, 0, 0), dim, (6.0, 6.0, 6.0))
    assert all(R.same_bits(a, b) for a, b in zip(got_al + raw_wt, wal + wwt))
    assert np.isfinite(got).all() and got.max() > 0
    want = ctx.deconvolve(got_al, psfs, norm_wt, params)
    assert R.same_bits(got, want)


def test_simulate_beads_fuse(ctx, mvs, loop):
    """The simulator's own entry point does the same chain."""
    pts, _ = loop_cloud(mvs)
    sb = mvs.SimulateBeads([0, 45], 0, LOOP_BEADS, ((0, 0, 0), (127, 127, 95)), LOOP_INTERVAL, D.BEAD_SIGMA)
    sb.points = pts
    fused, regs, fused_true = sb.fuse(reference=1, detector=loop["det"], matcher=mvs.BeadRegistration(ctx=ctx))
    assert regs[1] is None and REG.same_bits(regs[0], loop["reg"])
    assert R.same_bits(fused, loop["fused"])
    assert R.same_bits(fused_true, R.fuse(loop["imgs"], [loop["truth"], R.identity()], (0, 0, 0), LOOP_DIM)[0])
