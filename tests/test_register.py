"""The bead registration on the GPU against the restatement of tests/register_reference.py, bit for bit (NaNs compared as NaNs): the
neighbours and descriptors over every tile and split edge, stride and kind of cloud, the ratio-test candidates and their order, RANSAC
and the refit with their flags, the whole call against the chained stages, and the loop closed on the device -- two rendered views
registered from their detections alone."""
import numpy as np
import pytest

from . import dog_reference as D
from . import register_reference as R
from .test_register_host import LOOP_BEADS, LOOP_INTERVAL, loop_cloud, planted, rotated_cloud, true_pairs

pytestmark = pytest.mark.gpu
F64 = np.float64
GUARD = 0xAB
PAD = 64                                                   # guard bytes behind every output


# ---- device helpers ---------------------------------------------------------------------------------------------------------------------
class Arena:
    """Device buffers of one test case: inputs that must come back unchanged, outputs with guard bytes behind them."""

    def __init__(self, ctx):
        self.ctx, self.ptrs, self.inputs = ctx, [], []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.ctx.dev_free(p)

    def put(self, array):
        raw = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
        ptr = self.ctx.dev_alloc(max(len(raw), 8))
        self.ptrs.append(ptr)
        if len(raw):
            self.ctx.upload(ptr, raw)
        self.inputs.append((ptr, raw.copy()))
        return ptr

    def out(self, nbytes):
        ptr = self.ctx.dev_alloc(nbytes + PAD)
        self.ptrs.append(ptr)
        self.ctx.upload(ptr, np.full(nbytes + PAD, GUARD, np.uint8))
        return ptr

    def get(self, ptr, nbytes, written):
        """The first `written` bytes of an output of nbytes; everything behind them must still be guard bytes."""
        raw = self.ctx.download(ptr, (nbytes + PAD,), np.uint8)
        assert np.all(raw[written:] == GUARD), "written past the end of an output"
        return raw[:written].copy()

    def check_inputs(self):
        for ptr, raw in self.inputs:
            if len(raw):
                assert np.array_equal(self.ctx.download(ptr, (len(raw),), np.uint8), raw), "an input was written"


def as_list(pos, stride):
    """A point list at byte stride 24 (packed) or 40 (mvsim_peak records, pos first, the rest junk that must not matter)."""
    pos = np.asarray(pos, F64).reshape(-1, 3)
    if stride == 24:
        return pos.copy()
    rec = np.zeros(len(pos), D.PEAK_DTYPE)
    rec["pos"], rec["value"], rec["flags"], rec["voxel"] = pos, 1e30, -1, np.arange(len(pos)) * 7919
    return rec


def count_ptr(arena, n):
    return arena.put(np.array([n], np.int64))


def run_neighbours(ctx, pos, redundancy, stride=24, spare=0):
    """k_knn + k_descriptors through the C ABI with capacity = n + spare and n read from the device: (idx, d2, desc, n_described)."""
    pos = np.asarray(pos, F64).reshape(-1, 3)
    n, K = len(pos), 3 + redundancy
    S, cap = len(R.subsets(K)), max(1, len(pos) + spare)
    with Arena(ctx) as A:
        lst, cnt = A.put(as_list(pos, stride)) if n else A.put(np.zeros(5)), count_ptr(A, n)
        idx, d2, desc, nd = A.out(4 * K * cap), A.out(8 * K * cap), A.out(48 * S * cap), A.out(8)
        ctx.knn_dev(lst, stride, cnt, cap, redundancy, idx, d2)
        ctx.bead_descriptors_dev(lst, stride, cnt, cap, redundancy, idx, desc, nd)
        got = (A.get(idx, 4 * K * cap, 4 * K * n).view(np.int32).reshape(n, K), A.get(d2, 8 * K * cap, 8 * K * n).view(F64).reshape(n, K),
               A.get(desc, 48 * S * cap, 48 * S * n).view(F64).reshape(n, S, 6), int(A.get(nd, 8, 8).view(np.int64)[0]))
        A.check_inputs()
    return got


def check_neighbours(ctx, pos, redundancy, stride=24, spare=0):
    idx, d2, desc, nd = run_neighbours(ctx, pos, redundancy, stride, spare)
    want_idx, want_d2 = R.knn(pos, 3 + redundancy)
    assert np.array_equal(idx, want_idx), "neighbour indices"
    assert R.same_bits(d2, want_d2), "neighbour distances"
    want = R.descriptors(pos, want_idx)
    assert R.same_bits(desc, want), "descriptors"
    assert nd == int(R.described(want).sum())
    return desc


def run_match(ctx, desc_a, desc_b, redundancy, ratio, capacity, spare=0):
    """(the candidates written, n_candidates)"""
    na, nb = len(desc_a), len(desc_b)
    ca, cb = max(1, na + spare), max(1, nb + spare)
    with Arena(ctx) as A:
        da, db = A.put(desc_a if na else np.zeros(6)), A.put(desc_b if nb else np.zeros(6))
        out, cnt = A.out(24 * capacity), A.out(8)
        ctx.match_descriptors_dev(da, count_ptr(A, na), ca, db, count_ptr(A, nb), cb, redundancy, ratio, capacity, out, cnt)
        total = int(A.get(cnt, 8, 8).view(np.int64)[0])
        got = A.get(out, 24 * capacity, 24 * min(total, capacity)).view(R.MATCH_DTYPE)
        A.check_inputs()
    return got, total


def check_match(ctx, desc_a, desc_b, redundancy, ratio=3.0, capacity=None, spare=0, want=None):
    want = R.match(desc_a, desc_b, ratio) if want is None else want
    cap = max(1, len(want)) if capacity is None else capacity
    got, total = run_match(ctx, desc_a, desc_b, redundancy, ratio, cap, spare)
    assert total == len(want)
    assert R.same_bits(got, want[:cap]), "candidates"
    return want


def run_ransac(ctx, mvs, pa, pb, cand, p, capacity=None, stride_a=24, stride_b=40, with_mask=True, n_candidates=None):
    pa, pb = np.asarray(pa, F64).reshape(-1, 3), np.asarray(pb, F64).reshape(-1, 3)
    cap = max(1, len(cand)) if capacity is None else capacity
    total = len(cand) if n_candidates is None else n_candidates
    M = min(max(total, 0), cap)
    with Arena(ctx) as A:
        la, lb = A.put(as_list(pa, stride_a)) if len(pa) else A.put(np.zeros(5)), A.put(as_list(pb, stride_b)) if len(pb) else A.put(np.zeros(5))
        cd = A.put(cand) if len(cand) else A.put(np.zeros(1, R.MATCH_DTYPE))
        res, mask = A.out(160), A.out(cap)
        ctx.ransac_affine_dev(la, stride_a, count_ptr(A, len(pa)), max(1, len(pa)), lb, stride_b, count_ptr(A, len(pb)), max(1, len(pb)), cd,
                              count_ptr(A, total), cap, res, mask if with_mask else 0, mvs.match_params(**p))
        got = A.get(res, 160, 160).view(R.REGISTRATION_DTYPE)[0]
        got_mask = A.get(mask, cap, M if with_mask else 0)
        A.check_inputs()
    return got, got_mask


def check_ransac(ctx, mvs, pa, pb, cand, capacity=None, **kw):
    p = R.params(**kw)
    want, want_mask = R.ransac_refit(pa, pb, cand, p, capacity=capacity)
    got, mask = run_ransac(ctx, mvs, pa, pb, cand, p, capacity)
    assert R.same_bits(got, want), (got, want)
    assert np.array_equal(mask, want_mask), "inlier mask"
    return want, want_mask


# ---- clouds -----------------------------------------------------------------------------------------------------------------------------
def cloud(kind, n, seed=0):
    rng = np.random.default_rng(1000 * seed + n)
    if kind == "random":
        return rng.uniform(0, 200, (n, 3))
    if kind == "lattice":                                  # many equal distances: the index decides
        side = int(np.ceil(n ** (1 / 3)))
        g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(F64)
        return g[rng.permutation(len(g))[:n]]
    if kind == "duplicates":                               # every point up to four times
        base = rng.uniform(0, 50, (max(1, n // 3), 3))
        return base[rng.integers(0, len(base), n)]
    pts = rng.uniform(0, 200, (n, 3))                      # "nonfinite": NaN and +-inf planted in single coordinates
    bad = rng.permutation(n)[:max(1, n // 6)]
    pts[bad, rng.integers(0, 3, len(bad))] = rng.choice([np.nan, np.inf, -np.inf], len(bad))
    return pts


def split_edges(mvs):
    """List sizes one below, at and one above the tile of k_knn, and around the first size at which a split takes two tiles."""
    g = mvs.match_geometry(1)
    tile = g["knn_tile"]
    first = next(n for n in range(1, 8192) if mvs.match_geometry(n)["knn_tiles_per_split"] > 1)
    return sorted({tile - 1, tile, tile + 1, 2 * tile + 1, first - 2, first - 1, first})


FIXED_SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000]


@pytest.mark.parametrize("n", FIXED_SIZES)
def test_neighbours_and_descriptors_equal_the_restatement(ctx, n):
    pos = cloud("random", n)
    for r in (0, 1, 2):
        for stride in (24, 40):
            check_neighbours(ctx, pos, r, stride)


def test_neighbours_at_tile_and_split_edges(ctx, mvs):
    edges = split_edges(mvs)
    print("edge sizes:", edges)
    assert len(edges) >= 6 and max(edges) > 1024
    for n in edges:
        check_neighbours(ctx, cloud("random", n, seed=1), 1, 40 if n % 2 else 24)
    big = max(edges)
    check_neighbours(ctx, cloud("lattice", big), 2)
    check_neighbours(ctx, cloud("random", big, seed=2), 0)


@pytest.mark.parametrize("kind", ["lattice", "duplicates", "nonfinite"])
def test_ties_duplicates_and_non_finite_points(ctx, kind):
    for n in (5, 6, 65, 257, 1000):
        pos = cloud(kind, n)
        for r in (0, 1, 2):
            check_neighbours(ctx, pos, r, 40 if r == 1 else 24)
    if kind == "nonfinite":                                # nothing but non-finite points; one finite point among them
        pos = np.full((70, 3), np.nan)
        check_neighbours(ctx, pos, 1)
        pos[33] = (1.0, 2.0, 3.0)
        check_neighbours(ctx, pos, 0)


def test_count_is_read_from_the_device_below_the_capacity(ctx):
    for n, spare in ((0, 4), (3, 1), (64, 1), (65, 200), (300, 1000), (1000, 3000)):
        pos = cloud("random", n, seed=3)
        check_neighbours(ctx, pos, 1, 40, spare)
        check_neighbours(ctx, pos, 2, 24, spare)


# ---- matching ---------------------------------------------------------------------------------------------------------------------------
def described_pair(r, n, box, seed):
    A, B, perm = rotated_cloud(seed=seed, n=n, box=box)
    K = 3 + r
    return R.descriptors(A, R.knn(A, K)[0]), R.descriptors(B, R.knn(B, K)[0]), perm


@pytest.mark.parametrize("n,box", [(60, (128, 128, 96)), (300, (256, 256, 128)), (1000, (512, 512, 200))], ids=["60", "300", "1000"])
@pytest.mark.parametrize("r", [0, 1, 2])
def test_candidates_of_rotated_shuffled_cropped_copies(ctx, r, n, box):
    da, db, perm = described_pair(r, n, box, seed=4)
    want = check_match(ctx, da, db, r)
    true = true_pairs(want, perm)
    print(f"{len(da)} x {len(db)} points, redundancy {r}: {len(want)} candidates, {int(true.sum())} true")
    assert len(want) >= 8 and true.sum() >= 0.9 * len(want)
    # fewer records than candidates; a capacity above both counts; another ratio
    check_match(ctx, da, db, r, capacity=max(1, len(want) // 2), want=want)
    if n <= 300:
        check_match(ctx, da, db, r, spare=777, want=want)
        check_match(ctx, da, db, r, ratio=1.0)
        check_match(ctx, da, db, r, ratio=10.0)


def test_lists_that_yield_no_candidates(ctx):
    da, db, _ = described_pair(1, 60, (128, 128, 96), seed=4)
    assert len(check_match(ctx, da, db[:1], 1)) == 0       # one described point of B: no second best
    lone = np.full_like(db, np.nan)
    lone[7] = db[7]
    assert len(check_match(ctx, da, lone, 1)) == 0
    assert len(check_match(ctx, da, np.full_like(db, np.nan), 1)) == 0
    assert len(check_match(ctx, np.full_like(da, np.nan), db, 1)) == 0
    assert len(check_match(ctx, da[:0], db, 1)) == 0 and len(check_match(ctx, da, db[:0], 1)) == 0
    # two identical clusters in B: v1 == v2 for every point of A
    rng = np.random.default_rng(8)
    A = rng.integers(0, 60 * 1024, (40, 3)) / 1024.0                   # multiples of 2^-10: the shift below is exact in fp64,
    B = np.concatenate([A, A + np.array([1024.0, 0.0, 0.0])])          # so both clusters give the same bits
    for r in (0, 1, 2):
        K = 3 + r
        da, db = R.descriptors(A, R.knn(A, K)[0]), R.descriptors(B, R.knn(B, K)[0])
        want = check_match(ctx, da, db, r)
        assert len(want) == 0
        assert len(check_match(ctx, da, db[:40], r)) == 40             # one cluster alone: every point finds itself at v = 0


# ---- RANSAC and refit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [0, 3, 4, 5, 255, 256, 257, 2000])
def test_ransac_over_caller_supplied_candidates(ctx, mvs, M):
    pa, pb, cand, inlier, _ = planted(np.random.default_rng(M), M, 0.3)
    want, mask = check_ransac(ctx, mvs, pa, pb, cand, hypotheses=200, max_epsilon=1.0)
    print(f"M = {M}: {want['n_inliers']} inliers, best {want['best_hypothesis']}, refits {want['refits']}, flags {want['flags']}")
    if M < 4:
        assert want["flags"] == R.FEW_CANDIDATES | R.NO_MODEL | R.FEW_INLIERS and np.all(np.isnan(want["m"]))
    if M >= 255:
        assert want["flags"] == 0 and np.array_equal(mask.astype(bool), inlier)


@pytest.mark.parametrize("share", [0.0, 0.7])
def test_ransac_outlier_shares_and_seeds(ctx, mvs, share):
    for M, seed in ((257, 0), (600, 123456789012), (600, -77)):
        pa, pb, cand, inlier, _ = planted(np.random.default_rng(M + int(10 * share)), M, share)
        want, mask = check_ransac(ctx, mvs, pa, pb, cand, hypotheses=600, max_epsilon=1.0, seed=seed)
        assert want["flags"] == 0 and np.array_equal(mask.astype(bool), inlier), (M, seed, want)


@pytest.mark.parametrize("hypotheses", [1, 63, 64, 65, 10000])
def test_ransac_hypothesis_counts(ctx, mvs, hypotheses):
    pa, pb, cand, _, _ = planted(np.random.default_rng(17), 300, 0.3)
    want, _ = check_ransac(ctx, mvs, pa, pb, cand, hypotheses=hypotheses, max_epsilon=1.0)
    assert 0 <= want["best_hypothesis"] < hypotheses or want["flags"] & R.NO_MODEL


def test_ransac_flags(ctx, mvs):
    rng = np.random.default_rng(1)
    pa, pb, cand, _, _ = planted(rng, 300, 0.3, noise=0.5)
    full, _ = check_ransac(ctx, mvs, pa, pb, cand, hypotheses=64, max_epsilon=1.0, seed=3)
    assert full["refits"] >= 2 and full["flags"] == 0, "the case must need more than one refit round"
    for cap in (0, 1):
        want, _ = check_ransac(ctx, mvs, pa, pb, cand, hypotheses=64, max_epsilon=1.0, seed=3, max_refits=cap)
        assert want["flags"] == R.CAPPED and want["refits"] == cap
    want, _ = check_ransac(ctx, mvs, pa, pb, cand, hypotheses=64, max_epsilon=1.0, seed=3, min_inliers=int(full["n_inliers"]) + 1)
    assert want["flags"] == R.FEW_INLIERS
    want, _ = check_ransac(ctx, mvs, pa, pb, cand, hypotheses=64, max_epsilon=1.0, seed=3, min_inlier_ratio=0.9)
    assert want["flags"] == R.FEW_INLIERS
    # coplanar candidates: no hypothesis has a model
    flat = pa.copy()
    flat[:, 2] = 5.0
    want, mask = check_ransac(ctx, mvs, flat, pb, cand, hypotheses=64)
    assert want["flags"] == R.NO_MODEL | R.FEW_INLIERS and want["best_hypothesis"] == -1 and not mask.any()
    # fewer records than candidates; indices that are no points of their lists; no mask asked for
    check_ransac(ctx, mvs, pa, pb, cand, capacity=100, hypotheses=64, max_epsilon=1.0)
    odd = cand.copy()
    odd["a"][::7], odd["b"][3::11] = -1, 300
    want, mask = check_ransac(ctx, mvs, pa, pb, odd, hypotheses=64, max_epsilon=1.0)
    assert not mask[::7].any() and not mask[3::11].any() and want["n_inliers"] > 50
    p = R.params(hypotheses=64, max_epsilon=1.0)
    got, none = run_ransac(ctx, mvs, pa, pb, cand, p, with_mask=False)
    assert R.same_bits(got, R.ransac_refit(pa, pb, cand, p)[0]) and len(none) == 0


# ---- chaining and repeatability ---------------------------------------------------------------------------------------------------------
def whole_dev(ctx, mvs, A_pos, B_pos, p, stride_a=40, stride_b=24, spare=5):
    with Arena(ctx) as A:
        la, lb = A.put(as_list(A_pos, stride_a)), A.put(as_list(B_pos, stride_b))
        ca, cb = len(A_pos) + spare, len(B_pos) + spare
        got = ctx.register_beads_dev(la, stride_a, count_ptr(A, len(A_pos)), ca, lb, stride_b, count_ptr(A, len(B_pos)), cb,
                                     params=mvs.match_params(**p))
        A.check_inputs()
    return got


def same_result(got, want):
    return R.same_bits(got[0], want[0]) and R.same_bits(got[1], want[1]) and np.array_equal(got[2], want[2])


@pytest.mark.parametrize("r", [0, 1, 2])
def test_whole_call_equals_the_stages_the_host_entry_and_itself(ctx, mvs, r):
    A_pos, B_pos, perm = rotated_cloud(seed=6, n=300, box=(256, 256, 128))
    p = R.params(redundancy=r, max_epsilon=1.0, hypotheses=300)
    ref = R.register(A_pos, B_pos, p)
    want = (ref["result"], ref["candidates"], ref["mask"])
    print(f"redundancy {r}: {len(want[1])} candidates, {want[0]['n_inliers']} inliers, flags {want[0]['flags']}")
    assert want[0]["flags"] == 0 and np.all(true_pairs(want[1], perm)[want[2].astype(bool)])
    first = whole_dev(ctx, mvs, A_pos, B_pos, p)
    assert same_result(first, want), "the whole call against the restatement"
    # the stages chained through the C ABI
    desc_a, desc_b = check_neighbours(ctx, A_pos, r, 40), check_neighbours(ctx, B_pos, r, 24)
    cand = check_match(ctx, desc_a, desc_b, r, p["ratio"], capacity=len(A_pos))
    res, mask = run_ransac(ctx, mvs, A_pos, B_pos, cand, p, capacity=len(A_pos))
    res["n_a"], res["n_b"] = first[0]["n_a"], first[0]["n_b"]            # the stage alone sees no descriptors
    assert same_result((res, cand, mask), first), "the stages chained against the whole call"
    # the host entry, with both kinds of list; a second call; a call after the caches were released
    assert same_result(ctx.register_beads(as_list(A_pos, 40), B_pos, mvs.match_params(**p)), first)
    assert same_result(mvs.BeadRegistration(ctx=ctx, **p).register(A_pos, as_list(B_pos, 40)), first)
    assert same_result(whole_dev(ctx, mvs, A_pos, B_pos, p, 24, 40, spare=0), first)
    ctx.release_caches()
    assert same_result(whole_dev(ctx, mvs, A_pos, B_pos, p), first)


def test_host_entry_with_short_and_empty_lists(ctx, mvs):
    some = cloud("random", 30)
    for a, b in ((some[:0], some), (some, some[:0]), (some[:3], some), (some, some[:1])):
        res, cand, mask = ctx.register_beads(a, b)
        want = R.register(a, b, R.params())
        assert R.same_bits(res, want["result"]) and len(cand) == len(mask) == 0
        assert res["flags"] == R.FEW_CANDIDATES | R.NO_MODEL | R.FEW_INLIERS
    views = mvs.BeadRegistration(ctx=ctx, max_epsilon=1.0).register_views([some, some + 3.0, some[::-1] * 1.0], fixed=1)
    assert views[1] is None and views[0][0]["flags"] == 0 and views[2][0]["flags"] == 0
    assert np.abs(views[0][0]["m"].reshape(3, 4) - np.hstack([np.eye(3), np.full((3, 1), 3.0)])).max() < 1e-9


# ---- the closed loop --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u16", [False, True], ids=["float", "uint16"])
def test_rendered_views_register_from_their_detections(ctx, mvs, u16):
    """The cloud of tests/test_register_host.py (its seed is recorded there) under the identity and 45 degrees about x: rendered,
    detected and registered on the device with nothing downloaded in between.  Every inlier is a true pair; the result is the
    restatement's over the downloaded detections; and the registration's own transform maps the true positions of A onto those of B
    within twice what the least-squares fit over the truth-paired detections does."""
    pts, mats = loop_cloud(mvs)
    truth = [mvs.beads.apply_affine(m, pts) for m in mats]
    sigma, dim = D.BEAD_SIGMA, (128, 128, 96)
    det = mvs.DifferenceOfGaussian(threshold=5.0, ctx=ctx, capacity=256)
    p = R.params()
    item, cap = D.PEAK_DTYPE.itemsize, det.capacity
    img = ctx.dev_alloc(dim[0] * dim[1] * dim[2] * (2 if u16 else 4))
    lists = ctx.dev_alloc(2 * (cap * item + 8))
    out = ctx.dev_alloc(256 + 25 * cap)
    try:
        pk = [lists, lists + cap * item + 8]
        for m, at in zip(mats, pk):
            ctx.render_beads_dev(pts, LOOP_INTERVAL, sigma, None if u16 else [img], [img] if u16 else None, matrices=np.asarray(m)[None])
            ctx.detect_beads_dev(img, np.uint16 if u16 else np.float32, dim, cap, at, at + cap * item, params=det.params)
        ctx.register_beads_dev(pk[0], item, pk[0] + cap * item, cap, pk[1], item, pk[1] + cap * item, cap, out, out + 256, out + 256 + 24 * cap,
                               params=mvs.match_params(**p))
        res = ctx.download(out, (1,), R.REGISTRATION_DTYPE)[0]
        found = [int(ctx.download(at + cap * item, (1,), np.int64)[0]) for at in pk]
        peaks = [ctx.download(at, (n,), D.PEAK_DTYPE) for at, n in zip(pk, found)]
        listed = int(res["n_candidates"])
        cand = ctx.download(out + 256, (listed,), R.MATCH_DTYPE)
        mask = ctx.download(out + 256 + 24 * cap, (listed,), np.uint8)
    finally:
        for ptr in (img, lists, out):
            ctx.dev_free(ptr)
    assert found == [LOOP_BEADS, LOOP_BEADS]
    # which bead a detection is: the true position within 0.5 voxel
    bead = []
    for t, pkv in zip(truth, peaks):
        d = np.linalg.norm(pkv["pos"][:, None] - t[None], axis=2)
        assert np.all(d.min(axis=1) <= 0.5)
        bead.append(np.argmin(d, axis=1))
    inl = mask.astype(bool)
    assert res["flags"] == 0 and res["n_inliers"] >= p["min_inliers"] and res["n_inliers"] == inl.sum()
    assert np.all(bead[0][cand["a"][inl]] == bead[1][cand["b"][inl]]), "an inlier is no true pair"
    want = R.register(peaks[0]["pos"], peaks[1]["pos"], p)
    assert R.same_bits(res, want["result"]) and R.same_bits(cand, want["candidates"]) and np.array_equal(mask, want["mask"])
    # accuracy against the fit that knows the truth
    order = [np.argsort(b) for b in bead]                   # detection of bead i, per view
    src = np.hstack([peaks[0]["pos"][order[0]], np.ones((LOOP_BEADS, 1))])
    fit, *_ = np.linalg.lstsq(src, peaks[1]["pos"][order[1]], rcond=None)
    r_ref = np.linalg.norm(np.hstack([truth[0], np.ones((LOOP_BEADS, 1))]) @ fit - truth[1], axis=1).max()
    r_reg = np.linalg.norm(R.apply(res["m"], truth[0]) - truth[1], axis=1).max()
    print(f"{'uint16' if u16 else 'float'}: {listed} candidates, {int(inl.sum())} inliers, mean inlier error {res['mean_error']:.4f}; "
          f"r_ref {r_ref:.4f}, registration {r_reg:.4f} voxel")
    assert r_reg <= 2 * r_ref
    # the simulator's own entry point does the same
    sb = mvs.SimulateBeads([0, 45], 0, LOOP_BEADS, ((0, 0, 0), (127, 127, 95)), LOOP_INTERVAL, sigma)
    sb.points = pts
    res2, cand2, mask2, true_m = sb.register(0, 1, det, mvs.BeadRegistration(ctx=ctx), u16)
    assert R.same_bits(res2, res) and R.same_bits(cand2, cand) and np.array_equal(mask2, mask)
    assert np.abs(R.apply(true_m, truth[0]) - truth[1]).max() < 1e-9
    assert np.abs(res["m"].reshape(3, 4) - true_m)[:, :3].max() < 0.01
