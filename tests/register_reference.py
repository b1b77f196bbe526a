"""The bead registration restated in numpy, literally as include/mvsim.h states it: fp64 throughout, every + - * / sqrt an operation of
its own, sums in the stated order (np.add.accumulate adds left to right), orders as (value, index) through stable sorts.  The all-pairs
steps run in chunks so that a thousand points stay within a few hundred MB.  Not a fast implementation -- the yardstick the GPU kernels
and mvsim_fit_affine are held to, bit for bit."""
import itertools

import numpy as np

FIT_CHUNK, MAX_DRAWS, MAX_POINTS = 256, 32, 65536
FEW_CANDIDATES, NO_MODEL, CAPPED, FEW_INLIERS = 1, 2, 4, 8
MATCH_DTYPE = np.dtype([("a", np.int32), ("b", np.int32), ("v_best", np.float64), ("v_second", np.float64)])
REGISTRATION_DTYPE = np.dtype([("m", np.float64, (12,)), ("mean_error", np.float64), ("max_error", np.float64), ("n_a", np.int64),
                               ("n_b", np.int64), ("n_candidates", np.int64), ("n_inliers", np.int64), ("best_hypothesis", np.int64),
                               ("refits", np.int32), ("flags", np.int32)])
DEFAULTS = dict(ratio=3.0, max_epsilon=5.0, min_inlier_ratio=0.1, seed=0, redundancy=1, hypotheses=10000, max_refits=8, min_inliers=12)
F64 = np.float64


def params(**kw):
    p = dict(DEFAULTS)
    assert set(kw) <= set(p), kw
    p.update(kw)
    return p


def same_bits(a, b):
    """Equal bit for bit, except that any NaN equals any NaN; structured arrays field by field."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.names:
        return all(same_bits(a[n], b[n]) for n in a.dtype.names)
    if a.dtype == F64:
        return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


def d2(a, b):
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


# ---- step 1 ------------------------------------------------------------------------------------------------------------------------------
def knn(pos, K, chunk=512):
    """(idx (n, K) int32, d2 (n, K)): the K other finite points with the smallest (d2, index); missing ranks -1 and +inf."""
    pos = np.asarray(pos, F64).reshape(-1, 3)
    n = len(pos)
    finite = np.isfinite(pos).all(axis=1)
    idx = np.full((n, K), -1, np.int32)
    dd = np.full((n, K), np.inf, F64)
    take = min(K, n)
    with np.errstate(all="ignore"):
        for q0 in range(0, n, chunk):
            q = np.arange(q0, min(n, q0 + chunk))
            D = d2(pos[q, None, :], pos[None, :, :])
            out = ~finite[None, :] | ~finite[q, None] | (q[:, None] == np.arange(n)[None, :])
            order = np.lexsort((D, out), axis=-1)[:, :take]              # excluded last, then d2, ties by index (the sort is stable)
            rows = np.arange(len(q))[:, None]
            ok = ~out[rows, order]
            idx[q, :take] = np.where(ok, order, -1)
            dd[q, :take] = np.where(ok, D[rows, order], np.inf)
    return idx, dd


# ---- step 2 ------------------------------------------------------------------------------------------------------------------------------
def subsets(K):
    return np.array(list(itertools.combinations(range(K), 3)), np.int32)


def descriptors(pos, idx):
    """(n, S, 6): |pa| |pb| |pc| |ab| |ac| |bc| per rank triple; NaN for a point with a missing rank."""
    pos = np.asarray(pos, F64).reshape(-1, 3)
    K = idx.shape[1]
    trip = subsets(K)
    out = np.full((len(pos), len(trip), 6), np.nan, F64)
    has = np.nonzero((idx >= 0).all(axis=1))[0]
    with np.errstate(all="ignore"):
        p = pos[has]
        for s, (i, j, k) in enumerate(trip):
            a, b, c = pos[idx[has, i]], pos[idx[has, j]], pos[idx[has, k]]
            for t, (u, w) in enumerate(((p, a), (p, b), (p, c), (a, b), (a, c), (b, c))):
                out[has, s, t] = np.sqrt(d2(u, w))
    return out


def described(desc):
    return ~np.isnan(desc[:, 0, 0])


# ---- step 3 ------------------------------------------------------------------------------------------------------------------------------
def match(desc_a, desc_b, ratio, budget=1 << 24):
    """(all candidates in ascending a, as MATCH_DTYPE)."""
    S = desc_a.shape[1]
    ratio2 = F64(ratio) * F64(ratio)
    ia, ib = np.nonzero(described(desc_a))[0], np.nonzero(described(desc_b))[0]
    out = []
    if len(ib) < 2:
        return np.zeros(0, MATCH_DTYPE)
    B = desc_b[ib]
    chunk = max(1, budget // (len(ib) * S * S * 6))
    with np.errstate(all="ignore"):
        for c0 in range(0, len(ia), chunk):
            rows = ia[c0:c0 + chunk]
            e = desc_a[rows][:, :, None, None, :] - B[None, None, :, :, :]          # (c, S, nb, S, 6)
            e = e * e
            dist = ((((e[..., 0] + e[..., 1]) + e[..., 2]) + e[..., 3]) + e[..., 4]) + e[..., 5]
            v = np.where(np.isnan(dist), np.inf, dist).min(axis=(1, 3))              # (c, nb)
            order = np.argsort(v, axis=1, kind="stable")[:, :2]                      # (v, index): ib is ascending
            r = np.arange(len(rows))
            v1, v2 = v[r, order[:, 0]], v[r, order[:, 1]]
            yes = v1 * ratio2 < v2
            rec = np.zeros(int(yes.sum()), MATCH_DTYPE)
            rec["a"], rec["b"], rec["v_best"], rec["v_second"] = rows[yes], ib[order[yes, 0]], v1[yes], v2[yes]
            out.append(rec)
    return np.concatenate(out) if out else np.zeros(0, MATCH_DTYPE)


# ---- step 4 ------------------------------------------------------------------------------------------------------------------------------
def _ordered_sum(x):
    """x: (..., chunks, slots) with +0.0 where a candidate is not selected.  A chunk's sum starts from +0.0 and adds ascending, the total
    starts from +0.0 and adds the chunks' sums ascending.  (A running sum that started from +0.0 is never -0.0, so adding the +0.0 of a
    skipped candidate changes no bit; the + 0.0 behind each accumulate is the start value, which matters for a lone -0.0 only.)"""
    if x.shape[-1] == 0 or x.shape[-2] == 0:
        return np.zeros(x.shape[:-2], F64)
    per_chunk = np.add.accumulate(x, axis=-1)[..., -1] + 0.0
    return np.add.accumulate(per_chunk, axis=-1)[..., -1] + 0.0


def _fit_grid(pq, sel):
    """pq (..., chunks, slots, 6), sel (..., chunks, slots) -> (m (..., 12), has_model (...))."""
    with np.errstate(all="ignore"):
        n = sel.sum(axis=(-1, -2))
        dn = n.astype(F64)
        cen = np.stack([_ordered_sum(np.where(sel, pq[..., t], 0.0)) / dn for t in range(6)], axis=-1)
        c = cen[..., None, None, :]
        px, py, pz = pq[..., 0] - c[..., 0], pq[..., 1] - c[..., 1], pq[..., 2] - c[..., 2]
        qx, qy, qz = pq[..., 3] - c[..., 3], pq[..., 4] - c[..., 4], pq[..., 5] - c[..., 5]
        prods = [px * px, px * py, px * pz, py * py, py * pz, pz * pz,
                 qx * px, qx * py, qx * pz, qy * px, qy * py, qy * pz, qz * px, qz * py, qz * pz]
        mom = [_ordered_sum(np.where(sel, v, 0.0)) for v in prods]
        m00, m01, m02, m11, m12, m22 = mom[:6]
        m10, m20, m21 = m01, m02, m12
        det = m00 * m11 * m22 + m01 * m12 * m20 + m02 * m10 * m21 - m02 * m11 * m20 - m00 * m12 * m21 - m01 * m10 * m22
        idet = 1.0 / det
        inv = [[(m11 * m22 - m12 * m21) * idet, (m02 * m21 - m01 * m22) * idet, (m01 * m12 - m02 * m11) * idet],
               [(m12 * m20 - m10 * m22) * idet, (m00 * m22 - m02 * m20) * idet, (m02 * m10 - m00 * m12) * idet],
               [(m10 * m21 - m11 * m20) * idet, (m01 * m20 - m00 * m21) * idet, (m00 * m11 - m01 * m10) * idet]]
        rows = []
        for r in range(3):
            cr = mom[6 + 3 * r:9 + 3 * r]
            a = [(cr[0] * inv[0][k] + cr[1] * inv[1][k]) + cr[2] * inv[2][k] for k in range(3)]
            t = cen[..., 3 + r] - ((a[0] * cen[..., 0] + a[1] * cen[..., 1]) + a[2] * cen[..., 2])
            rows += a + [t]
        has = (n >= 4) & (det != 0.0) & np.isfinite(det)
    return np.stack(rows, axis=-1), has


def fit_affine(p, q, mask=None):
    """Step 4 over pairs p[i] -> q[i] selected by mask: the 12 doubles of the model, or None."""
    p, q = np.asarray(p, F64).reshape(-1, 3), np.asarray(q, F64).reshape(-1, 3)
    n = len(p)
    sel = np.ones(n, bool) if mask is None else np.asarray(mask).astype(bool)
    chunks = max(1, -(-n // FIT_CHUNK))
    pq = np.zeros((chunks * FIT_CHUNK, 6), F64)
    pq[:n, :3], pq[:n, 3:] = p, q
    s = np.zeros(chunks * FIT_CHUNK, bool)
    s[:n] = sel
    m, has = _fit_grid(pq.reshape(chunks, FIT_CHUNK, 6), s.reshape(chunks, FIT_CHUNK))
    return m if has else None


def residual2(m, pq):
    """e2 of pairs pq (M, 6) under models m (..., 12): (..., M)."""
    m = np.asarray(m, F64)[..., None, :]
    with np.errstate(all="ignore"):
        e = [(((m[..., 4 * r] * pq[:, 0] + m[..., 4 * r + 1] * pq[:, 1]) + m[..., 4 * r + 2] * pq[:, 2]) + m[..., 4 * r + 3]) - pq[:, 3 + r]
             for r in range(3)]
        return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]


# ---- step 5 ------------------------------------------------------------------------------------------------------------------------------
_JR_A, _JR_C, _JR_MASK = np.uint64(0x5DEECE66D), np.uint64(0xB), np.uint64((1 << 48) - 1)


def _next31(state, active):
    """java.util.Random.next(31) of the generators in `active`, which advance; the others stand still."""
    with np.errstate(over="ignore"):
        state[active] = (state[active] * _JR_A + _JR_C) & _JR_MASK
    return (state >> np.uint64(17)).astype(np.int64)


def _next_int(state, bound, active):
    """nextInt(bound) of the JDK specification for the generators in `active`."""
    r = _next31(state, active)
    if bound & (bound - 1) == 0:
        return (bound * r) >> 31
    u = r.copy()
    while True:
        r = u % bound
        again = active & (u - r + (bound - 1) >= (1 << 31))       # the int overflow of the JDK's loop condition
        if not again.any():
            return r
        u = np.where(again, _next31(state, again), u)


def draw4(seed, h, M):
    """Hypotheses h (array) over M candidates: (idx (H, 4) sorted ascending, void (H,))."""
    h = np.asarray(h, np.int64)
    with np.errstate(over="ignore"):
        s = (np.int64(seed) + h).astype(np.uint64)                # wraps as a Java long does
    state = (s ^ _JR_A) & _JR_MASK
    idx = np.full((len(h), 4), -1, np.int64)
    have = np.zeros(len(h), np.int64)
    for _ in range(MAX_DRAWS):
        active = have < 4
        if not active.any():
            break
        v = _next_int(state, int(M), active)
        fresh = active & (idx != v[:, None]).all(axis=1)
        idx[fresh, have[fresh]] = v[fresh]
        have[fresh] += 1
    return np.sort(idx, axis=1), have < 4


def hypothesis_models(pq, seed, h):
    """The models of hypotheses h over the gathered pairs pq (M, 6): (m (H, 12), has_model (H,))."""
    M = len(pq)
    idx, void = draw4(seed, h, M)
    idx = np.where(void[:, None], 0, idx)
    chunk = idx // FIT_CHUNK
    rank = np.concatenate([np.zeros((len(idx), 1), np.int64), np.cumsum(chunk[:, 1:] != chunk[:, :-1], axis=1)], axis=1)
    grid = np.zeros((len(idx), 4, 4, 6), F64)                     # [chunk in order of appearance][sample]: the same association of sums
    sel = np.zeros((len(idx), 4, 4), bool)
    rows = np.arange(len(idx))
    for k in range(4):
        grid[rows, rank[:, k], k] = pq[idx[:, k]]
        sel[rows, rank[:, k], k] = True
    m, has = _fit_grid(grid, sel)
    return m, has & ~void


def gather(pos_a, pos_b, cand):
    pos_a, pos_b = np.asarray(pos_a, F64).reshape(-1, 3), np.asarray(pos_b, F64).reshape(-1, 3)
    a, b = cand["a"].astype(np.int64), cand["b"].astype(np.int64)
    ok = (a >= 0) & (a < len(pos_a)) & (b >= 0) & (b < len(pos_b))
    pq = np.full((len(cand), 6), np.nan, F64)
    pq[ok, :3], pq[ok, 3:] = pos_a[a[ok]], pos_b[b[ok]]
    return pq


def ransac(pq, p, block=256):
    """(best hypothesis, its count) -- the highest count, ties to the lowest h; (-1, 0) when no hypothesis counts anything."""
    eps2 = F64(p["max_epsilon"]) * F64(p["max_epsilon"])
    best_h, best_c = -1, 0
    for h0 in range(0, p["hypotheses"], block):
        h = np.arange(h0, min(p["hypotheses"], h0 + block))
        m, has = hypothesis_models(pq, p["seed"], h)
        count = np.where(has, (residual2(m, pq) <= eps2).sum(axis=1), 0)
        k = int(np.argmax(count))
        if count[k] > best_c:
            best_h, best_c = int(h[k]), int(count[k])
    return best_h, best_c


# ---- steps 5 and 6 ---------------------------------------------------------------------------------------------------------------------
def ransac_refit(pos_a, pos_b, cand, p, capacity=None, n_candidates=None):
    """(REGISTRATION_DTYPE record, mask) over the first min(len(cand), capacity) candidates."""
    capacity = max(len(cand), 1) if capacity is None else capacity
    M = min(len(cand), capacity)
    pq = gather(pos_a, pos_b, cand[:M])
    eps2 = F64(p["max_epsilon"]) * F64(p["max_epsilon"])
    res = np.zeros(1, REGISTRATION_DTYPE)[0]
    res["n_candidates"] = len(cand) if n_candidates is None else n_candidates
    flags = FEW_CANDIDATES if M < 4 else 0
    model, mask, refits, best = np.full(12, np.nan), np.zeros(M, bool), 0, -1
    if M >= 4:
        h, count = ransac(pq, p)
        if count >= 4:
            best = h
            model = hypothesis_models(pq, p["seed"], [h])[0][0]
            mask = residual2(model, pq) <= eps2
    if best < 0:
        flags |= NO_MODEL
    else:
        while True:
            if refits == p["max_refits"]:
                flags |= CAPPED
                break
            new = fit_affine(pq[:, :3], pq[:, 3:], mask)
            if new is None:
                flags |= NO_MODEL
                break
            refits += 1
            model = new
            now = residual2(model, pq) <= eps2
            same = np.array_equal(now, mask)
            mask = now
            if same:
                break
    n = int(mask.sum())
    if n < p["min_inliers"] or F64(n) < F64(p["min_inlier_ratio"]) * F64(M):
        flags |= FEW_INLIERS
    res["m"] = model
    if n:
        with np.errstate(all="ignore"):
            e = np.sqrt(residual2(model, pq))
        chunks = -(-M // FIT_CHUNK)
        padded = np.zeros(chunks * FIT_CHUNK, F64)
        padded[:M] = np.where(mask, e, 0.0)
        res["mean_error"] = _ordered_sum(padded.reshape(chunks, FIT_CHUNK)) / F64(n)
        res["max_error"] = e[mask].max()
    else:
        res["mean_error"] = res["max_error"] = np.nan
    res["n_inliers"], res["best_hypothesis"], res["refits"], res["flags"] = n, best, refits, flags
    return res, mask.astype(np.uint8)


def register(pos_a, pos_b, p):
    """The whole recipe: a dict of every stage's output."""
    K = 3 + p["redundancy"]
    out = {}
    for name, pos in (("a", pos_a), ("b", pos_b)):
        idx, dd = knn(pos, K)
        out["idx_" + name], out["d2_" + name], out["desc_" + name] = idx, dd, descriptors(pos, idx)
    cand = match(out["desc_a"], out["desc_b"], p["ratio"])
    res, mask = ransac_refit(pos_a, pos_b, cand, p, capacity=max(len(np.asarray(pos_a).reshape(-1, 3)), 1))
    res["n_a"], res["n_b"] = int(described(out["desc_a"]).sum()), int(described(out["desc_b"]).sum())
    out.update(candidates=cand, result=res, mask=mask)
    return out


# ---- clouds for the tests ----------------------------------------------------------------------------------------------------------------
def rotation_x(deg, centre):
    """Rotation about the x axis through `centre` as a 3 x 4 matrix."""
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    A = np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
    centre = np.asarray(centre, F64)
    return np.hstack([A, (centre - A @ centre)[:, None]])


def apply(m, pts):
    m = np.asarray(m, F64).reshape(3, 4)
    return np.asarray(pts, F64) @ m[:, :3].T + m[:, 3]


def inside(pts, box, margin):
    return np.all((pts >= margin) & (pts <= np.asarray(box, F64) - 1 - margin), axis=1)
