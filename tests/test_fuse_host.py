"""The view fusion without a GPU: the parameter block and the view record, the host helpers (inverse, bounds, PSF matrix) against the
restatement of tests/fuse_reference.py bit for bit, every refusal of the entry points (each is reached before a device call), and the
restatement on its own."""
import ctypes as C

import numpy as np
import pytest

from . import fuse_reference as R

F64 = np.float64


@pytest.fixture(autouse=True)
def library_with_the_fusion(mvs):
    """Every test of this file, the restatement's own included, speaks about a library that has the fusion."""
    missing = [n for n in ("mvsim_fuse_views_dev", "mvsim_align_views_dev", "mvsim_fuse_invert", "mvsim_fusion_bounds") if n not in mvs._lib.SIGNATURES]
    assert not missing, missing


def matrices(seed=0, n=40):
    """Random, rotated, scaled and sheared 3 x 4 matrices."""
    rng = np.random.default_rng(seed)
    out = [R.identity(), R.translation((3, -4.5, 7.25))]
    for k in range(n):
        kind = k % 4
        if kind == 0:
            m = rng.normal(0, 1, (3, 4))
        elif kind == 1:
            m = R.rotation(k % 3, rng.uniform(-180, 180), rng.uniform(0, 100, 3))
        elif kind == 2:
            m = np.hstack([np.diag(rng.uniform(0.2, 5, 3)), rng.uniform(-50, 50, (3, 1))])
        else:
            m = R.identity()
            m[0, 1], m[1, 2], m[2, 0] = rng.uniform(-1, 1, 3)
            m[:, 3] = rng.uniform(-50, 50, 3)
        out.append(m)
    return out


def test_defaults_and_struct_sizes(mvs):
    assert C.sizeof(mvs._lib.FuseParams) == 32 and C.sizeof(mvs._lib.FuseView) == 136
    p = mvs.fuse_params()
    assert list(p.blend) == [8.0, 8.0, 8.0] and p.background == 0.0 and p.src_type == mvs._lib.MVSIM_SRC_F32
    assert list(mvs.fuse_params(blend=3.5).blend) == [3.5, 3.5, 3.5] and list(mvs.fuse_params(blend=(1, 2, 3)).blend) == [1.0, 2.0, 3.0]
    with pytest.raises(TypeError):
        mvs.fuse_params(nonsense=1)
    g = mvs.fusion_geometry()
    assert all(b >= 1 for b in g["brick"]) and g["max_blocks"] >= 8 and g["max_blocks"] % 8 == 0
    assert mvs._lib.load().mvsim_fusion_geometry(None) == mvs._lib.MVSIM_EINVAL
    mvs._lib.load().mvsim_fuse_params_default(None)        # a null block is ignored


def test_invert_equals_the_restatement(mvs):
    for m in matrices():
        got, want = mvs.fuse_invert(m), R.invert(m)
        assert want is not None and R.same_bits(got.reshape(12), want), m
        back = np.vstack([got, [0, 0, 0, 1]]) @ np.vstack([m, [0, 0, 0, 1]])
        assert np.abs(back - np.eye(4)).max() < 1e-9


def test_invert_refuses_singular_and_non_finite_matrices(mvs):
    flat = R.identity()
    flat[2, 2] = 0.0
    twice = R.identity()
    twice[1] = twice[0]
    huge = R.identity() * 1e200                            # det overflows
    for m in (flat, twice, huge, np.zeros((3, 4))):
        assert mvs.fuse_invert(m) is None and R.invert(m) is None
    for at in range(12):
        for bad in (np.nan, np.inf, -np.inf):
            m = R.rotation(0, 30, (5, 5, 5)).reshape(12).copy()
            m[at] = bad
            assert mvs.fuse_invert(m) is None and R.invert(m) is None
    L = mvs._lib.load()
    m, s = (C.c_double * 12)(), C.c_int(0)
    assert L.mvsim_fuse_invert(None, m, C.byref(s)) == L.mvsim_fuse_invert(m, None, C.byref(s)) == L.mvsim_fuse_invert(m, m, None) == mvs._lib.MVSIM_EINVAL
    keep = (C.c_double * 12)(*[7.0] * 12)                  # a singular matrix leaves inv untouched
    assert L.mvsim_fuse_invert(m, keep, C.byref(s)) == 0 and s.value == 1 and list(keep) == [7.0] * 12


def test_bounds_equal_the_restatement(mvs):
    ms = matrices(seed=1, n=12)
    rng = np.random.default_rng(2)
    dims = [tuple(int(v) for v in rng.integers(1, 60, 3)) for _ in ms]
    for n in (1, 2, 5, len(ms)):
        assert mvs.fusion_bounds(ms[:n], dims[:n]) == R.bounds(ms[:n], dims[:n])
    assert mvs.fusion_bounds([R.identity()], [(10, 20, 30)]) == ((0, 0, 0), (10, 20, 30))
    assert mvs.fusion_bounds([R.translation((-2.5, 0, 3))], [(10, 1, 30)]) == ((-3, 0, 3), (11, 1, 30))
    pair = [R.identity(), R.translation((4, -3, 2))]
    assert mvs.fusion_bounds(pair, [(10, 10, 10)] * 2) == ((0, -3, 0), (14, 13, 12)) == R.bounds(pair, [(10, 10, 10)] * 2)
    assert mvs.fusion_bounds(pair, [(10, 10, 10)] * 2, True) == ((4, 0, 2), (6, 7, 8)) == R.bounds(pair, [(10, 10, 10)] * 2, True)
    rot = [R.identity(), R.rotation(0, 45, (20, 20, 20)), R.rotation(2, 30, (20, 20, 20))]
    for inter in (False, True):
        assert mvs.fusion_bounds(rot, [(41, 41, 41)] * 3, inter) == R.bounds(rot, [(41, 41, 41)] * 3, inter)


def test_bounds_refusals(mvs):
    apart = [R.identity(), R.translation((100, 0, 0))]
    assert R.bounds(apart, [(10, 10, 10)] * 2, True) is None
    with pytest.raises(ValueError, match="empty"):
        mvs.fusion_bounds(apart, [(10, 10, 10)] * 2, True)
    assert mvs.fusion_bounds(apart, [(10, 10, 10)] * 2) == ((0, 0, 0), (110, 10, 10))
    bad = R.identity()
    bad[1, 3] = np.nan
    with pytest.raises(ValueError, match="finite"):
        mvs.fusion_bounds([bad], [(4, 4, 4)])
    with pytest.raises(ValueError):
        mvs.fusion_bounds([R.identity()], [(4, 0, 4)])
    with pytest.raises(ValueError):
        mvs.fusion_bounds([R.identity()] * 33, [(4, 4, 4)] * 33)
    L = mvs._lib.load()
    m, d, o = (C.c_double * 12)(), (C.c_int64 * 3)(1, 1, 1), (C.c_int64 * 3)()
    assert L.mvsim_fusion_bounds(m, d, 0, 0, o, o) == mvs._lib.MVSIM_EINVAL and L.mvsim_fusion_bounds(None, d, 1, 0, o, o) == mvs._lib.MVSIM_EINVAL


def test_psf_matrix_for_odd_and_even_extents(mvs):
    rot = R.rotation(0, 45, (0, 0, 0))
    for kdim, odim in (((5, 5, 5), (5, 5, 5)), ((4, 6, 8), (4, 6, 8)), ((5, 4, 7), (9, 8, 6)), ((1, 1, 1), (3, 3, 3))):
        for m in (R.identity(), rot, matrices(seed=3, n=4)[-1]):
            got = mvs.psf_matrix(m, kdim, odim)
            assert R.same_bits(got, R.psf_matrix(m, kdim, odim))
            c, c2 = np.array([k // 2 for k in kdim], F64), np.array([k // 2 for k in odim], F64)
            assert np.abs(got[:, :3] @ c + got[:, 3] - c2).max() < 1e-9, "the centre goes to the centre"
            assert np.array_equal(got[:, :3], np.asarray(m)[:, :3])
    with pytest.raises(ValueError):
        mvs.psf_matrix(rot, (0, 1, 1), (1, 1, 1))


def test_every_refusal_is_reachable_without_a_device(mvs):
    """A null context is the LAST thing every entry point notices: each refusal below is reached before a device call."""
    L, EINVAL = mvs._lib.load(), mvs._lib.MVSIM_EINVAL
    buf = (C.c_char * 4096)()
    base = C.addressof(buf)                                # never dereferenced: no call gets as far as a launch

    def msg():
        return (L.mvsim_last_error() or b"").decode()

    def view(src=base, dim=(4, 4, 4), m_dev=None):
        v = mvs._lib.FuseView()
        v.src, v.m_dev = src, m_dev
        for d in range(3):
            v.dim[d] = dim[d]
        for k, val in enumerate(R.identity().reshape(12)):
            v.m[k] = val
        return v

    def table(*views):
        return (mvs._lib.FuseView * len(views))(*views)

    i3 = lambda *v: (C.c_int64 * 3)(*v)                    # noqa: E731
    out = C.c_void_p(base + 2048)
    outs = (C.c_void_p * 2)(base + 2048, base + 3072)
    for fn, tail, host in ((L.mvsim_fuse_views_dev, (out, None, None), False), (L.mvsim_fuse_views, (out, None, None), True),
                           (L.mvsim_align_views_dev, (outs, None, None), False), (L.mvsim_align_views, (outs, outs, None), True)):
        good = [table(view(), view()), 2, i3(0, 0, 0), i3(4, 4, 4), C.byref(mvs.fuse_params())]
        assert fn(None, *good, *tail) == EINVAL and "ctx" in msg(), msg()

        def refused(at, value, tail=tail):
            args = list(good)
            args[at] = value
            assert fn(None, *args, *tail) == EINVAL, (fn.__name__, at)
            assert "ctx" not in msg(), (fn.__name__, at, msg())

        for at in (0, 2, 3, 4):
            refused(at, None)
        for n in (0, -1, 33):
            refused(1, n)
        refused(0, table(view(src=None), view()))
        for dim in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
            refused(0, table(view(), view(dim=dim)))
            refused(3, i3(*dim))
        for blend in (-1.0, np.nan, np.inf, (8.0, 8.0, -0.5)):
            refused(4, C.byref(mvs.fuse_params(blend=blend)))
        for t in (-1, 2):
            refused(4, C.byref(mvs.fuse_params(src_type=t)))
        # an output that overlaps a source: the last voxel of the source is the first of the output
        refused(0, table(view(), view(src=base + 2048 - 255)))
        assert fn(None, *good, None, *tail[1:]) == EINVAL and "ctx" not in msg()
        if host:                                           # host buffers take host matrices only
            refused(0, table(view(), view(m_dev=base)))
    assert L.mvsim_fuse_views_dev(None, *good, out, C.c_void_p(base + 100), None) == EINVAL and "overlaps" in msg()
    weights = (C.c_void_p * 2)(None, base + 100)
    assert L.mvsim_align_views_dev(None, *good, outs, weights, None) == EINVAL and "overlaps" in msg()


# ---- the restatement on its own -----------------------------------------------------------------------------------------------------------
def volume(shape, seed=0):
    return np.random.default_rng(seed).uniform(-3, 900, shape).astype(np.float32)


def test_restatement_identity_returns_the_source_bits():
    for shape in ((1, 1, 1), (3, 1, 2), (7, 9, 11)):
        src = volume(shape)
        dim = shape[::-1]
        out, den, status = R.fuse([src], [R.identity()], (0, 0, 0), dim, blend=(0, 0, 0))
        assert R.same_bits(out, src) and np.all(den == 1.0) and status[0] == 0
        al, wt, _ = R.align([src.astype(np.uint16)], [R.identity()], (0, 0, 0), dim, blend=(0, 0, 0))
        assert R.same_bits(al[0], src.astype(np.uint16).astype(np.float32)) and np.all(wt[0] == 1.0)


def test_restatement_integer_translation_returns_the_shifted_source():
    src = volume((6, 7, 8), seed=1)
    t = (2, -3, 1)                                         # output = view + t
    out, den, _ = R.fuse([src], [R.translation(t)], (-4, -4, -4), (16, 16, 16), blend=(0, 0, 0), background=-7.0)
    want = np.full((16, 16, 16), -7.0, np.float32)
    want[4 + 1:4 + 1 + 6, 4 - 3:4 - 3 + 7, 4 + 2:4 + 2 + 8] = src
    assert R.same_bits(out, want)
    assert den.sum() == src.size


def test_restatement_quarter_turn_equals_rot90():
    src = volume((5, 9, 9), seed=2)
    # 90 degrees about z through the centre of the xy plane: (x, y) -> (c - (y - c), c + (x - c)), exact in fp64
    m = np.array([[0.0, -1.0, 0.0, 8.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])
    out, _, _ = R.fuse([src], [m], (0, 0, 0), (9, 9, 5), blend=(0, 0, 0))
    # out[z, y', x'] = src[z, y, x] with x' = 8 - y, y' = x
    assert R.same_bits(out, np.rot90(src, k=-1, axes=(1, 2)))
    want = np.empty_like(src)
    for y in range(9):
        for x in range(9):
            want[:, x, 8 - y] = src[:, y, x]
    assert R.same_bits(out, want)


def test_restatement_weights_and_average():
    """Two copies of one volume average to the volume wherever both have weight; the ramp is the smoothstep of the distance to the
    nearest face; a singular view is absent."""
    src = volume((12, 12, 12), seed=3)
    out, den, status = R.fuse([src, src, src], [R.identity(), R.identity(), np.zeros((3, 4))], (0, 0, 0), (12, 12, 12), blend=(4, 4, 4))
    assert list(status) == [0, 0, R.SINGULAR]
    assert np.abs(out[1:-1, 1:-1, 1:-1] - src[1:-1, 1:-1, 1:-1]).max() <= 1e-4 * np.abs(src).max()
    assert np.all(out[0] == 0.0) and np.all(den[0] == 0.0), "weight 0 on a face: background"
    assert den[6, 6, 6] == 2.0
    q = 1.0 / 4.0
    assert den[6, 6, 1] == np.float32(2 * (q * q) * (3.0 - 2.0 * q))
