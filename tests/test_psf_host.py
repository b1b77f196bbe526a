"""The PSF extraction without a GPU: the parameter block and the result record, the host helpers (offsets, selection, finish) against
the restatement of tests/psf_reference.py bit for bit, every refusal of the entry points (each is reached before a device call), and
the restatement on its own."""
import ctypes as C

import numpy as np
import pytest

from . import fuse_reference as FR
from . import psf_reference as R

F64 = np.float64


@pytest.fixture(autouse=True)
def library_with_the_extraction(mvs):
    """Every test of this file, the restatement's own included, speaks about a library that has the PSF extraction."""
    missing = [n for n in ("mvsim_extract_psf_dev", "mvsim_psf_offsets", "mvsim_psf_select", "mvsim_psf_finish") if n not in mvs._lib.SIGNATURES]
    assert not missing, missing


def matrices():
    """The matrices the host and the GPU tests share: identity, a rotation about each axis, a z spacing of 3, a shear."""
    c = (19.5, 16.0, 8.0)
    shear = FR.identity()
    shear[0, 1], shear[1, 2], shear[2, 0], shear[:, 3] = 0.3, -0.2, 0.1, (1.5, 2.0, -0.75)
    return {"none": None, "identity": FR.identity(), "rot_x": FR.rotation(0, 45, c), "rot_y": FR.rotation(1, -21, c),
            "rot_z": FR.rotation(2, 57, c), "z_spacing": np.hstack([np.diag([1.0, 1.0, 3.0]), [[0.0], [0.0], [-4.0]]]), "shear": shear}


def singular_matrices():
    flat = FR.identity()
    flat[2, 2] = 0.0
    nan, inf = FR.identity(), FR.identity()
    nan[1, 0], inf[0, 2] = np.nan, np.inf
    return {"flat": flat, "zero": np.zeros((3, 4)), "nan": nan, "inf": inf, "huge": FR.identity() * 1e200}


def test_defaults_and_struct_sizes(mvs):
    assert C.sizeof(mvs._lib.PsfParams) == 64 and C.sizeof(mvs._lib.PsfResult) == 72 and R.RESULT_DTYPE.itemsize == 72
    p = mvs.psf_params()
    assert list(p.kdim) == [15, 15, 15] and list(p.min_separation) == [15.0, 15.0, 15.0]
    assert (p.src_type, p.subtract_min, p.normalize, p.pad) == (mvs._lib.MVSIM_SRC_F32, 1, 1, 0)
    assert list(mvs.psf_params(kdim=(3, 5, 7)).kdim) == [3, 5, 7] and list(mvs.psf_params(min_separation=2.5).min_separation) == [2.5] * 3
    with pytest.raises(TypeError):
        mvs.psf_params(nonsense=1)
    g = mvs.psf_geometry()
    assert g["chunk"] == R.CHUNK == mvs._lib.MVSIM_PSF_CHUNK and g["taps_per_block"] >= 64 and g["select_tile"] >= 64
    assert g["max_blocks"] == -(-R.MAX_DIM ** 3 // g["taps_per_block"]) * (R.MAX_POINTS // R.CHUNK)
    assert mvs._lib.load().mvsim_psf_geometry(None) == mvs._lib.MVSIM_EINVAL
    mvs._lib.load().mvsim_psf_params_default(None)         # a null block is ignored
    assert (mvs._lib.MVSIM_PSF_MAX_POINTS, mvs._lib.MVSIM_PSF_MAX_DIM) == (R.MAX_POINTS, R.MAX_DIM)


@pytest.mark.parametrize("kdim", [(1, 1, 1), (3, 1, 5), (7, 7, 7), (15, 15, 21), (63, 3, 1)])
def test_offsets_equal_the_restatement(mvs, kdim):
    for name, m in matrices().items():
        got, want = mvs.psf_offsets(m, kdim), R.offsets(m, kdim)
        assert want is not None and R.same_bits(got, want), name
        if name in ("none", "identity"):
            jx, jy, jz = R.taps_j(kdim)
            assert np.array_equal(got, np.stack([jx, jy, jz], axis=-1)), "with the identity the offset is the tap's own index"
    m = matrices()["rot_x"].copy()
    m[:, 3] = np.nan                                        # only A is used
    assert R.same_bits(mvs.psf_offsets(m, kdim), R.offsets(matrices()["rot_x"], kdim))


def test_offsets_refuse_singular_and_non_finite_matrices(mvs):
    for name, m in singular_matrices().items():
        assert mvs.psf_offsets(m, (3, 3, 3)) is None and R.offsets(m, (3, 3, 3)) is None, name
    for kdim in ((0, 3, 3), (3, 4, 3), (3, 3, 65), (-1, 3, 3)):
        with pytest.raises(ValueError):
            mvs.psf_offsets(None, kdim)


def cloud(seed, n, dim, spread=4.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-spread, np.array(dim, F64) - 1 + spread, (n, 3))


def same_record(a, b):
    return all(R.same_bits(np.asarray(a[k]), np.asarray(b[k])) for k in R.RESULT_DTYPE.names)


def test_selection_equals_the_restatement(mvs):
    dim = (40, 33, 17)
    seen = set()
    for name, m in matrices().items():
        for seed, (kdim, sep) in enumerate([((3, 3, 3), (0, 0, 0)), ((5, 3, 7), (4.0, 4.0, 4.0)), ((7, 7, 7), (2.5, 0.0, 9.0)), ((3, 5, 3), (3.0, 50.0, 6.0))]):
            pos = cloud(seed, 90, dim)
            pos[3], pos[17, 1], pos[40, 2], pos[41, 0] = np.nan, np.inf, -np.inf, np.nan
            pos[50] = pos[51]                               # an exact duplicate crowds both
            use = (np.random.default_rng(seed).uniform(size=len(pos)) > 0.2).astype(np.uint8)
            for u in (None, use):
                got_st, got = mvs.psf_select(pos, dim, m, u, mvs.psf_params(kdim=kdim, min_separation=sep))
                want_st, want = R.select(pos, dim, m, u, kdim, sep)
                assert np.array_equal(got_st, want_st) and same_record(got, want), (name, kdim, sep)
                assert got["n_listed"] == len(pos) == got["n_used"] + got["n_nonfinite"] + got["n_masked"] + got["n_outside"] + got["n_crowded"]
                assert want["n_nonfinite"] == 4
                seen |= set(int(v) for v in want_st)
                if all(sep) and u is None:
                    assert want_st[50] == want_st[51] and want_st[50] in (R.CROWDED, R.OUTSIDE)
    assert seen == {R.USED, R.NONFINITE, R.MASKED, R.OUTSIDE, R.CROWDED}


def test_selection_edges(mvs):
    """A corner exactly on 0 and on N - 1 is inside, one ulp beyond is outside; a separation exactly equal to min_separation does not
    crowd, one ulp less does; a masked or outside neighbour crowds all the same, a non-finite one does not."""
    dim, kdim = (40, 31, 17), (5, 3, 7)                    # 37 + 2 and 29 + 1 stay in the binade of N - 1: the ulp survives the sum
    p = mvs.psf_params(kdim=kdim, min_separation=(0, 0, 0))
    lo, hi = np.array([2.0, 1.0, 3.0]), np.array([37.0, 29.0, 13.0])
    pos = np.array([lo, hi, [np.nextafter(2.0, 0), 1, 3], [2, 1, np.nextafter(3.0, 0)], [np.nextafter(37.0, 99), 29, 13], [37, np.nextafter(29.0, 99), 13]])
    for m in (None, FR.identity()):
        st, rec = mvs.psf_select(pos, dim, m, None, p)
        assert list(st) == [0, 0, 3, 3, 3, 3] and np.array_equal(st, R.select(pos, dim, m, None, kdim, (0, 0, 0))[0])
    dim, sep = (40, 33, 17), (4.0, 4.0, 4.0)
    p = mvs.psf_params(kdim=(1, 1, 1), min_separation=sep)
    base = np.array([10.0, 10.0, 8.0])
    for other, crowded in (((14.0, 10, 8), False), ((np.nextafter(14.0, 0), 10, 8), True), ((13, 13, 11.5), True), ((13, 13, 12.0), False),
                           ((10.0, 10.0, 8.0), True), ((np.nan, 10, 8), False)):
        pos = np.array([base, other])
        st, _ = mvs.psf_select(pos, dim, None, None, p)
        assert np.array_equal(st, R.select(pos, dim, None, None, (1, 1, 1), sep)[0])
        assert (st[0] == R.CROWDED) == crowded, other
    pos = np.array([base, base + 1.0, [-50.0, 10, 8], [-49.0, 10, 8]])
    st, rec = mvs.psf_select(pos, dim, None, np.array([1, 0, 1, 1], np.uint8), p)
    assert list(st) == [R.CROWDED, R.MASKED, R.OUTSIDE, R.OUTSIDE] and rec["n_used"] == 0
    # no points at all
    st, rec = mvs.psf_select(np.zeros((0, 3)), dim, None, None, p)
    assert len(st) == 0 and rec["n_listed"] == 0 and rec["flags"] == 0


def test_selection_with_a_singular_matrix(mvs):
    pos = cloud(5, 20, (40, 33, 17))
    for name, m in singular_matrices().items():
        st, rec = mvs.psf_select(pos, (40, 33, 17), m, None, mvs.psf_params(kdim=3))
        want_st, want = R.select(pos, (40, 33, 17), m, None, (3, 3, 3))
        assert want_st is None and same_record(rec, want) and rec["flags"] == R.SINGULAR and rec["n_listed"] == 20 and rec["n_used"] == 0, name


@pytest.mark.parametrize("kdim", [(1, 1, 1), (3, 1, 5), (7, 7, 7), (15, 15, 21), (63, 3, 1)])
def test_finish_equals_the_restatement(mvs, kdim):
    shape = kdim[::-1]
    rng = np.random.default_rng(kdim[0])
    cases = {"random": rng.uniform(50, 9000, shape), "negative": rng.uniform(-100, 100, shape), "constant": np.full(shape, 7.0),
             "zeros": np.zeros(shape), "nan": rng.uniform(1, 2, shape), "inf": rng.uniform(1, 2, shape), "minus_zero": np.abs(rng.normal(0, 1, shape))}
    cases["nan"].flat[-1] = np.nan
    cases["inf"].flat[0] = np.inf
    cases["minus_zero"].flat[0], cases["minus_zero"].flat[-1] = 0.0, -0.0
    for name, totals in cases.items():
        for n_used in (1, 3, 257):
            for sub in (1, 0):
                for norm in (1, 0):
                    rec = R.record(n_used + 2)
                    rec["n_used"], rec["n_masked"] = n_used, 2
                    p = mvs.psf_params(kdim=kdim, subtract_min=sub, normalize=norm)
                    got, got_rec = mvs.psf_finish(totals, rec, p)
                    want, want_rec = R.finish(totals, rec, sub, norm)
                    assert R.same_bits(got, want) and same_record(got_rec, want_rec), (name, n_used, sub, norm)
    flat = R.finish(cases["constant"], rec, 1, 1)
    assert flat[1]["flags"] == R.FLAT and np.all(flat[0] == 0.0)
    for flags, n_used, want_flags in ((0, 0, R.NO_BEADS), (R.SINGULAR, 0, R.SINGULAR), (R.SINGULAR, 5, R.SINGULAR)):
        rec = R.record(9, flags)
        rec["n_used"] = n_used
        got, got_rec = mvs.psf_finish(cases["random"], rec, mvs.psf_params(kdim=kdim))
        want, want_rec = R.finish(cases["random"], rec)
        assert R.same_bits(got, want) and same_record(got_rec, want_rec) and got_rec["flags"] == want_flags
        assert not got.any() and not np.signbit(got).any()


def test_every_refusal_is_reachable_without_a_device(mvs):
    """A null context is the LAST thing every entry point notices: each refusal below is reached before a device call."""
    L, EINVAL = mvs._lib.load(), mvs._lib.MVSIM_EINVAL
    buf = (C.c_char * 8192)()
    base = C.addressof(buf)                                # never dereferenced: no call gets as far as a launch
    P = lambda off: C.c_void_p(base + off)                 # noqa: E731
    i3 = lambda *v: (C.c_int64 * 3)(*v)                    # noqa: E731
    m12 = np.ascontiguousarray(FR.identity().reshape(12))
    M = C.c_void_p(m12.ctypes.data)

    def msg():
        return (L.mvsim_last_error() or b"").decode()

    def params(**kw):
        return C.byref(mvs.psf_params(kdim=3, **kw))

    bad_params = [None] + [C.byref(mvs.psf_params(kdim=k)) for k in ((0, 3, 3), (3, 2, 3), (3, 3, 65), (-3, 3, 3))]
    bad_params += [params(min_separation=s) for s in (-1.0, np.nan, np.inf, (1.0, 1.0, -0.5))] + [params(src_type=t) for t in (-1, 2)]
    bad_dims = [None, i3(0, 4, 4), i3(4, -1, 4), i3(4, 4, 0)]
    bad_strides, bad_caps = (0, 16, 23, 28, -24), (0, -1, R.MAX_POINTS + 1)

    # name: (function, good arguments behind the context, {argument index: bad values})
    dev = {
        "extract_dev": (L.mvsim_extract_psf_dev, [P(0), i3(4, 4, 4), P(1024), 24, P(2048), 8, None, None, None, params(), P(4096), P(5120), None],
                        {0: [None], 1: bad_dims, 2: [None], 3: bad_strides, 4: [None], 5: bad_caps, 9: bad_params, 10: [None, P(252), P(0)], 11: [None]}),
        "select_dev": (L.mvsim_psf_select_dev, [P(1024), 24, P(2048), 8, None, None, None, i3(4, 4, 4), params(), P(3072), P(5120)],
                       {0: [None], 1: bad_strides, 2: [None], 3: bad_caps, 7: bad_dims, 8: bad_params, 9: [None], 10: [None]}),
        "gather_dev": (L.mvsim_psf_gather_dev, [P(0), i3(4, 4, 4), P(1024), 24, P(2048), 8, P(3072), None, None, params(), P(4096)],
                       {0: [None], 1: bad_dims, 2: [None], 3: bad_strides, 4: [None], 5: bad_caps, 6: [None], 9: bad_params, 10: [None]}),
        "finish_dev": (L.mvsim_psf_finish_dev, [P(4096), params(), P(0), P(5120)], {0: [None], 1: bad_params, 2: [None], 3: [None]}),
        "use_dev": (L.mvsim_psf_use_from_matches_dev, [P(0), P(2048), 8, None, 0, 8, P(3072)],
                    {0: [None], 1: [None], 2: bad_caps, 4: [-1, 2], 5: bad_caps, 6: [None]}),
        "extract": (L.mvsim_extract_psf, [P(0), i3(4, 4, 4), P(1024), 24, 8, None, None, params(), P(4096), C.cast(P(5120), C.POINTER(mvs._lib.PsfResult)), None],
                    {0: [None], 1: bad_dims, 2: [None], 3: bad_strides, 4: [-1, R.MAX_POINTS + 1], 7: bad_params, 8: [None, P(252)], 9: [None]}),
    }
    for name, (fn, good, bad) in dev.items():
        assert fn(None, *good) == EINVAL and "ctx" in msg(), (name, msg())
        for at, values in bad.items():
            for value in values:
                args = list(good)
                args[at] = value
                assert fn(None, *args) == EINVAL, (name, at)
                assert "ctx" not in msg(), (name, at, msg())
    # both matrices at once
    for name, at in (("extract_dev", 7), ("select_dev", 5), ("gather_dev", 7)):
        fn, good, _ = dev[name]
        args = list(good)
        args[at], args[at + 1] = M, P(6144)
        assert fn(None, *args) == EINVAL and "exclude" in msg(), name
        args[at + 1] = None
        assert fn(None, *args) == EINVAL and "ctx" in msg(), name
    fn, good, _ = dev["extract_dev"]
    args = list(good)
    args[10] = P(252)                                      # the last voxel of the image is the first tap of the PSF
    assert fn(None, *args) == EINVAL and "overlaps" in msg()
    # the host helpers
    st, rec, one = (C.c_ubyte * 8)(), mvs._lib.PsfResult(), C.c_int(0)
    good = [P(1024), 24, 8, None, None, i3(4, 4, 4), params(), st, C.byref(rec)]
    assert L.mvsim_psf_select(*good) == 0
    for at, values in {0: [None], 1: bad_strides, 2: [-1, R.MAX_POINTS + 1], 5: bad_dims, 6: bad_params, 7: [None], 8: [None]}.items():
        for value in values:
            args = list(good)
            args[at] = value
            assert L.mvsim_psf_select(*args) == EINVAL, at
    totals, out = np.ones(27), np.zeros(27, np.float32)
    good = [C.c_void_p(totals.ctypes.data), params(), C.c_void_p(out.ctypes.data), C.byref(rec)]
    assert L.mvsim_psf_finish(*good) == 0
    for at, values in {0: [None], 1: bad_params, 2: [None], 3: [None]}.items():
        for value in values:
            args = list(good)
            args[at] = value
            assert L.mvsim_psf_finish(*args) == EINVAL, at
    off = np.zeros(81)
    assert L.mvsim_psf_offsets(None, i3(3, 3, 3), C.c_void_p(off.ctypes.data), C.byref(one)) == 0 and one.value == 0
    for args in ((None, None, C.c_void_p(off.ctypes.data), C.byref(one)), (None, i3(3, 3, 3), None, C.byref(one)),
                 (None, i3(3, 3, 3), C.c_void_p(off.ctypes.data), None)):
        assert L.mvsim_psf_offsets(*args) == EINVAL


# ---- the restatement on its own -----------------------------------------------------------------------------------------------------------
def volume(shape, seed=0):
    return np.random.default_rng(seed).uniform(-3, 900, shape).astype(np.float32)


def test_restatement_integer_bead_under_the_identity_returns_the_window():
    img = volume((17, 33, 40), seed=1)
    for m in (None, FR.identity()):
        psf, rec, status, totals = R.extract(img, [[20.0, 11.0, 8.0]], m, None, (5, 3, 7), (0, 0, 0), subtract_min=0, normalize=0)
        assert list(status) == [0] and rec["n_used"] == 1 and rec["flags"] == 0
        assert R.same_bits(psf, img[8 - 3:8 + 4, 11 - 1:11 + 2, 20 - 2:20 + 3])
        assert R.same_bits(totals, img[8 - 3:8 + 4, 11 - 1:11 + 2, 20 - 2:20 + 3].astype(F64))
    u16 = img.astype(np.uint16)
    psf, _, _, _ = R.extract(u16, [[20.0, 11.0, 8.0]], None, None, (5, 3, 7), (0, 0, 0), subtract_min=0, normalize=0)
    assert R.same_bits(psf, u16[5:12, 10:13, 18:23].astype(np.float32))


def test_restatement_mean_minimum_and_normalisation():
    """Two beads at integer positions: the mean of the two windows; the minimum comes off, the sum goes to one."""
    img = volume((17, 33, 40), seed=2)
    pos = [[20.0, 11.0, 8.0], [9.0, 20.0, 5.0]]
    w = [img[z - 1:z + 2, y - 1:y + 2, x - 1:x + 2].astype(F64) for x, y, z in ((20, 11, 8), (9, 20, 5))]
    psf, rec, status, totals = R.extract(img, pos, None, None, (3, 3, 3), (0, 0, 0))
    mean = (w[0] + w[1]) / 2.0
    assert R.same_bits(totals, w[0] + w[1]) and rec["minimum"] == mean.min() and rec["n_used"] == 2
    assert abs(float(psf.astype(F64).sum()) - 1.0) < 1e-6 and psf.min() == 0.0
    assert np.allclose(psf, (mean - mean.min()) / (mean - mean.min()).sum(), rtol=1e-6)
    # half a voxel along x: the average of two neighbouring windows
    psf, _, _, _ = R.extract(img, [[20.5, 11.0, 8.0]], None, None, (3, 3, 3), (0, 0, 0), 0, 0)
    a, b = img[7:10, 10:13, 19:22].astype(F64), img[7:10, 10:13, 20:23].astype(F64)
    assert R.same_bits(psf, (a + 0.5 * (b - a)).astype(np.float32))


def test_restatement_chunked_sums_differ_from_a_flat_sum_only_by_rounding():
    rng = np.random.default_rng(3)
    totals = rng.uniform(0, 1e6, (5, 9, 13))
    rec = R.record(600)
    rec["n_used"] = 600
    psf, out = R.finish(totals, rec, 1, 1)
    mean = totals / 600.0
    assert out["minimum"] == mean.min() and abs(out["sum"] - (mean - mean.min()).sum()) < 1e-9 * out["sum"]
    assert R.use_from_matches([(0, 5), (2, 9), (7, 1), (1, -1)], 9, 3, [1, 0, 1, 1], 0, 4).tolist() == [1, 0, 0, 0]
    assert R.use_from_matches([(0, 5), (2, 9), (7, 1)], 3, 8, None, 1, 8).tolist() == [0, 1, 0, 0, 0, 1, 0, 0]
