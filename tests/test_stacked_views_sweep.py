"""mvsim_simulate_views_dev with the views STACKED (csrc/api_view.cpp: views_enqueue_batched), swept over every kernel form that call
reaches (tests/stacked_views_cases.py).  The stacked call hands the view index to kernels that otherwise never see one: the LDS-table
rotate + attenuate kernel (inverse models from a table, blockIdx.z), passes A, B, D and E (V x Nz planes, the z-blocked pitches), the
PSF's passes (V x Kz planes of taps), the direct z pass (blockIdx.y: source, destination, taps and partial sums of the view) and the
sampler's per-view table.

Every case asserts, per view:
  a. the stacked path ran (mvsim_get_extract_path reports V views in the last extract, 1 behind the single view in front of it);
  b. noisy and noise-free acquisitions -- and the caller's normalised PSFs -- equal V sequential mvsim_simulate_view_dev calls of a fresh
     context bit for bit (a case's own convolution options, zconv_strided / exp, are set in both contexts: they choose the z kernel, and
     k_zconv and k_zconv_strided differ in their summation order by design);
  c. the noise-free acquisition is within CONV_TOL = 1e-5 of the range of the fp64 oracle's rotate -> attenuate -> exact direct sum ->
     adjustImage, planes [::inc];
  d. the noisy acquisition equals the oracle's counter sampler on the GPU's own noise-free planes, bit for bit.
Then the workspaces across calls (a single sparse view behind a stack, stacks of changing geometry) and every reason for which
views_batchable declines, each beside the same call made batchable.

The CPU tests hold the table to the library's own geometry (mvsim_fft_geometry, mvsim_zpass_geometry), check that every target is named
by exactly one case which lands on it, and that the inputs expose a view that reads its neighbour's taps, angle or factor.

Largest range-normalised fp64 error of (c) measured on the MI355X: 3.99e-07 (the split y lines, 64 x 2010 x 2 with 3 x 31 x 2 taps); the
other cases 1.98e-07 .. 3.79e-07.  With the z pass handing every view the taps of view 0 (taps_view dropped from zconv_view) all 19 cases
of test_stacked_views_sweep fail."""
import ctypes as C
import zlib

import numpy as np
import pytest

from . import stacked_views_cases as S
from .conftest import rel_to_max

CONV_TOL = 1e-5          # range-normalised: the project's contract (tests/test_conv_sweep.py)
REF_DELTA = float(np.float32(0.01))
MIN_VALUE, TARGET = 1e-4, 1.0
ZINLINE_MIN_KZ = 48      # MVSIM_ZINLINE_MIN_KZ


def _same(a, b):
    """np.array_equal on the bit patterns (+0 is not -0, NaN equals itself)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _i64(vals):
    return (C.c_int64 * len(vals))(*vals)


def _ground_truth(shape, seed):
    """Random float32 values under a ramp along y and z (so that no two angles see the same volume), about a fifth of them exact zeros,
    an empty margin of up to three voxels along every axis long enough to have one."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    v = rng.random(shape, dtype=np.float32) * (rng.random(shape, dtype=np.float32) < 0.8)
    ramp = 0.25 + np.arange(ny, dtype=np.float32)[None, :, None] / ny + 0.5 * np.arange(nz, dtype=np.float32)[:, None, None] / nz
    v = (v * ramp).astype(np.float32)
    for ax, n in enumerate(shape):
        if n >= 5:
            m = min(max(1, n // 10), 3)
            sl = [slice(None)] * 3
            for s in (slice(0, m), slice(n - m, n)):
                sl[ax] = s
                v[tuple(sl)] = 0
    return np.ascontiguousarray(v)


def _inputs(case):
    """(ground truth, V raw PSFs): random asymmetric PSFs, a fresh draw per view."""
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    gt = _ground_truth(case.shape, int(rng.integers(1 << 30)))
    psfs = [rng.random(case.kshape, dtype=np.float32) + np.float32(0.05) for _ in range(case.V)]
    return gt, psfs


def _oracle_view(orc, gt, psf_raw, degrees, inc, factor_of=None):
    """The fp64 yardstick of one noise-free acquisition: (planes [::inc] of the adjusted exact convolution, adjustImage's factor, the
    convolved volume before the adjustment).  factor_of: adjust with this factor instead of the view's own."""
    att = orc.attenuate3d(orc.rotate_around_axis(gt, 0, degrees), REF_DELTA)
    con = orc.convolve_direct(att, psf_raw.copy())
    raw = con.copy()
    corr = orc.adjust_image(con, MIN_VALUE, TARGET)
    if factor_of is not None:
        con = (raw.astype(np.float64) * factor_of).astype(np.float32) + np.float32(MIN_VALUE)       # Tools.adjustImage, two roundings
    return np.ascontiguousarray(con[::inc]), corr, raw


# ------------------------------------------------------------------------------------------------ CPU: table, coverage, yardstick
def _fft_geometry(mvs, dim, kdim):
    g = _i64([0] * 5)
    return list(g) if mvs._lib.load().mvsim_fft_geometry(_i64(dim), _i64(kdim), g) == 0 else None


def test_zpass_geometry_query(mvs):
    """mvsim_zpass_geometry (host only): consistent with mvsim_fft_geometry and with itself over seeded shapes; refusals."""
    rng = np.random.default_rng(S.SEED)
    seen = set()
    for _ in range(4000):
        dim = [int(x) for x in rng.integers(1, 700, 3)]
        kdim = [int(x) for x in rng.integers(1, 65, 3)]
        inc = int(rng.integers(1, 9))
        fg, zg = _fft_geometry(mvs, dim, kdim), mvs.zpass_geometry(dim, kdim, inc)
        if fg is None:
            assert zg is None
            continue
        if zg is None:                                   # the inline FFT z pass of deep PSFs, unless the strided kernel takes the view
            assert kdim[2] >= ZINLINE_MIN_KZ and dim[2] + kdim[2] - 1 > 448, (dim, kdim, inc)
            continue
        kernel, zc, nch, nkxb = zg
        assert fg[4] == 1 and nkxb * 16 == fg[3] and zc >= 1 and nch == (dim[2] + zc - 1) // zc, (dim, kdim, inc, zg)
        assert kernel in ((0,) if inc == 1 or inc > 4 else (0, inc)), (dim, kdim, inc, zg)
        if kernel:
            assert zc % kernel == 0
        seen.add(kernel)
    assert seen == {0, 2, 3, 4}
    assert mvs.zpass_geometry((20, 22, 37), (3, 3, 15), 2)[0] == 2 and mvs.zpass_geometry((20, 22, 37), (3, 3, 15), 1)[0] == 0
    assert mvs.zpass_geometry((20, 22, 37), (3, 3, 65), 2) is None            # more than 64 z taps: the FFT z pass
    assert mvs.zpass_geometry((20, 22, 37), (3, 3, 15), 0) is None            # inc < 1
    assert mvs.zpass_geometry((4, 2241, 4), (3, 41, 2), 1) is None            # past the size table
    with pytest.raises(ValueError):
        mvs._lib.check(mvs._lib.load().mvsim_zpass_geometry(_i64((20, 22, 37)), _i64((3, 3, 65)), 2, _i64([0] * 4)))


def test_the_smallest_column_group_count_is_two(mvs):
    """nkxb == 1, which the sweep was asked for, does not exist: the shortest x half length is 16 points, 17 columns, two groups."""
    assert min(S.pick_x(n) for n in range(1, 40)) == 16
    assert mvs.zpass_geometry((1, 1, 1), (1, 1, 1), 1)[3] == 2 and mvs.zpass_geometry((2, 3, 4), (1, 2, 3), 1)[3] == 2


def test_stacked_sweep_lands_where_it_says_and_covers_every_target(mvs):
    cases = S.cases()
    assert len({c.name for c in cases}) == len(cases)
    named = [t for c in cases for t in c.targets]
    dup = {t for t in named if named.count(t) > 1}
    assert not dup, sorted(dup)                                   # one case per target: dropping any case leaves its targets unswept
    assert set(named) == set(S.TARGETS) and len(S.TARGETS) == len(set(S.TARGETS)), sorted(set(named) ^ set(S.TARGETS))
    for c in cases:
        assert c.targets, c.id
        nx, ny, nz = c.dim
        kx, ky, kz = c.kdim
        # what views_batchable asks of the geometry, restated: Nx <= Ny, the direct z pass, one reflection reaches every y halo row
        assert 2 <= c.V <= S.MAX_VIEWS and nx <= ny and kz <= 64 and ny > 1 and ky // 2 < ny and ky - 1 - ky // 2 < ny, c.id
        assert nx * ny * nz <= 1 << 26 and c.inc >= 1 and len(set(zip(c.degrees, range(c.V)))) == c.V
        fg = _fft_geometry(mvs, c.dim, c.kdim)
        px, py, pitch = c.padded()
        assert fg is not None and (fg[0], fg[1], fg[2], fg[3], fg[4]) == (px, py, nz, pitch, 1), (c.id, fg)
        zg = mvs.zpass_geometry(c.dim, c.kdim, c.inc)
        assert zg is not None and zg[3] == pitch // S.NLZ, (c.id, zg)
        lands = S.landing(c) | S.zpass_targets(c, zg)
        assert set(c.targets) <= lands, (c.id, sorted(set(c.targets) - lands))
        assert c.macs <= S.MAX_MACS, (c.id, c.macs)               # the fp64 direct sum of a view stays cheap
        assert len({c.seed(v) for v in range(c.V)}) == c.V and len({c.stream(v) for v in range(c.V)}) == c.V
    by = {c.name: c for c in cases}
    # the landings the table cannot compute itself, spelt out: the library's z kernel and chunk count
    assert mvs.zpass_geometry(by["chunks"].dim, by["chunks"].kdim, 1)[2] >= 2
    for name, kernel in (("inc2", 2), ("inc3", 3), ("inc4", 4), ("refused", 0), ("inc5", 0), ("inc7", 0), ("inc11", 0), ("forced", 0)):
        assert mvs.zpass_geometry(by[name].dim, by[name].kdim, by[name].inc)[0] == kernel, name
    assert by["angles"].degrees.count(120) == 2 and set(by["angles"].degrees) == {0, 90, 180, -90, 33, -52, 120}


def _sensitivity_sample():
    """The cases cheap enough to convolve three times per view on the CPU: all but the long rows and columns."""
    return [c for c in S.cases() if 3 * c.V * c.macs <= 4 * S.MAX_MACS]


@pytest.mark.parametrize("case", _sensitivity_sample(), ids=lambda c: c.id)
def test_stacked_inputs_expose_a_neighbours_operand(orc, case):
    """A view convolved with its neighbour's PSF, rotated by its neighbour's angle or adjusted by its neighbour's factor is far outside
    the tolerance (100 x CONV_TOL, the margin of test_sweep_inputs_expose_convolution_mistakes): what a wrong view stride would do."""
    gt, psfs = _inputs(case)
    right = [_oracle_view(orc, gt, psfs[v], case.degrees[v], case.inc) for v in range(case.V)]
    for v in range(case.V):
        w = (v + 1) % case.V
        want, corr, _ = right[v]
        assert abs(right[w][1] / corr - 1) > 1e-3, (v, corr, right[w][1])
        wrong = {"neighbour's factor": _oracle_view(orc, gt, psfs[v], case.degrees[v], case.inc, factor_of=right[w][1])[0],
                 "neighbour's PSF": _oracle_view(orc, gt, psfs[w], case.degrees[v], case.inc)[0]}
        if case.degrees[w] != case.degrees[v]:
            wrong["neighbour's angle"] = _oracle_view(orc, gt, psfs[v], case.degrees[w], case.inc)[0]
        for name, bad in wrong.items():
            assert rel_to_max(bad, want) > 100 * CONV_TOL, (v, name, rel_to_max(bad, want))
    assert len(_sensitivity_sample()) >= 12


# ------------------------------------------------------------------------------------------------ GPU
def _params(c, case, v, snr, **over):
    kw = dict(degrees=case.degrees[v], delta=REF_DELTA, inc=case.inc, snr=snr, seed=case.seed(v), stream=case.stream(v), conv_method=1,
              min_value=MIN_VALUE, target_average=TARGET)
    kw.update(over)
    return c.view_params(**kw)


class _Buffers:
    """The ground truth and one acquisition per view on the device."""

    def __init__(self, c, gt, nzo):
        self.c, self.shapes = c, [(int(k), gt.shape[1], gt.shape[2]) for k in nzo]
        self.dim = gt.shape[::-1]
        self.d_gt = c.dev_alloc(gt.nbytes)
        c.upload(self.d_gt, gt)
        self.acq = [c.dev_alloc(int(np.prod(s)) * 4) for s in self.shapes]

    def sentinel(self, views=None):
        for v in (range(len(self.acq)) if views is None else views):
            self.c.upload(self.acq[v], np.full(self.shapes[v], -1.0, np.float32))

    def fetch(self):
        return [self.c.download(a, s) for a, s in zip(self.acq, self.shapes)]

    def free(self):
        for d in [self.d_gt] + self.acq:
            self.c.dev_free(d)


def _sequential(mvs, gt, psfs, make_params, nzo, opts=None, con=None):
    """V mvsim_simulate_view_dev calls in a fresh context -> (acquisitions, the PSFs as the calls leave them)."""
    with mvs.Context(0) as c:
        for k, v in (opts or {}).items():
            c.set_option(k, v)
        b = _Buffers(c, gt, nzo)
        d_con = c.dev_alloc(gt.nbytes) if con is not None else 0
        try:
            mine = [p.copy() for p in psfs]
            for v in range(len(psfs)):
                b.sentinel([v])
                c.simulate_view_dev(b.d_gt, b.dim, mine[v], make_params(c, v), b.acq[v], con_dptr=d_con if con == v else 0)
                assert c.extract_path()[4] == 1
            return b.fetch(), mine
        finally:
            b.free()
            if d_con:
                c.dev_free(d_con)


def _stacked(c, b, psfs, make_params, expect_views):
    """One mvsim_simulate_views_dev call on sentinel-filled outputs -> (acquisitions, the PSFs as the call leaves them)."""
    b.sentinel()
    mine = [p.copy() for p in psfs]
    c.simulate_views_dev(b.d_gt, b.dim, mine, [make_params(c, v) for v in range(len(psfs))], b.acq)
    assert c.extract_path()[4] == expect_views, c.extract_path()
    return b.fetch(), mine


@pytest.mark.gpu
@pytest.mark.parametrize("case", S.cases(), ids=lambda c: c.id)
def test_stacked_views_sweep(mvs, orc, case):
    gt, psfs = _inputs(case)
    V, nzo = case.V, [case.nzo] * case.V
    want = {snr: _sequential(mvs, gt, psfs, lambda c, v, snr=snr: _params(c, case, v, snr), nzo, case.opts) for snr in (25.0, -1.0)}
    got = {}
    with mvs.Context(0) as c:
        for k, val in case.opts.items():
            c.set_option(k, val)
        b = _Buffers(c, gt, nzo)
        try:
            # a. a single view first, then the stack: the last extract served one view, then V
            c.simulate_view_dev(b.d_gt, b.dim, psfs[0].copy(), _params(c, case, 0, 25.0), b.acq[0])
            assert c.extract_path()[4] == 1
            for snr in (25.0, -1.0):
                got[snr] = _stacked(c, b, psfs, lambda c, v, snr=snr: _params(c, case, v, snr), V)
        finally:
            b.free()
    # b. bit identity with the sequential views, the PSF arrays included
    for snr in (25.0, -1.0):
        for v in range(V):
            assert _same(got[snr][0][v], want[snr][0][v]), (snr, v, float(np.mean(got[snr][0][v] != want[snr][0][v])))
            assert _same(got[snr][1][v], want[snr][1][v]), (snr, v)
            assert abs(float(got[snr][1][v].astype(np.float64).sum()) - 1.0) < 1e-6
    worst = 0.0
    for v in range(V):
        nf, noisy = got[-1.0][0][v], got[25.0][0][v]
        assert nf.shape == (case.nzo,) + case.shape[1:] and float(nf.min()) > -0.5               # no sentinel (-1) left
        # c. against the fp64 oracle
        ref, _, _ = _oracle_view(orc, gt, psfs[v], case.degrees[v], case.inc)
        assert np.isfinite(ref).all() and float(ref.max()) > 1.0                                 # a populated view: its mean is 1
        err = rel_to_max(nf, ref)
        worst = max(worst, err)
        assert err <= CONV_TOL, (v, err)
        # d. counts on identical lambda: the GPU's own noise-free planes at k * inc of an otherwise zero volume
        lam = np.zeros(case.shape, np.float32)
        lam[::case.inc] = nf
        counts = orc.extract_slices_counter(lam, case.inc, 25.0, case.seed(v), case.stream(v))
        assert _same(noisy, counts), (v, float(np.mean(noisy != counts)))
        assert float(noisy.max()) > 0
    print(f"stacked sweep {case.id}: fp64 error {worst:.3e} of the range")


# ---- workspaces across calls
def _specimen(shape, seed=77):
    """Random values confined to two middle planes and the middle quarter of y: a small angle keeps it thin (tests/test_skip_tail.py)."""
    nz, ny, nx = shape
    rng = np.random.default_rng(seed)
    v = np.zeros(shape, dtype=np.float32)
    y0, y1 = ny // 2 - ny // 8, ny // 2 + ny // 8
    for z in range(nz // 2 - 1, nz // 2 + 1):
        v[z, y0:y1, :] = rng.random((y1 - y0, nx), dtype=np.float32) + np.float32(0.25)
    return v


@pytest.mark.gpu
def test_single_sparse_view_behind_a_stack(mvs):
    """A stack of dense views with values around 1e6 leaves every workspace full of large numbers; the single sparse view behind it
    runs the fused rotate kernel with plane flags, row bits and the sparse tail, which store nothing into -- and read nothing from -- what
    they know to be empty.  Nothing of the stack may show: the view equals a fresh context's bit for bit."""
    shape, kshape, V = (24, 128, 128), (5, 5, 17), 4
    rng = np.random.default_rng(5)
    dense = (rng.random(shape, dtype=np.float32) + np.float32(0.5)) * np.float32(1e6)
    psfs = [rng.random(kshape, dtype=np.float32) + np.float32(0.05) for _ in range(V)]
    sparse, psf = _specimen(shape), rng.random(kshape, dtype=np.float32) + np.float32(0.05)
    res = {}
    for behind in (True, False):
        with mvs.Context(0) as c:
            c.set_option("fused_fftx", "roles")
            if behind:
                b = _Buffers(c, dense, [shape[0]] * V)
                try:
                    acqs, _ = _stacked(c, b, psfs, lambda c, v: c.view_params(degrees=20 + 40 * v, delta=1e-9, inc=1, snr=25.0, seed=S.SEED,
                                                                              stream=v, conv_method=1), V)
                    assert min(float(a.max()) for a in acqs) > 0
                finally:
                    b.free()
            for degrees, inc in ((0, 1), (3, 2)):
                p = c.view_params(degrees=degrees, inc=inc, snr=25.0, seed=S.SEED, stream=3, conv_method=1)
                res[behind, degrees] = c.simulate_view(sparse, psf.copy(), p)
                assert c.tail_path()[0] == 1 and c.extract_path()[4] == 1, (behind, degrees, c.tail_path())
    for degrees in (0, 3):
        assert _same(res[True, degrees]["acq"], res[False, degrees]["acq"]), degrees
        assert res[True, degrees]["corr"] == res[False, degrees]["corr"]
        assert float(res[True, degrees]["acq"].max()) > 0


@pytest.mark.gpu
def test_stacks_of_changing_geometry_in_one_context(mvs):
    """Stack A, a smaller stack B, A again, another view count each time, through one context's workspaces: every acquisition equals the
    same call in a fresh context, and A's views do not depend on how many views ran beside them."""
    rng = np.random.default_rng(11)
    geo = {"A": ((37, 40, 36), (15, 5, 7), 3), "B": ((9, 21, 18), (4, 3, 2), 2)}         # (shape, PSF shape, inc)
    gts = {k: _ground_truth(g[0], 100 + i) for i, (k, g) in enumerate(geo.items())}
    psfs = {k: [rng.random(g[1], dtype=np.float32) + np.float32(0.05) for _ in range(5)] for k, g in geo.items()}
    runs = (("A", 3), ("B", 5), ("A", 2), ("B", 2), ("A", 5))

    def params(k):
        return lambda c, v: c.view_params(degrees=(25, -70, 130, 5, -160)[v], inc=geo[k][2], snr=25.0, seed=S.SEED + v, stream=v, conv_method=1)

    def call(c, k, V):
        nzo = [(geo[k][0][0] - 1) // geo[k][2] + 1] * V
        b = _Buffers(c, gts[k], nzo)
        try:
            return _stacked(c, b, psfs[k][:V], params(k), V)[0]
        finally:
            b.free()

    with mvs.Context(0) as c:
        got = [call(c, k, V) for k, V in runs]
    for (k, V), g in zip(runs, got):
        with mvs.Context(0) as fresh:
            want = call(fresh, k, V)
        for v in range(V):
            assert _same(g[v], want[v]), (k, V, v)
            assert float(g[v].max()) > 0
    for v in range(2):
        assert _same(got[0][v], got[2][v]) and _same(got[0][v], got[4][v])


# ---- every refusal of views_batchable
_R_SHAPE, _R_KSHAPE, _R_V = (24, 26, 24), (9, 4, 3), 3
_OPTION_FREE = ("view_batch", "view_lanes", "graph")       # what does not change a view's arithmetic: the reference context leaves them alone

#   name: (context options, per-view parameter overrides {view: {...}}, Kz, view that asks for `con` or None, views, snr)
_REFUSALS = {
    "delta differs": ({}, {1: dict(delta=0.02)}, 9, None, _R_V, 25.0),
    "inc differs": ({}, {2: dict(inc=3)}, 9, None, _R_V, 25.0),
    "snr differs": ({}, {1: dict(snr=12.0)}, 9, None, _R_V, 25.0),
    "min_value differs": ({}, {0: dict(min_value=2e-4)}, 9, None, _R_V, 25.0),
    "target_average differs": ({}, {2: dict(target_average=2.0)}, 9, None, _R_V, 25.0),
    "axis 1": ({}, {1: dict(axis=1)}, 9, None, _R_V, 25.0),
    "axis 2 in every view": ({}, {v: dict(axis=2) for v in range(_R_V)}, 9, None, _R_V, 25.0),
    "con requested": ({}, {}, 9, 1, _R_V, 25.0),
    "conv_method 2": ({}, {v: dict(conv_method=2) for v in range(_R_V)}, 9, None, _R_V, 25.0),
    "Kz 65": ({}, {}, 65, None, _R_V, 25.0),
    "fft_zpass fft": ({"fft_zpass": "fft"}, {}, 9, None, _R_V, 25.0),
    "fft_zpass inline": ({"fft_zpass": "inline"}, {}, 9, None, _R_V, 25.0),
    "early_sum 0": ({"early_sum": 0}, {}, 9, None, _R_V, 25.0),
    "fuse_tail 1": ({"fuse_tail": 1}, {}, 9, None, _R_V, 25.0),
    "graph 1": ({"graph": 1}, {}, 9, None, _R_V, 25.0),
    "poisson_queue 0 with noise": ({"poisson_queue": 0}, {}, 9, None, _R_V, 25.0),
    "view_batch 0": ({"view_batch": 0}, {}, 9, None, _R_V, 25.0),
    "one view": ({}, {}, 9, None, 1, 25.0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("reason", sorted(_REFUSALS), ids=lambda r: r.replace(" ", "_"))
def test_views_the_stack_declines_run_one_by_one(mvs, reason):
    """views_batchable says no (view_lanes = 1: the views then run one after the other on the context itself): the call succeeds, the
    last extract served one view, the outputs are the sequential calls'.  Beside each, the same call made batchable reports V."""
    opts, over, kz, con, V, snr = _REFUSALS[reason]
    gt = _ground_truth(_R_SHAPE, 21)
    rng = np.random.default_rng(22)
    psfs = [rng.random((kz,) + _R_KSHAPE[1:], dtype=np.float32) + np.float32(0.05) for _ in range(V)]
    base = dict(degrees=0, delta=REF_DELTA, inc=2, snr=snr, seed=S.SEED, stream=0, conv_method=1, min_value=MIN_VALUE, target_average=TARGET)

    def params(overrides):
        def make(c, v):
            kw = dict(base, degrees=(25, -70, 130)[v], seed=S.SEED + v, stream=v + 1)
            kw.update(overrides.get(v, {}))
            return c.view_params(**kw)
        return make

    def nzo_of(overrides, views):
        return [(_R_SHAPE[0] - 1) // dict(base, **overrides.get(v, {}))["inc"] + 1 for v in range(views)]

    with mvs.Context(0) as c:
        c.set_option("view_lanes", 1)
        # the positive control: the same call without the reason -- default options, like parameters, at most 64 z taps, two views or more
        # (poisson_queue = 0 alone stays: it only refuses noisy views, so its control is the noise-free call)
        ctl_V = max(V, 2)
        ctl_psfs = [rng.random((min(kz, 64),) + _R_KSHAPE[1:], dtype=np.float32) + np.float32(0.05) for _ in range(ctl_V)]
        ctl_over = {}
        if reason == "poisson_queue 0 with noise":
            c.set_option("poisson_queue", 0)
            ctl_over = {v: dict(snr=-1.0) for v in range(ctl_V)}
        b = _Buffers(c, gt, nzo_of(ctl_over, ctl_V))
        try:
            ctl, _ = _stacked(c, b, ctl_psfs, params(ctl_over), ctl_V)
            assert all(float(a.min()) > -0.5 for a in ctl)          # no sentinel (-1) left
        finally:
            b.free()
        # the refused call
        for k, val in opts.items():
            c.set_option(k, val)
        nzo = nzo_of(over, V)
        b = _Buffers(c, gt, nzo)
        d_con = c.dev_alloc(gt.nbytes) if con is not None else 0
        try:
            b.sentinel()
            mine = [p.copy() for p in psfs]
            c.simulate_views_dev(b.d_gt, b.dim, mine, [params(over)(c, v) for v in range(V)], b.acq,
                                 con_dptrs=[d_con if v == con else 0 for v in range(V)] if con is not None else None)
            assert c.extract_path()[4] == 1, c.extract_path()
            got = b.fetch()
        finally:
            b.free()
            if d_con:
                c.dev_free(d_con)
    want, want_psfs = _sequential(mvs, gt, psfs, params(over), nzo, {k: v for k, v in opts.items() if k not in _OPTION_FREE}, con=con)
    for v in range(V):
        assert _same(got[v], want[v]), (reason, v, float(np.mean(got[v] != want[v])))
        assert _same(mine[v], want_psfs[v]) and float(got[v].min()) > -0.5 and float(got[v].max()) > 0
