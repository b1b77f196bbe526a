"""mvsim_simulate_iteration_dev -- the device-resident body of `main`'s view loop (SimulateMultiViewDataset.java:567-613; csrc/api_view.cpp)
-- swept over what tests/test_gpu_parity.py::test_main_loop_iteration_device_resident leaves unobserved (tests/iteration_cases.py).

Part 1, one iteration against the oracle, per case: all five outputs.
  acq           noise-free: within CONV_TOL = 1e-5 of the range of the fp64 oracle's view; sampled: bit-equal to mvsim_simulate_view_dev with
                the same parameters in a fresh context with the same options (that path is held to the oracle by the Poisson sweep);
  iso           bit-equal to the oracle's makeIsotropic of the GPU's acq;
  view          bit-equal to the oracle's rotateAroundAxis(GPU's iso, axis, back);
  view_psf      bit-equal to the oracle's rotateAroundAxis(normalised PSF, axis, back), and the caller's PSF comes back normalised;
  view_weights  bit-equal to mvsim_compute_weight_image_dev + mvsim_rotate_around_axis_dev on the same context, and within 2e-7 of the
                oracle's rotateAroundAxis(computeWeightImage).
The view before each case's iteration runs another PSF through the context, so that a rotate-back of stale taps shows.  Then every subset of
the optional outputs in one context, and the refusals.

Part 2, a script of 43 iterations through ONE context (iteration_cases.script): the ground truth rewritten in place through one device
pointer across the sixteen-view flag cycle of rotate_attenuate_fftx (sparse, dense, values around 1e6, all zero, all NaN), `main`'s
pattern of V angles and per-view PSFs for three rounds, PSFs that hit the cache between iterations that go round it, the size change
A -> C -> A -> release_caches -> A with the weight image asked for every time.  In four modes -- synchronised, unsynchronised (a caller's
stream, every iteration into buffers of its own, nothing downloaded before the end), option graph, psf_cache = 0 -- every output of every
iteration equals the same iteration run alone in a fresh context with the same options, bit for bit.

Part 3, on the CPU with the oracle alone: the variants a wrong implementation could plausibly produce (back with the wrong sign, the centre
of the acquisition's size instead of the isotropic volume's, the previous view's PSF, the un-normalised PSF, makeIsotropic with inc +- 1)
differ from the right answer on at least 1 % of the voxels of every case, so no case passes by symmetry.

Measured on the MI355X: the largest range-normalised error of a noise-free acq against the fp64 oracle is 2.13e-07 (inc1-nz13), the others
5.8e-08 .. 2.08e-07; every rotated weight image equals the oracle's bit for bit.  The script, per mode (flagged / unflagged views at the
flagged shape, graph replays, PSF cache hits / misses at the end): synchronised 6 / 16 and the unsampled NaN volume, 0, 30 / 6;
unsynchronised 20 / 2 (the hint lags the enqueue), 0, 30 / 6; graph 23 / 0 (the captured view carries flags), 27, 0 / 0; psf_cache = 0
6 / 16, 0, 0 / 0.  With the isotropic view rotated about the centre of `dim` instead of its own, the seven part-1 cases whose two centres
differ fail (axis0-B, axis1-B, inc3-nz17, inc4-nz12, inc3-nz12, both flagged 3-degree cases); with the weight image kept across a change
of size, every mode of the script fails at the first view behind the flagged shape, in view_weights."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from . import iteration_cases as I
from .conftest import rel_to_max

CONV_TOL = 1e-5          # range-normalised: the project's contract (tests/test_conv_sweep.py)
WEIGHT_TOL = 2e-7        # test_main_loop_iteration_device_resident's bound on the rotated weight image
CASES = I.cases()
BASE = {"fused_fftx": "roles"}                       # part 2: the flagged shape forced onto the fused rotate kernel
MODES = {"sync": {}, "unsync": {}, "graph": {"graph": 1}, "nocache": {"psf_cache": 0}}


def _same(a, b):
    """np.array_equal on the bit patterns (tests/test_row_bits.py): NaN equals itself, +0 is not -0."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


class Dev:
    """Device allocations, each `offset` floats past its own (256-byte aligned) base, as tests/test_deconvolve.py places them."""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def alloc(self, shape, offset=0):
        base = self.ctx.dev_alloc(int(np.prod(shape)) * 4 + 4 * offset + 64)
        assert base % 16 == 0
        self.ptrs.append(base)
        return base + 4 * offset

    def put(self, a, offset=0):
        a = np.ascontiguousarray(a, dtype=np.float32)
        p = self.alloc(a.shape, offset)
        self.ctx.upload(p, a)
        return p

    def free(self):
        self.ctx.synchronize()
        for p in self.ptrs:
            self.ctx.dev_free(p)
        self.ptrs = []


def _iterate(c, d_gt, dim, psf, params, back, ptr):
    """One mvsim_simulate_iteration_dev into the buffers `ptr` names (acq and any of the optional four)."""
    c.simulate_iteration_dev(d_gt, dim, psf, params, back, ptr["acq"], iso_dptr=ptr.get("iso", 0), view_dptr=ptr.get("view", 0),
                             view_weights_dptr=ptr.get("view_weights", 0), view_psf_dptr=ptr.get("view_psf", 0))


def _params(c, x):
    """ViewParams of a Case or a Step."""
    kw = dict(axis=x.axis, degrees=x.degrees, inc=x.inc, snr=x.snr, seed=x.seed, stream=x.stream, conv_method=getattr(x, "conv_method", 1))
    if hasattr(x, "delta"):
        kw["delta"] = x.delta
    return c.view_params(**kw)


# ------------------------------------------------------------------------------------------------ CPU: the table and its inputs
def test_every_target_is_covered_by_a_case_that_lands_on_it():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    claimed = set()
    for c in CASES:
        assert c.shape[2] <= c.shape[1], c.name                          # the view pipeline refuses Nx > Ny
        assert c.targets and set(c.targets) <= set(I.TARGETS), c.name
        assert set(c.targets) <= I.landing(c), (c.name, set(c.targets) - I.landing(c))
        claimed |= set(c.targets)
    assert claimed == set(I.TARGETS), set(I.TARGETS) - claimed
    # the issue's own values
    assert {c.shape for c in CASES} >= {(13, 22, 20), (11, 13, 9), (24, 128, 128)}
    assert {c.kshape for c in CASES} >= {(4, 5, 3), (3, 6, 5), (5, 5, 17)}
    assert {(c.inc, c.shape[0]) for c in CASES} >= {(i, 13) for i in (1, 2, 3, 4)} | {(2, 12), (4, 12), (3, 17)}


def test_the_script_holds_what_the_issue_asks_for():
    steps = I.script()
    its = [s for s in steps if s is not I.RELEASE]
    assert len(its) >= 36
    # three rounds of main's pattern, back = -angle, per-view PSFs
    main = [s for s in its if s.shape == I.A_SHAPE and s.degrees in I.A_ANGLES and s.back == -s.degrees]
    assert len(main) == 3 * len(I.A_ANGLES) and len({s.psf for s in main}) == len(I.A_ANGLES)
    assert main[:4] == main[4:8] == main[8:]
    # view_psf interleaved with iterations that do not ask for it; PSFs that repeat next to PSFs seen once
    kinds = ["view_psf" in s.wants for s in its]
    assert any(a and not b for a, b in zip(kinds, kinds[1:])) and any(b and not a for a, b in zip(kinds, kinds[1:]))
    count = {}
    for s in its:
        count[s.psf] = count.get(s.psf, 0) + 1
    assert 1 in count.values() and max(count.values()) > 1
    # the flag cycle: sparse, other sparse, dense, sixteen sparse volumes of distinct empty-plane counts, 1e6, zero, sparse; one NaN volume
    f = [s for s in its if s.shape == I.F_SHAPE]
    names = [s.gt for s in f]
    assert names[:3] == ["f-sparse-a", "f-sparse-b", "f-dense"] and names[-3:] == ["f-loud", "f-zero", "f-sparse-a"]
    middle = [n for n in names[3:-3] if n != "f-nan"]
    assert len(middle) == 16 and len({I.empty_planes(n) for n in middle}) == 16
    assert names.count("f-nan") == 1 and all(s.snr < 0 for s in f if s.gt == "f-nan")
    after_nan = f[names.index("f-nan") + 1]
    assert after_nan.snr >= 0 and 0 < I.empty_planes(after_nan.gt) < I.F_SHAPE[0]
    assert len({(s.degrees, s.back, s.inc, s.seed, s.stream, s.delta, s.psf) for s in f}) == 1          # one key: replays on changed contents
    # A -> C -> A -> release -> A with the weight image every time
    k = steps.index(I.RELEASE)
    assert [s.shape for s in steps[k - 3:k]] == [I.A_SHAPE, I.C_SHAPE, I.A_SHAPE] and steps[k + 1].shape == I.A_SHAPE
    assert all("view_weights" in s.wants for s in steps[k - 3:k] + [steps[k + 1]])


_ORACLE = {}


def _oracle(orc, synth, case):
    """The oracle's iteration of a case, computed once, shared, never written to."""
    if case.name not in _ORACLE:
        gt, psf, prev = I.case_inputs(synth, case)
        pn = psf.copy()
        orc.norm_image(pn)
        view = orc.simulate_view(gt, psf.copy(), case.degrees, axis=case.axis, inc=case.inc, snr=case.snr, seed=case.seed, stream=case.stream)
        _ORACLE[case.name] = {"acq": view["acq"], "pn": pn, "gt": gt, "psf": psf, "prev": prev}
    return _ORACLE[case.name]


def _differ(a, b):
    """Share of voxels on which two volumes differ (over the planes both have)."""
    n = min(a.shape[0], b.shape[0])
    return float(np.mean(a[:n] != b[:n]))


def _wrong_centre(orc, iso, nz, axis, back):
    """rotateAroundAxis of `iso` about the centre of a volume of nz planes, (nz - 1) / 2 in integer arithmetic, instead of its own: the
    volume padded with empty planes (outside is zero anyway) until its centre plane is that one, rotated, cropped."""
    niso = iso.shape[0]
    want = (nz - 1) // 2
    n = next(m for m in (2 * want + 1, 2 * want + 2) if m >= niso)
    assert (n - 1) // 2 == want
    pad = np.zeros((n,) + iso.shape[1:], dtype=np.float32)
    pad[:niso] = iso
    return orc.rotate_around_axis(pad, axis, back)[:niso]


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_wrong_variants_show_on_the_oracle(orc, synth, case):
    o = _oracle(orc, synth, case)
    acq, pn = o["acq"], o["pn"]
    assert abs(float(pn.sum(dtype=np.float64)) - 1.0) < 1e-5 and not _same(pn, o["psf"])
    iso = orc.make_isotropic(acq, case.inc)
    assert iso.shape[0] == case.niso
    view = orc.rotate_around_axis(iso, case.axis, case.back)
    vpsf = orc.rotate_around_axis(pn, case.axis, case.back)
    vw = orc.rotate_around_axis(orc.compute_weight_image(case.shape), case.axis, case.back)
    floor = 0.01
    if case.back not in (0, 180):
        assert _differ(orc.rotate_around_axis(iso, case.axis, -case.back), view) >= floor
        assert _differ(orc.rotate_around_axis(pn, case.axis, -case.back), vpsf) >= floor
        assert _differ(orc.rotate_around_axis(orc.compute_weight_image(case.shape), case.axis, -case.back), vw) >= floor
    if (case.niso - 1) // 2 != (case.shape[0] - 1) // 2 and case.axis != 2 and case.back != 0:      # (about z the z centre is not used)
        assert _differ(_wrong_centre(orc, iso, case.shape[0], case.axis, case.back), view) >= floor
    pprev = o["prev"].copy()
    orc.norm_image(pprev)
    assert _differ(orc.rotate_around_axis(pprev, case.axis, case.back), vpsf) >= floor
    assert _differ(orc.rotate_around_axis(o["psf"], case.axis, case.back), vpsf) >= floor
    for inc in (case.inc - 1, case.inc + 1):
        if inc >= 1:
            other = orc.make_isotropic(acq, inc)
            assert other.shape[0] != iso.shape[0] or case.nzo == 1
            assert _differ(other, iso) >= floor, inc


# ------------------------------------------------------------------------------------------------ part 1 on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_one_iteration_against_the_oracle(mvs, orc, synth, case):
    o = _oracle(orc, synth, case)
    gt, psf, prev, pn = o["gt"], o["psf"], o["prev"], o["pn"]
    shapes = case.out_shapes()
    nz, ny, nx = case.shape
    with mvs.Context(0) as c:
        for k, v in case.opts.items():
            c.set_option(k, v)
        dev = Dev(c)
        try:
            d_gt = dev.put(gt)
            ptr = {k: dev.alloc(s, case.offsets.get(k, 0)) for k, s in shapes.items()}
            p = _params(c, case)
            # the view before this one: another PSF through ctx->psf_dev
            _iterate(c, d_gt, case.dim, prev.copy(), p, case.back, {"acq": ptr["acq"], "view_psf": ptr["view_psf"]})
            praw = psf.copy()
            _iterate(c, d_gt, case.dim, praw, p, case.back, ptr)
            got = {k: c.download(ptr[k], s) for k, s in shapes.items()}
            tail, planes = c.tail_path(), c.plane_stats()
            d_w, d_wr = dev.alloc(case.shape), dev.alloc(case.shape)
            c.compute_weight_image_dev(case.dim, d_w)
            c.rotate_around_axis_dev(d_w, case.dim, case.axis, case.back, d_wr)
            chained = c.download(d_wr, case.shape)
        finally:
            dev.free()
    assert _same(praw, pn)                                               # the caller's PSF comes back normalised (Q5)
    if case.snr < 0:
        err = rel_to_max(got["acq"], o["acq"])
        print(f"{case.name}: acq against the fp64 oracle, range-normalised {err:.3e}")
        assert err <= CONV_TOL
    else:
        with mvs.Context(0) as c:
            for k, v in case.opts.items():
                c.set_option(k, v)
            dev = Dev(c)
            try:
                d_gt, d_acq = dev.put(gt), dev.alloc(shapes["acq"], case.offsets.get("acq", 0))
                c.simulate_view_dev(d_gt, case.dim, psf.copy(), _params(c, case), d_acq)
                alone = c.download(d_acq, shapes["acq"])
            finally:
                dev.free()
        assert _same(got["acq"], alone)
        assert float(got["acq"].max()) > 0
    if case.specimen == "slab":                                          # the acquisition came from the sparse tail, planes were skipped
        assert tail[0] == 1 and tail[1] in (1, case.inc), tail
        assert planes[0] == nz and planes[1] > 0 and planes[2] > 0, planes
    # behind the view everything is bit-exact on identical input: feed the oracle what the GPU produced
    assert _same(got["iso"], orc.make_isotropic(got["acq"], case.inc))
    assert _same(got["view"], orc.rotate_around_axis(got["iso"], case.axis, case.back))
    assert _same(got["view_psf"], orc.rotate_around_axis(pn, case.axis, case.back))
    assert _same(got["view_weights"], chained)
    werr = float(np.abs(got["view_weights"] - orc.rotate_around_axis(orc.compute_weight_image(case.shape), case.axis, case.back)).max())
    print(f"{case.name}: rotated weight image against the oracle {werr:.3e}")
    assert werr <= WEIGHT_TOL


@pytest.mark.gpu
def test_every_subset_of_the_optional_outputs(mvs, synth):
    """The 16 subsets of {iso, view, view_weights, view_psf} one after the other in ONE context, the PSF alternating: `view` without `iso`
    goes through the vol_c scratch, view_psf or not decides whether the view goes round the PSF cache.  acq and every output asked for
    equal the all-outputs run of that PSF; a buffer not asked for keeps what it held."""
    shape, kshape = I.A_SHAPE, I.A_PSF
    gt = I.phantom(synth, shape, 94)
    psfs = [I.random_psf(kshape, 800), I.random_psf(kshape, 801)]
    step = I.Step(shape, "gt", 0, kshape, 33, -33, I.OUTPUTS, inc=2, snr=25.0, stream=2)
    shapes = step.out_shapes()
    mark = {k: np.full(s, -7.0, dtype=np.float32) for k, s in shapes.items()}
    want = []
    for psf in psfs:
        with mvs.Context(0) as c:
            dev = Dev(c)
            try:
                ptr = {k: dev.alloc(s) for k, s in shapes.items()}
                _iterate(c, dev.put(gt), step.dim, psf.copy(), _params(c, step), step.back, ptr)
                want.append({k: c.download(ptr[k], s) for k, s in shapes.items()})
            finally:
                dev.free()
    assert not _same(want[0]["acq"], want[1]["acq"]) and not _same(want[0]["view_psf"], want[1]["view_psf"])
    with mvs.Context(0) as c:
        dev = Dev(c)
        try:
            d_gt = dev.put(gt)
            ptr = {k: dev.alloc(s) for k, s in shapes.items()}
            p = _params(c, step)
            moved = []
            for bits in range(16):
                asked = tuple(k for i, k in enumerate(I.OUTPUTS) if bits >> i & 1)
                for k in shapes:
                    c.upload(ptr[k], mark[k])
                before = c.psf_cache_stats()
                _iterate(c, d_gt, step.dim, psfs[bits % 2].copy(), p, step.back, {k: ptr[k] for k in ("acq",) + asked})
                after = c.psf_cache_stats()
                moved.append((after["hits"] + after["misses"]) - (before["hits"] + before["misses"]))
                assert moved[-1] == (0 if "view_psf" in asked else 1), (asked, before, after)
                for k, s in shapes.items():
                    got = c.download(ptr[k], s)
                    assert _same(got, want[bits % 2][k] if k == "acq" or k in asked else mark[k]), (asked, k)
            assert c.psf_cache_stats()["hits"] == 6 and c.psf_cache_stats()["misses"] == 2
        finally:
            dev.free()


@pytest.mark.gpu
def test_refusals(mvs, synth):
    """iso == view, a null `more`, Nx > Ny."""
    shape, kshape = I.A_SHAPE, I.A_PSF
    gt, psf = I.phantom(synth, shape, 94), I.random_psf(kshape, 800)
    step = I.Step(shape, "gt", 0, kshape, 33, -33, I.OUTPUTS, inc=2, snr=-1.0)
    shapes = step.out_shapes()
    with mvs.Context(0) as c:
        dev = Dev(c)
        try:
            d_gt = dev.put(gt)
            ptr = {k: dev.alloc(s) for k, s in shapes.items()}
            p = _params(c, step)
            with pytest.raises(Exception, match="different buffers"):
                _iterate(c, d_gt, step.dim, psf.copy(), p, step.back, {"acq": ptr["acq"], "iso": ptr["iso"], "view": ptr["iso"]})
            o = mvs._lib.ViewOutputs(None, None, None, ptr["acq"])
            pc = psf.copy()
            rc = c._L.mvsim_simulate_iteration_dev(c._h, C.c_void_p(d_gt), (C.c_int64 * 3)(*step.dim), pc.ctypes.data_as(C.c_void_p),
                                                   (C.c_int64 * 3)(*kshape[::-1]), C.byref(p), step.back, C.byref(o), None)
            assert rc != 0 and _same(pc, psf)                            # refused before anything was touched
            wide = I.Step((13, 20, 22), "gt", 0, kshape, 33, -33, ("iso",), inc=2, snr=-1.0)
            with pytest.raises(Exception, match="Nx > Ny"):
                _iterate(c, d_gt, wide.dim, psf.copy(), p, wide.back, {"acq": ptr["acq"], "iso": ptr["iso"]})
            # the context is still good for a whole iteration
            _iterate(c, d_gt, step.dim, psf.copy(), p, step.back, ptr)
            assert np.isfinite(c.download(ptr["view"], shapes["view"])).all()
        finally:
            dev.free()


# ------------------------------------------------------------------------------------------------ part 2: one context, many iterations
_FRESH = {}
_VOLUMES = {}
MARKER_DIM = (4, 4, 1)


def _volumes(synth):
    if not _VOLUMES:
        _VOLUMES.update(I.volumes(synth))
    return _VOLUMES


def _options(mode):
    return dict(BASE, **MODES[mode])


def _fresh(mvs, synth, opts, step):
    """The iteration alone in a fresh context with these options: computed once per (options, iteration), shared, never written to."""
    key = (tuple(sorted((k, str(v)) for k, v in opts.items())), step)
    if key not in _FRESH:
        with mvs.Context(0) as c:
            for k, v in opts.items():
                c.set_option(k, v)
            dev = Dev(c)
            try:
                d_gt = dev.put(_volumes(synth)[step.gt])
                shapes = step.out_shapes()
                ptr = {k: dev.alloc(s) for k, s in shapes.items()}
                _iterate(c, d_gt, step.dim, I.random_psf(step.kshape, step.psf), _params(c, step), step.back, ptr)
                res = {k: c.download(ptr[k], s) for k, s in shapes.items()}
                res["path"] = c.extract_path()
                _FRESH[key] = res
            finally:
                dev.free()
    return _FRESH[key]


def _flag_model(f_steps):
    """What the comment in rotate_attenuate_fftx promises for synchronised views: the first view carries flags; a view carries them while
    the last flagged view reported empty planes; behind one that reported none, fifteen run without and the sixteenth carries them again."""
    hint, since, out = -1, 0, []
    for s in f_steps:
        flagged = not (hint == 0 and since < 15)
        since = 0 if flagged else since + 1
        if flagged:
            hint = I.empty_planes(s.gt)
        out.append(flagged)
    return out


class _CacheModel:
    """Hits and misses of the PSF cache the script's order implies (content and geometry; release_caches empties it)."""

    def __init__(self):
        self.seen, self.hits, self.misses = set(), 0, 0

    def step(self, s):
        if "view_psf" in s.wants:
            return
        key = (s.psf, s.kshape, s.shape)
        if key in self.seen:
            self.hits += 1
        else:
            self.misses += 1
            self.seen.add(key)


def _flagged(s, replayed, tail, planes, log):
    """Did this view carry plane flags?  A sampled view the host enqueued: its tail ran sparse.  A replayed or an unsampled one: the plane
    statistics are its own -- None where that cannot be told, the view before it having left the same."""
    if s.shape != I.F_SHAPE:
        return False
    if not replayed and s.snr >= 0:
        return tail[0] == 1
    own = planes[:2] == (s.shape[0], I.empty_planes(s.gt))
    return None if own and log and log[-1]["planes"] == planes else own


def _report(mode, log, stats, n):
    f = [e for e in log if e["step"].shape == I.F_SHAPE]
    print(f"iteration script, mode {mode}: {n} iterations; at the flagged shape {sum(e['flagged'] is True for e in f)} ran flagged, "
          f"{sum(e['flagged'] is False for e in f)} unflagged, {sum(e['flagged'] is None for e in f)} not told (of {len(f)}); "
          f"graph replays {sum(e['replayed'] for e in log)}; "
          f"PSF cache at the end hits {stats['hits']} misses {stats['misses']} evictions {stats['evictions']} bytes {stats['bytes']}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("sync", "graph", "nocache"))
def test_many_iterations_through_one_context(mvs, synth, mode):
    """Synchronised: every iteration is downloaded and compared before the next is enqueued.  One output buffer set per distinct set of
    parameters, whatever the ground truth buffer holds, so that option graph meets the same key again: first sight eager, second captured,
    later ones replayed -- on what the buffer holds by then.

    A replay is told from a view the host enqueued by mvsim_get_extract_path: a one-plane extract in front of every iteration leaves its
    own path there, a view the host enqueues overwrites it, a replayed graph cannot."""
    opts, vols, steps = _options(mode), _volumes(synth), I.script()
    model, log = _CacheModel(), []
    with mvs.Context(0) as c:
        for k, v in opts.items():
            c.set_option(k, v)
        dev = Dev(c)
        try:
            d_gt = dev.alloc(I.F_SHAPE)
            m_in, m_out = dev.put(np.ones(MARKER_DIM[::-1], dtype=np.float32)), dev.alloc(MARKER_DIM[::-1])
            bufs, held = {}, None
            for i, s in enumerate(steps):
                if s is I.RELEASE:
                    c.release_caches()
                    model.seen.clear()
                    continue
                want = _fresh(mvs, synth, opts, s)
                if s.gt != held:
                    c.upload(d_gt, vols[s.gt])                           # rewritten in place, the same device pointer
                    held = s.gt
                slot = dataclasses.replace(s, gt="")                     # what a captured view is keyed by, but not what the buffer holds
                if slot not in bufs:
                    bufs[slot] = {k: dev.alloc(shape) for k, shape in s.out_shapes().items()}
                c.extract_slices_dev(m_in, MARKER_DIM, 1, -1.0, 0, 0, m_out)
                marker = c.extract_path()
                assert marker != want["path"]
                before = c.psf_cache_stats()
                _iterate(c, d_gt, s.dim, I.random_psf(s.kshape, s.psf), _params(c, s), s.back, bufs[slot])
                after = c.psf_cache_stats()
                got = {k: c.download(bufs[slot][k], shape) for k, shape in s.out_shapes().items()}
                path, tail, planes = c.extract_path(), c.tail_path(), c.plane_stats()
                for k in got:
                    assert _same(got[k], want[k]), (mode, i, s.gt, k)
                replayed = path == marker
                if not replayed:
                    assert path == want["path"], (i, path, want["path"])
                model.step(s)
                if mode == "sync":
                    assert (after["hits"], after["misses"]) == (model.hits, model.misses), (i, after)
                    moved = (after["hits"] - before["hits"]) + (after["misses"] - before["misses"])
                    assert moved == (0 if "view_psf" in s.wants else 1), (i, before, after)
                else:                                                    # a captured graph holds pointers; psf_cache = 0
                    assert (after["hits"], after["misses"], after["bytes"]) == (0, 0, 0), (i, after)
                log.append(dict(step=s, replayed=replayed, tail=tail, planes=planes, flagged=_flagged(s, replayed, tail, planes, log)))
            stats = c.psf_cache_stats()
        finally:
            dev.free()
    _report(mode, log, stats, I.n_iterations(steps))
    replays = sum(e["replayed"] for e in log)
    f = [e for e in log if e["step"].shape == I.F_SHAPE]
    if mode == "graph":
        # round three of main's pattern replays what round two captured; so does the flagged shape from its third view on
        main = [e for e in log if e["step"].shape == I.A_SHAPE and e["step"].degrees in I.A_ANGLES]
        assert [e["replayed"] for e in main] == [False] * 8 + [True] * 4
        assert sum(e["replayed"] for e in f) >= 16 and any(e["replayed"] and e["step"].gt == "f-loud" for e in f)
        return
    assert replays == 0
    # the sixteen-view flag cycle, as the comment in rotate_attenuate_fftx promises it
    expect = _flag_model([e["step"] for e in f])
    assert expect == [True] * 3 + [False] * 15 + [True] * 3 + [False] * 2
    for k, (e, flagged) in enumerate(zip(f, expect)):
        s = e["step"]
        if flagged:
            assert e["planes"][:2] == (I.F_SHAPE[0], I.empty_planes(s.gt)), (k, s.gt, e["planes"])         # its own count
            assert s.snr < 0 or e["tail"][0] == 1, (k, s.gt, e["tail"])
            assert (e["planes"][2] > 0) == (I.empty_planes(s.gt) > 0), (k, s.gt, e["planes"])      # (every sparse run here leaves > Kz - 1 empty)
        else:
            assert e["planes"] == f[k - 1]["planes"] and e["planes"][1] == 0, (k, s.gt, e["planes"])       # the stats do not move
            assert e["tail"][0] == 0, (k, s.gt, e["tail"])
    assert all(e["planes"] == f[-1]["planes"] for e in log[len(f):])                                        # small views carry no flags



@pytest.mark.gpu
def test_many_iterations_unsynchronised(mvs, synth):
    """The script enqueued on a caller's stream with no host synchronisation between iterations: the ground truth rewritten by
    device-to-device copies on that stream, every iteration into output buffers of its own, nothing downloaded before the end (the one
    wait inside is mvsim_release_caches' own).  Nothing about flags is asserted -- the hint is read without waiting -- only the outputs,
    and the PSF cache's counters, which the host keeps."""
    opts, vols, steps = _options("unsync"), _volumes(synth), I.script()
    hip = C.CDLL("libamdhip64.so")                                       # the runtime libmvsim.so itself is linked against
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    model, log, outs = _CacheModel(), [], []
    try:
        with mvs.Context(0) as c:
            for k, v in opts.items():
                c.set_option(k, v)
            dev = Dev(c)
            try:
                staged = {name: dev.put(vols[name]) for name in {s.gt for s in steps if s is not I.RELEASE}}
                d_gt = dev.alloc(I.F_SHAPE)
                for s in steps:                                          # every buffer before the first iteration: no allocation of ours between them
                    outs.append(None if s is I.RELEASE else {k: dev.alloc(shape) for k, shape in s.out_shapes().items()})
                c.synchronize()
                c.set_stream(stream.value)
                held = None
                for s, ptr in zip(steps, outs):
                    if s is I.RELEASE:
                        c.release_caches()
                        model.seen.clear()
                        continue
                    if s.gt != held:
                        assert hip.hipMemcpyAsync(d_gt, staged[s.gt], vols[s.gt].nbytes, 3, stream) == 0      # 3: device to device
                        held = s.gt
                    before = c.psf_cache_stats()
                    _iterate(c, d_gt, s.dim, I.random_psf(s.kshape, s.psf), _params(c, s), s.back, ptr)
                    after = c.psf_cache_stats()
                    model.step(s)
                    assert (after["hits"], after["misses"]) == (model.hits, model.misses), (s.gt, after)
                    moved = (after["hits"] - before["hits"]) + (after["misses"] - before["misses"])
                    assert moved == (0 if "view_psf" in s.wants else 1), (s.gt, before, after)
                    log.append(dict(step=s, replayed=False, flagged=c.tail_path()[0] == 1 if s.snr >= 0 else None))   # the host's decision at enqueue time
                c.synchronize()
                stats = c.psf_cache_stats()
                for i, (s, ptr) in enumerate(zip(steps, outs)):
                    if s is I.RELEASE:
                        continue
                    want = _fresh(mvs, synth, opts, s)
                    for k, shape in s.out_shapes().items():
                        assert _same(c.download(ptr[k], shape), want[k]), (i, s.gt, k)
                c.set_stream(None)
            finally:
                dev.free()
    finally:
        assert hip.hipStreamDestroy(stream) == 0
    _report("unsync", log, stats, I.n_iterations(steps))
