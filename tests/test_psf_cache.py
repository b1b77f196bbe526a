"""PSF spectra cached by content (option psf_cache, csrc/psf_cache.h).  A whole single view on the direct z pass whose
normalised PSF and geometry the context has seen uploads no PSF and launches neither PSF pass; the z pass reads the spectrum the first
such view computed.  Exact: every acquisition and adjustImage factor equals psf_cache = 0 bit for bit, and mvsim_get_psf_cache_stats
counts what the sequence of calls says.

Volumes are (nz, ny, nx) = (24, 128, 128), the smallest the fused rotate kernel takes (tests/test_skip_tail.py), forced onto it with
fused_fftx = roles; PSFs are 7 x 7 x 5 and 15^3.  One case runs at (64, 512, 512) = 2^24 voxels, the threshold from which the PSF's passes
and k_plane_flags_finish run on the side stream: only there a hit has a fork to keep (flagged views) or to drop (views without flags).
The policy itself -- LRU order, the cap, equal hashes of different contents -- runs on the CPU in tests/c_abi/psf_cache_main.cpp."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

SEED = 464232194
SHAPE = (24, 128, 128)
OTHER_SHAPE = (24, 144, 140)
PSF_SMALL, PSF_LARGE = (5, 7, 7), (15, 15, 15)      # (kz, ky, kx)
BASE = {"fused_fftx": "roles"}
MIB = 1 << 20


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _specimen(shape=SHAPE, seed=91, planes=None, offset=0.0):
    """Random values in a few middle planes, the middle quarter of y (a flagged view with empty planes); offset > 0: no empty voxel."""
    nz, ny, nx = shape
    rng = np.random.default_rng(seed)
    v = np.full(shape, offset, dtype=np.float32)
    for z in (range(nz // 2 - 2, nz // 2 + 2) if planes is None else planes):
        v[z, ny // 2 - ny // 8:ny // 2 + ny // 8, :] += rng.random((ny // 8 * 2, nx), dtype=np.float32) + np.float32(0.25)
    return v


def _psf(kshape, seed=0):
    return np.random.default_rng(900 + seed).random(kshape, dtype=np.float32) + np.float32(0.05)


def _view(c, gt, psf_raw, degrees=0, inc=1, **params):
    """One host-buffer view; the PSF array it was given comes back too (normalised in place)."""
    p = c.view_params(degrees=degrees, inc=inc, snr=25.0, seed=SEED, stream=3, conv_method=params.pop("conv_method", 1), **params)
    psf = psf_raw.copy()
    res = c.simulate_view(gt, psf, p, want=("acq",))
    return {"acq": res["acq"], "corr": res["corr"], "psf": psf}


def _ctx(mvs, cache, options=None):
    c = mvs.Context(0)
    for k, v in dict(BASE, **(options or {})).items():
        c.set_option(k, v)
    c.set_option("psf_cache", cache)
    return c


def _equal(a, b):
    return _same(a["acq"], b["acq"]) and a["corr"] == b["corr"] and _same(a["psf"], b["psf"])


_OFF = {}


def _off(mvs, name, gt, psf_raw, options=None, **kw):
    """The view with psf_cache = 0 in a context of its own: computed once per name, shared, never written to."""
    if name not in _OFF:
        with _ctx(mvs, 0, options) as c:
            _OFF[name] = _view(c, gt, psf_raw, **kw)
            assert c.psf_cache_stats() == dict(hits=0, misses=0, evictions=0, bytes=0)
    return _OFF[name]


def _stats(c):
    s = c.psf_cache_stats()
    return s["hits"], s["misses"], s["evictions"]


def test_psf_cache_policy_on_the_cpu(mvs, tmp_path):
    """tests/c_abi/psf_cache_main.cpp: csrc/psf_cache.h compiled by plain g++ under ASan + UBSan (no HIP, no libmvsim.so; a child process,
    nothing preloaded): LRU order, the byte cap, equal-hash different-content as a miss, every key field, release."""
    exe = str(tmp_path / "psf_cache_main")
    cmd = [shutil.which("g++") or "g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
           "-Wextra", "-Werror", "-I" + os.path.join(os.path.dirname(os.path.abspath(mvs.__file__)), "csrc"),
           os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_abi", "psf_cache_main.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "psf cache ok:" in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-4000:]


@pytest.mark.gpu
@pytest.mark.parametrize("kshape,other", [(PSF_SMALL, PSF_LARGE), (PSF_LARGE, PSF_SMALL)])
def test_hit_is_identical_and_normalises_in_place(mvs, kshape, other):
    """The same PSF twice: one miss, one hit; acquisition, factor and the caller's normalised array are those of psf_cache = 0 -- also
    after a view with another PSF and values around 1e6 has been through every workspace in between."""
    gt, a, b = _specimen(), _psf(kshape), _psf(other, 1)
    loud = _specimen(seed=92, offset=1.0) * np.float32(1e6)
    off_a, off_loud = _off(mvs, ("a", kshape), gt, a), _off(mvs, ("loud", other), loud, b)
    with _ctx(mvs, 1024) as c:
        first = _view(c, gt, a)
        assert _stats(c) == (0, 1, 0) and c.psf_cache_stats()["bytes"] > 0
        second = _view(c, gt, a)
        assert _stats(c) == (1, 1, 0)
        held = c.psf_cache_stats()["bytes"]
        between = _view(c, loud, b)
        assert _stats(c) == (1, 2, 0) and c.psf_cache_stats()["bytes"] > held
        third = _view(c, gt, a)
        assert _stats(c) == (2, 2, 0)
        again = _view(c, loud, b)
        assert _stats(c) == (3, 2, 0)
    assert not _same(a, first["psf"])                       # the raw PSF was not normalised: the call did that, in place, hit or miss
    for got in (first, second, third):
        assert _equal(got, off_a)
    assert _equal(between, off_loud) and _equal(again, off_loud)


@pytest.mark.gpu
def test_one_ulp_in_one_tap_is_a_miss(mvs):
    """A PSF one ulp away from a cached one in one tap is a miss and gives the psf_cache = 0 result of THAT PSF."""
    gt, a = _specimen(), _psf(PSF_SMALL)
    b = a.copy()
    b[2, 3, 3] = np.nextafter(b[2, 3, 3], np.float32(2.0))
    off_a, off_b = _off(mvs, ("a", PSF_SMALL), gt, a), _off(mvs, ("ulp", PSF_SMALL), gt, b)
    assert not _same(off_a["psf"], off_b["psf"])            # (the normalised taps -- the key -- differ too)
    with _ctx(mvs, 1024) as c:
        one = _view(c, gt, a)
        two = _view(c, gt, b)
        assert _stats(c) == (0, 2, 0)
        three = _view(c, gt, a)
        four = _view(c, gt, b)
        assert _stats(c) == (2, 2, 0)
    assert _equal(one, off_a) and _equal(three, off_a)
    assert _equal(two, off_b) and _equal(four, off_b)


@pytest.mark.gpu
def test_eviction_under_a_cap_of_one_entry(mvs):
    """A, B, A, B under a cap that holds one entry: four misses, three evictions, every result that of psf_cache = 0."""
    gt, a, b = _specimen(), _psf(PSF_LARGE), _psf(PSF_LARGE, 1)
    off_a, off_b = _off(mvs, ("a", PSF_LARGE), gt, a), _off(mvs, ("b", PSF_LARGE), gt, b)
    with _ctx(mvs, 1024) as c:
        _view(c, gt, a)
        entry = c.psf_cache_stats()["bytes"]
    cap = math.ceil(entry / MIB)
    assert entry <= cap * MIB < 2 * entry, (entry, cap)     # one entry fits, two do not
    with _ctx(mvs, cap) as c:
        got = [_view(c, gt, p) for p in (a, b, a, b)]
        assert _stats(c) == (0, 4, 3) and c.psf_cache_stats()["bytes"] == entry
        got.append(_view(c, gt, b))                         # the survivor is the last one in
        assert _stats(c) == (1, 4, 3)
    for g, want in zip(got, (off_a, off_b, off_a, off_b, off_b)):
        assert _equal(g, want)


@pytest.mark.gpu
def test_other_geometry_or_plan_is_never_a_stale_hit(mvs):
    """The same PSF at another volume size misses; options that change the plan (fft_zpass) or leave the hand-written passes (rocFFT,
    with and without fft_pad) bypass the cache; fft_pad on the hand-written path changes nothing the spectrum depends on.  Every result
    is that of psf_cache = 0 under the same options."""
    a = _psf(PSF_SMALL)
    gt, gt2 = _specimen(), _specimen(OTHER_SHAPE, seed=93)
    with _ctx(mvs, 1024) as c:
        assert _equal(_view(c, gt, a), _off(mvs, ("a", PSF_SMALL), gt, a))
        assert _stats(c) == (0, 1, 0)
        assert _equal(_view(c, gt2, a), _off(mvs, ("a144", PSF_SMALL), gt2, a))
        assert _stats(c) == (0, 2, 0)
        assert _equal(_view(c, gt, a), _off(mvs, ("a", PSF_SMALL), gt, a))
        assert _equal(_view(c, gt2, a), _off(mvs, ("a144", PSF_SMALL), gt2, a))
        assert _stats(c) == (2, 2, 0)
        for i, opts in enumerate(({"fft_zpass": "fft"}, {"fft_zpass": "inline"}, {"fft_backend": "rocfft"},
                                  {"fft_backend": "rocfft", "fft_pad": "160,160,48"})):
            for k, v in opts.items():
                c.set_option(k, v)
            assert _equal(_view(c, gt, a), _off(mvs, ("a", PSF_SMALL, i), gt, a, options=opts)), opts
            assert _stats(c) == (2, 2, 0), opts             # a bypass: the counters stay
            c.set_option("fft_zpass", "auto"); c.set_option("fft_backend", "custom"); c.set_option("fft_pad", "auto")
        c.set_option("fft_pad", "160,160,48")               # read by the rocFFT path alone: the plan and the key are the same
        assert _equal(_view(c, gt, a), _off(mvs, ("a", PSF_SMALL, "pad"), gt, a, options={"fft_pad": "160,160,48"}))
        assert _stats(c) == (3, 2, 0)


@pytest.mark.gpu
def test_release_and_stats(mvs):
    """mvsim_release_caches frees every entry (bytes 0) and keeps the counters; the next view misses."""
    gt, a = _specimen(), _psf(PSF_SMALL)
    off_a = _off(mvs, ("a", PSF_SMALL), gt, a)
    with _ctx(mvs, 1024) as c:
        assert c.psf_cache_stats() == dict(hits=0, misses=0, evictions=0, bytes=0)
        _view(c, gt, a); _view(c, gt, a)
        s = c.psf_cache_stats()
        assert (s["hits"], s["misses"], s["evictions"]) == (1, 1, 0) and s["bytes"] > a.nbytes
        c.release_caches()
        assert c.psf_cache_stats() == dict(hits=1, misses=1, evictions=0, bytes=0)
        assert _equal(_view(c, gt, a), off_a)
        assert c.psf_cache_stats() == dict(hits=1, misses=2, evictions=0, bytes=s["bytes"])
        assert _equal(_view(c, gt, a), off_a)
        assert _stats(c) == (2, 2, 0)
        c.set_option("psf_cache", 0)                        # off: the entries stay where they are, nothing looks at them
        assert _equal(_view(c, gt, a), off_a)
        assert c.psf_cache_stats() == dict(hits=2, misses=2, evictions=0, bytes=s["bytes"])


@pytest.mark.gpu
def test_bypasses_leave_the_counters_alone(mvs):
    """Stacked views, a z slab, a captured graph, the stencil and the convolution stage operator neither look a PSF up nor enter one --
    with an entry of the very PSF in the cache -- and give what psf_cache = 0 gives."""
    gt, a = _specimen(), _psf(PSF_SMALL)
    nz, ny, nx = SHAPE
    dims = (nx, ny, nz)

    def others(c):
        out = {}
        c.set_option("view_batch", 1)
        params = [c.view_params(degrees=d, inc=1, snr=25.0, seed=SEED + v, stream=3, conv_method=1) for v, d in enumerate((0, 3))]
        out["stacked"] = c.simulate_views(gt, [a.copy(), a.copy()], params)
        d_gt, d_acq = c.dev_alloc(gt.nbytes), c.dev_alloc(gt.nbytes)
        try:
            c.upload(d_gt, gt)
            p = c.view_params(degrees=0, inc=1, snr=25.0, seed=SEED, stream=3, conv_method=1)
            own = c.view_slab_convolve_dev(d_gt, dims, a.copy(), p, 8, 16)
            k = c.view_slab_finish_dev(dims, p, 8, 16, own, d_acq)
            c.synchronize()
            out["slab"] = [c.download(d_acq, (k, ny, nx))]
        finally:
            c.dev_free(d_gt)
            c.dev_free(d_acq)
        out["stencil"] = [_view(c, gt, a, conv_method=2)["acq"]]
        out["stage"] = [c.convolve(gt, a.copy(), method=1)]
        c.set_option("graph", 1)
        out["graph"] = [_view(c, gt, a)["acq"] for _ in range(3)]          # eager, captured, replayed
        c.set_option("graph", 0)
        return out

    with _ctx(mvs, 0) as c:
        want = others(c)
    with _ctx(mvs, 1024) as c:
        _view(c, gt, a)
        assert _stats(c) == (0, 1, 0)
        got = others(c)
        assert _stats(c) == (0, 1, 0)
        assert _equal(_view(c, gt, a), _off(mvs, ("a", PSF_SMALL), gt, a))
        assert _stats(c) == (1, 1, 0)
    for name in want:
        assert len(got[name]) == len(want[name]) and all(_same(g, w) for g, w in zip(got[name], want[name])), name


@pytest.mark.gpu
def test_hits_on_the_side_stream(mvs):
    """2^24 voxels: the PSF's passes of a miss, and k_plane_flags_finish of every flagged view, run on the side stream.  A hit behind a
    flagged view keeps that kernel's fork and join; a hit of a view without flags (a volume without empty planes: only the first and
    every sixteenth view carry them) records neither.  The same sequence of views with psf_cache = 0 gives the same bits."""
    shape = (64, 512, 512)
    sparse = _specimen(shape, seed=94, planes=(30, 31, 32))
    dense = _specimen(shape, seed=95, planes=(30, 31, 32), offset=0.5)
    a, b = _psf((3, 5, 5)), _psf((3, 5, 5), 1)
    seq = ((sparse, a), (sparse, a), (dense, a), (dense, b), (dense, a), (sparse, b))
    res = {}
    for cache in (0, 1024):
        with _ctx(mvs, cache) as c:
            res[cache] = [_view(c, gt, p) for gt, p in seq]
            assert _stats(c) == ((4, 2, 0) if cache else (0, 0, 0))
    for on, off in zip(res[1024], res[0]):
        assert _equal(on, off)
