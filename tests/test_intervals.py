"""extractSlices over intervals of volumes that stay on the device (mvsim_extract_intervals*, extract_interval.hip) against the oracle and
against the existing path on the host-cropped tile.  Every comparison is bit-exact (floats on their uint32 view): lambda is identical on
both sides.  The case list and the host-side tests: tests/test_intervals_host.py."""
import ctypes as C

import numpy as np
import pytest

from . import test_intervals_host as H

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15
STREAM = 5


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _values(shape_zyx, seed):
    """v log-uniform over [1e-4, 200] with a few exact zeros, one negative and one NaN: with the snrs of the sweep, lambda spans the
    shortcut, the inversion and the PTRS regimes (lambda <= 0 or NaN gives 0, Q9)."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape_zyx))
    v = np.exp(rng.uniform(np.log(1e-4), np.log(200.0), n)).astype(np.float32)
    v[rng.choice(n, max(3, n // 97), replace=False)] = 0.0
    v[n // 3] = -1.5
    v[n // 2] = np.nan
    return v.reshape(shape_zyx)


class _Dev:
    """Host volumes uploaded once per module, device buffers freed at the end."""

    def __init__(self, ctx):
        self.ctx, self.ptrs, self.vols = ctx, [], {}

    def alloc(self, nbytes):
        p = self.ctx.dev_alloc(max(4, nbytes))
        self.ptrs.append(p)
        return p

    def volume(self, dim_xyz, seed=1):
        key = (tuple(dim_xyz), seed)
        if key not in self.vols:
            host = _values(tuple(dim_xyz)[::-1], seed)
            d = self.alloc(host.nbytes)
            self.ctx.upload(d, host)
            self.vols[key] = (host, d)
        return self.vols[key]

    def close(self):
        for p in self.ptrs:
            self.ctx.dev_free(p)


@pytest.fixture(scope="module")
def ictx(mvs):
    c = mvs.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev(ictx):
    d = _Dev(ictx)
    yield d
    ictx.synchronize()
    d.close()


def _crop(host, mn, mx):
    return np.ascontiguousarray(host[mn[2]:mx[2] + 1, mn[1]:mx[1] + 1, mn[0]:mx[0] + 1])


def _want(orc, crop, inc, snr, seed, stream):
    if snr < 0:
        return np.ascontiguousarray(crop[::inc])
    return orc.extract_slices_counter(crop, inc, snr, seed, stream)


@pytest.mark.parametrize("name,dim,mn,mx", H.SWEEP, ids=[c[0] for c in H.SWEEP])
def test_sweep(mvs, orc, ictx, dev, name, dim, mn, mx):
    host, d = dev.volume(dim)
    crop = _crop(host, mn, mx)
    for inc in H.INCS:
        for snr in H.SNRS:
            job = mvs.interval_job(d, dim, mn, mx, inc, snr, SEED, STREAM)
            got = ictx.extract_intervals([job])[0]
            path = ictx.extract_path()
            want = _want(orc, crop, inc, snr, SEED, STREAM)
            assert _bits_equal(got, want), (name, inc, snr, "oracle")
            assert _bits_equal(got, ictx.extract_slices(crop, inc, snr, SEED, STREAM)), (name, inc, snr, "existing path")
            assert path[0] == H.K_INTERVAL and path[4] == 1, path
            if snr >= 0:
                assert path[3] > 0, (name, inc, snr, path)          # the two-launch form, not the queue-less sampler


def test_many_jobs_of_different_sizes(mvs, orc, ictx, dev):
    dim = (288, 288, 32)
    host_a, da = dev.volume(dim, 2)
    host_b, db = dev.volume(dim, 3)
    t0 = mvs.tile_interval(dim, (0.2,) * 3, 0)
    t1 = mvs.tile_interval(dim, (0.2,) * 3, 1)
    lo0, hi0 = t0[0][:2] + [0], t0[1][:2] + [31]
    lo1, hi1 = t1[0][:2] + [0], t1[1][:2] + [31]
    assert [b - a + 1 for a, b in zip(lo0, hi0)] == [174, 174, 32] and [b - a + 1 for a, b in zip(lo1, hi1)] == [173, 173, 32]
    spec = [(host_a, da, lo0, hi0, 3, 8.0, SEED, 1), (host_a, da, lo1, hi1, 3, 8.0, SEED + 1, 2),
            (host_b, db, (10, 20, 3), (200, 99, 30), 4, 25.0, SEED + 2, 3),                        # another volume, another inc
            (host_b, db, lo0, hi0, 3, 8.0, SEED + 3, 4), (host_b, db, (5, 6, 7), (60, 50, 20), 1, -1.0, 0, 0)]      # two more on the same volume
    jobs = [mvs.interval_job(d, dim, lo, hi, inc, snr, seed, st) for _, d, lo, hi, inc, snr, seed, st in spec]
    together = ictx.extract_intervals(jobs)
    path = ictx.extract_path()
    assert path[0] == H.K_INTERVAL
    alone = [ictx.extract_intervals([j])[0] for j in jobs]
    outs = [dev.alloc(a.nbytes) for a in alone]
    ictx.extract_intervals_dev(jobs, outs)
    for i, (host, _, lo, hi, inc, snr, seed, st) in enumerate(spec):
        assert _bits_equal(together[i], alone[i]), i
        assert _bits_equal(ictx.download(outs[i], alone[i].shape), alone[i]), i
        assert _bits_equal(alone[i], _want(orc, _crop(host, lo, hi), inc, snr, seed, st)), i
    # the arrays of an earlier call, written in place
    scratch = [np.full_like(a, -7.0) for a in alone]
    again = ictx.extract_intervals(jobs, out=scratch)
    assert all(a is b for a, b in zip(again, scratch)) and all(_bits_equal(a, b) for a, b in zip(again, alone))
    with pytest.raises(ValueError):
        ictx.extract_intervals(jobs, out=scratch[:-1])
    with pytest.raises(ValueError):
        ictx.extract_intervals(jobs[:1], out=[scratch[1]])
    # jobs 0 and 3 (equal tile, inc and snr) shared their launches with each other: the call's last launch had one job, the copy
    assert path[4] == 1
    ictx.extract_intervals([jobs[0], jobs[3]])
    assert ictx.extract_path()[4] == 2


def test_refused_voxels(mvs, orc):
    """Segments of one sixteenth, every voxel at lambda = 10: phase 1's squeeze accepts ~35 % (extract_plan.h), so most of every block's
    pending voxels are refused and k_poisson_refused samples them where they stand."""
    dim, mn, mx, snr = (101, 83, 41), (2, 1, 0), (97, 80, 39), 25.0
    mul = float(mvs._lib.load().mvsim_poisson_mul(float(np.float32(snr))))
    host = np.full(dim[::-1], np.float32(10.0 / mul), np.float32)
    want = orc.extract_slices_counter(_crop(host, mn, mx), 1, snr, SEED, STREAM)
    results = []
    for share in ("1", None):
        with mvs.Context(0) as c:
            if share:
                c.set_option("poisson_queue_share", share)
            d = c.dev_alloc(host.nbytes)
            c.upload(d, host)
            got = c.extract_intervals([mvs.interval_job(d, dim, mn, mx, 1, snr, SEED, STREAM)])[0]
            path, stats = c.extract_path(), c.queue_stats()
            c.dev_free(d)
        print("share", share, "path", path, "queue stats", stats)
        assert _bits_equal(got, want), share
        assert path[0] == H.K_INTERVAL and path[3] > 0
        if share:
            assert path[1] == 1 and stats["refused"] > 0, (path, stats)        # k_poisson_refused had voxels to walk
        else:
            assert path[1] == 0 and stats["refused"] == 0, (path, stats)
        results.append(got)
    assert _bits_equal(results[0], results[1])


def test_transfers(mvs, orc, ictx, dev):
    dim, mn, mx, snr = (130, 131, 64), (1, 2, 0), (128, 129, 63), 25.0
    host, d = dev.volume(dim, 4)
    job = mvs.interval_job(d, dim, mn, mx, 1, snr, SEED, STREAM)
    od = (C.c_int64 * 3)()
    mvs._lib.check(mvs._lib.load().mvsim_interval_out_dim(C.byref(job), od))
    assert od[0] * od[1] * od[2] == 1 << 20
    u0, f0 = ictx.transfer_stats()
    got = ictx.extract_intervals([job])[0]
    u1, f1 = ictx.transfer_stats()
    assert _bits_equal(got, orc.extract_slices_counter(_crop(host, mn, mx), 1, snr, SEED, STREAM))
    assert (u1 - u0, f1 - f0) == (1, 0)                    # the 16-bit path, no fallback
    # one voxel whose count cannot be a uint16: the output crosses as float32 after all
    hot = host.copy()
    mul = float(mvs._lib.load().mvsim_poisson_mul(float(np.float32(snr))))
    hot[10, 40, 50] = np.float32(80000.0 / mul)
    assert float(hot[10, 40, 50]) * mul > 70000
    d2 = dev.alloc(hot.nbytes)
    ictx.upload(d2, hot)
    got = ictx.extract_intervals([mvs.interval_job(d2, dim, mn, mx, 1, snr, SEED, STREAM)])[0]
    u2, f2 = ictx.transfer_stats()
    assert (u2 - u1, f2 - f1) == (1, 1)
    assert got.max() > 65535
    assert _bits_equal(got, orc.extract_slices_counter(_crop(hot, mn, mx), 1, snr, SEED, STREAM))


def test_errors_leave_the_context_usable(mvs, orc, ictx, dev):
    dim = H.VOL_A
    host, d = dev.volume(dim)
    n = dim[0] * dim[1] * dim[2]
    good = mvs.interval_job(d, dim, (3, 2, 1), (33, 27, 21), 3, 8.0, SEED, STREAM)
    out = dev.alloc(4 * n)
    out2 = dev.alloc(4 * n)
    L = mvs._lib.load()
    bad_jobs = {
        "null volume": mvs.interval_job(0, dim, (0, 0, 0), (3, 3, 3), 1, 8.0),
        "inc": mvs.interval_job(d, dim, (0, 0, 0), (3, 3, 3), 0, 8.0),
        "min > max": mvs.interval_job(d, dim, (4, 0, 0), (3, 3, 3), 1, 8.0),
        "leaves": mvs.interval_job(d, dim, (0, 0, 0), (37, 3, 3), 1, 8.0),
        "negative": mvs.interval_job(d, dim, (0, -1, 0), (3, 3, 3), 1, 8.0),
    }
    for what, job in bad_jobs.items():
        with pytest.raises(ValueError):
            ictx.extract_intervals_dev([job], [out])
        with pytest.raises(ValueError):
            ictx.extract_intervals([job])
    # the full-overlap tile of an even size (mvsim_tile_interval does not validate; the extract calls do)
    mn, mx, _ = mvs.tile_interval((64,) * 3, (1.0,) * 3, 0)
    big = dev.alloc(4 * 64 ** 3)
    for call in (lambda j: ictx.extract_intervals_dev([j], [out]), lambda j: ictx.extract_intervals([j])):
        with pytest.raises(ValueError, match="leaves the volume"):
            call(mvs.interval_job(big, (64,) * 3, mn, mx, 3, 8.0))
    # n out of range, null pointers
    with pytest.raises(ValueError):
        ictx.extract_intervals_dev([], [])
    with pytest.raises(ValueError):
        ictx.extract_intervals([])
    outs33 = (C.c_void_p * 33)(*[out + 4096 * i for i in range(33)])
    jobs33 = (mvs.IntervalJob * 33)(*[mvs.interval_job(d, dim, (0, 0, 0), (3, 3, 3), 1, 8.0) for _ in range(33)])
    for fn in (L.mvsim_extract_intervals_dev, L.mvsim_extract_intervals):
        assert fn(ictx._h, jobs33, 33, outs33) == mvs._lib.MVSIM_EINVAL
        assert fn(ictx._h, None, 1, outs33) == mvs._lib.MVSIM_EINVAL
        assert fn(ictx._h, jobs33, 1, None) == mvs._lib.MVSIM_EINVAL
        assert fn(ictx._h, jobs33, 2, (C.c_void_p * 2)(out, None)) == mvs._lib.MVSIM_EINVAL
    # outputs that overlap each other or a job's volume
    with pytest.raises(ValueError, match="overlap"):
        ictx.extract_intervals_dev([good, good], [out, out + 64])
    with pytest.raises(ValueError, match="overlap"):
        ictx.extract_intervals_dev([good], [d + 4 * (n - 8)])
    with pytest.raises(ValueError, match="overlap"):
        ictx.extract_intervals_dev([good, mvs.interval_job(out2, dim, (0, 0, 0), (3, 3, 3), 1, -1.0)], [out2 + 16, out])
    a = np.empty((7, 26, 31), np.float32)
    with pytest.raises(ValueError, match="overlap"):
        L_out = (C.c_void_p * 2)(a.ctypes.data, a.ctypes.data + 128)
        mvs._lib.check(L.mvsim_extract_intervals(ictx._h, (mvs.IntervalJob * 2)(good, good), 2, L_out))
    # ... and the context still works
    want = orc.extract_slices_counter(_crop(host, (3, 2, 1), (33, 27, 21)), 3, 8.0, SEED, STREAM)
    assert _bits_equal(ictx.extract_intervals([good])[0], want)
    ictx.extract_intervals_dev([good], [out])
    assert _bits_equal(ictx.download(out, want.shape), want)


def test_mirror_at_the_reference_size(mvs, synth):
    """SimulateTileStitching(resident=True) against the host-crop path of the same constructor: the volumes, the pairs, the translation."""
    T = mvs.SimulateTileStitching
    psf = synth.measured_like_psf(51)
    with T(mvs.JavaRandom(5), True, (0.2,) * 3, None, psf=psf.copy(), resident=True) as res:
        host = T(mvs.JavaRandom(5), True, (0.2,) * 3, None, psf=psf.copy())
        assert res.getCorrectTranslation() == host.getCorrectTranslation() == [114.5, 114.5, 115 / 3]
        assert res.getInterval(0) == host.getInterval(0) and res.getInterval(1) == host.getInterval(1)
        for snr in (-1.0, 8.0):
            a = res.getNextPair(snr)
            assert mvs.default_context().extract_path()[0] == H.K_INTERVAL and mvs.default_context().extract_path()[4] == 2      # one call, two jobs
            b = host.getNextPair(snr)
            assert a[0].shape == b[0].shape == (58, 174, 174)
            assert _bits_equal(a[0], b[0]) and _bits_equal(a[1], b[1]), snr
        assert _bits_equal(res.con, host.con) and _bits_equal(res.conHalfPixel, host.conHalfPixel)
        assert res.con is res.con                                   # downloaded once
    with pytest.raises(RuntimeError):
        res.getNextPair(8.0)
    with pytest.raises(RuntimeError):
        res.getNextPairs([8.0])
    del host
    with T(mvs.JavaRandom(5), True, (0.2,) * 3, None, psf=psf.copy(), resident=True) as third:
        state = third.rnd._s
        many = third.getNextPairs([8.0, 25.0, -1.0])
        third.rnd._s = state                                        # the same seeds again, one pair per call
        for snr, pair in zip((8.0, 25.0, -1.0), many):
            one = third.getNextPair(snr)
            assert _bits_equal(one[0], pair[0]) and _bits_equal(one[1], pair[1]), snr
        assert not _bits_equal(many[0][0], many[1][0])
        third.rnd._s = state                                        # ... and once more into the arrays of the first call
        kept = [(a.copy(), b.copy()) for a, b in many]
        for a, b in many:
            a.fill(-7.0)
            b.fill(-7.0)
        reused = third.getNextPairs([8.0, 25.0, -1.0], out=many)
        for (a, b), (c, d), (e, f) in zip(reused, many, kept):
            assert a is c and b is d and _bits_equal(a, e) and _bits_equal(b, f)
