"""MvsimNative.extractIntervals (and devAlloc / uploadFloats / devFree) through the fake JNIEnv of tests/test_jni_shim.py: array lengths
and buffer capacities are checked before the C ABI is reached; on the GPU the bytes equal the C ABI's."""
import ctypes as C

import numpy as np
import pytest

from tests.test_jni_shim import IAE, PREFIX, jvm, vm  # noqa: F401  (fixtures)

i32, i64, f32, ptr = C.c_int32, C.c_int64, C.c_float, C.c_void_p


def _bind(vm):
    fns = {}
    for name, res, args in (("extractIntervals", None, [i64, ptr, ptr, ptr, ptr, ptr, ptr]), ("devAlloc", i64, [i64, i64]), ("devFree", None, [i64, i64]),
                            ("uploadFloats", None, [i64, i64, ptr, i64])):
        fn = getattr(vm.lib, PREFIX + name)
        fn.restype = res
        fn.argtypes = [ptr, ptr] + args
        fns[name] = fn
    return fns


def _geometry(jobs):
    g = []
    for d, dim, mn, mx, *_ in jobs:
        g += [d] + list(dim) + list(mn) + list(mx)
    return g


def _call(vm, fn, h, jobs, outs, geometry=None, n_inc=None):
    """jobs: (volume dptr, dim, min, max, inc, snr, seed, stream)"""
    n = len(jobs) if n_inc is None else n_inc
    fn(vm.env, None, h, vm.longs(_geometry(jobs) if geometry is None else geometry), vm.ints([j[4] for j in jobs][:n] + [1] * max(0, n - len(jobs))),
       vm.floats([j[5] for j in jobs]), vm.longs([j[6] for j in jobs]), vm.ints([j[7] for j in jobs]), vm.objects(outs))


def test_extract_intervals_checks_lengths_and_capacities_before_the_c_abi(vm):
    """A null context: were the C ABI reached, it would answer 'ctx is null' -- every refusal here has another message."""
    fn = _bind(vm)["extractIntervals"]
    dim = (37, 29, 23)
    job = (0x10000, dim, (3, 2, 1), (33, 27, 21), 3, 8.0, 7, 0)            # 31 x 26 x 7 outputs
    need = 31 * 26 * 7
    ok = np.zeros(need, np.float32)
    # an undersized output buffer
    _call(vm, fn, 0, [job], [vm.float_buffer(np.zeros(need - 1, np.float32))])
    e = vm.exception()
    assert e[0] == IAE and "smaller than the tile" in e[1]
    _call(vm, fn, 0, [job, job], [vm.float_buffer(ok), vm.float_buffer(ok, capacity=need - 1)])
    e = vm.exception()
    assert e[0] == IAE and "smaller than the tile" in e[1]
    _call(vm, fn, 0, [job], [vm.heap_buffer(need)])                          # not a direct buffer
    assert vm.exception()[0] == IAE
    # mismatched array lengths
    _call(vm, fn, 0, [job], [vm.float_buffer(ok)], geometry=_geometry([job])[:9])
    e = vm.exception()
    assert e[0] == IAE and "per output expected" in e[1]
    _call(vm, fn, 0, [job], [vm.float_buffer(ok), vm.float_buffer(ok.copy())])          # two outputs, one job
    e = vm.exception()
    assert e[0] == IAE and "per output expected" in e[1]
    _call(vm, fn, 0, [job], [vm.float_buffer(ok)], n_inc=2)
    e = vm.exception()
    assert e[0] == IAE and "per output expected" in e[1]
    # no job, too many jobs, a null array
    _call(vm, fn, 0, [], [])
    assert vm.exception()[0] == IAE
    _call(vm, fn, 0, [job] * 33, [vm.float_buffer(ok.copy()) for _ in range(33)])
    e = vm.exception()
    assert e[0] == IAE and "1..32" in e[1]
    fn(vm.env, None, 0, None, vm.ints([3]), vm.floats([8.0]), vm.longs([7]), vm.ints([0]), vm.objects([vm.float_buffer(ok)]))
    assert vm.exception()[0] == IAE
    # an interval that leaves its volume: the shim asks mvsim_interval_out_dim (host only) before it looks at the buffer
    bad = (0x10000, dim, (3, 2, 1), (37, 27, 21), 3, 8.0, 7, 0)
    _call(vm, fn, 0, [bad], [vm.float_buffer(ok)])
    e = vm.exception()
    assert e[0] == IAE and "leaves the volume" in e[1]
    # the device-memory wrappers refuse what needs no device to refuse
    fns = _bind(vm)
    assert fns["devAlloc"](vm.env, None, 0, 0) == 0
    assert vm.exception()[0] == IAE
    fns["uploadFloats"](vm.env, None, 0, 0x10000, vm.float_buffer(ok), need + 1)
    assert vm.exception()[0] == IAE
    fns["uploadFloats"](vm.env, None, 0, 0, vm.float_buffer(ok), need)
    assert vm.exception()[0] == IAE
    fns["devFree"](vm.env, None, 0, 0)                                       # a null pointer is ignored
    assert vm.exception() is None


@pytest.mark.gpu
def test_extract_intervals_through_the_shim_equals_the_c_abi(vm, ctx, mvs):
    """The jobs of tests/test_intervals.py::test_many_jobs_of_different_sizes, volumes uploaded through the shim's own wrappers."""
    fns = _bind(vm)
    h = ctx._h.value
    dim = (288, 288, 32)
    rng = np.random.default_rng(11)
    vols, dptrs = [], []
    for _ in range(2):
        v = np.exp(rng.uniform(np.log(1e-4), np.log(200.0), dim[::-1])).astype(np.float32)
        d = fns["devAlloc"](vm.env, None, h, v.nbytes)
        assert vm.exception() is None and d != 0
        fns["uploadFloats"](vm.env, None, h, d, vm.float_buffer(v), v.size)
        assert vm.exception() is None
        vols.append(v)
        dptrs.append(d)
    t0, t1 = mvs.tile_interval(dim, (0.2,) * 3, 0), mvs.tile_interval(dim, (0.2,) * 3, 1)
    lo0, hi0, lo1, hi1 = t0[0][:2] + [0], t0[1][:2] + [31], t1[0][:2] + [0], t1[1][:2] + [31]
    seed = 0x9E3779B97F4A7C15 - (1 << 64)                                    # a Java long: negative
    jobs = [(dptrs[0], dim, lo0, hi0, 3, 8.0, seed, 1), (dptrs[0], dim, lo1, hi1, 3, 8.0, seed + 1, 2),
            (dptrs[1], dim, (10, 20, 3), (200, 99, 30), 4, 25.0, seed + 2, 3), (dptrs[1], dim, lo0, hi0, 3, 8.0, seed + 3, 4),
            (dptrs[1], dim, (5, 6, 7), (60, 50, 20), 1, -1.0, 0, 0)]
    cjobs = [mvs.interval_job(*j) for j in jobs]
    want = ctx.extract_intervals(cjobs)
    got = [np.zeros(w.size, np.float32) for w in want]
    _call(vm, fns["extractIntervals"], h, jobs, [vm.float_buffer(g) for g in got])
    assert vm.exception() is None
    for g, w, v in zip(got, want, (vols[0], vols[0], vols[1], vols[1], vols[1])):
        assert np.array_equal(g.view(np.uint32), w.ravel().view(np.uint32))
    assert np.array_equal(want[4], vols[1][7:21, 6:51, 5:61])               # the copy job: the crop itself
    # a C-ABI refusal maps as the other natives map it
    _call(vm, fns["extractIntervals"], h, [(0, dim, lo0, hi0, 3, 8.0, 1, 0)], [vm.float_buffer(got[0])])
    e = vm.exception()
    assert e[0] == IAE and "null volume" in e[1]
    for d in dptrs:
        fns["devFree"](vm.env, None, h, d)
        assert vm.exception() is None
