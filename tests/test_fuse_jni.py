"""MvsimNative.fuseViews and alignViews through the fake JNIEnv of tests/test_jni_shim.py: every length, null and capacity is refused
before the C ABI is reached, and one small run returns the bytes of Context.fuse_views and Context.align_views."""
import ctypes as C

import numpy as np
import pytest

from tests import fuse_reference as R
from tests.test_jni_shim import IAE, PREFIX, jvm, vm  # noqa: F401  (fixtures)

i32, i64, f32, f64, u8, ptr = C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_ubyte, C.c_void_p
F64 = np.float64


def _bind(vm):
    fuse = getattr(vm.lib, PREFIX + "fuseViews")
    fuse.restype = None
    fuse.argtypes = [ptr, ptr, i64, ptr, u8, ptr, ptr, ptr, ptr, f64, f64, f64, f32, ptr, ptr, ptr]
    align = getattr(vm.lib, PREFIX + "alignViews")
    align.restype = None
    align.argtypes = [ptr, ptr, i64, ptr, u8, ptr, ptr, ptr, ptr, f64, f64, f64, ptr, ptr, ptr]

    def call_fuse(h, views, dims, m12, out_min, out_dim, fused, sum_weights=None, status=None, blend=(8.0, 8.0, 8.0), background=0.0, u16=0):
        fuse(vm.env, None, h, views, u16, dims, m12, out_min, out_dim, blend[0], blend[1], blend[2], background, fused, sum_weights, status)

    def call_align(h, views, dims, m12, out_min, out_dim, aligned, weights=None, status=None, blend=(8.0, 8.0, 8.0), u16=0):
        align(vm.env, None, h, views, u16, dims, m12, out_min, out_dim, blend[0], blend[1], blend[2], aligned, weights, status)
    return call_fuse, call_align


def _buffer(vm, array, capacity=None):
    """A direct buffer over any numpy array; capacity in elements of the array's type."""
    vm._keep.append(array)
    return vm.lib.fake_buffer(array.ctypes.data, array.size if capacity is None else capacity)


def test_native_checks_its_arguments_before_the_c_abi(vm):
    call_fuse, call_align = _bind(vm)
    vol = lambda n=24: _buffer(vm, np.ones(n, np.float32))          # noqa: E731
    mats = lambda n=24: _buffer(vm, np.tile(R.identity().reshape(12), 2)[:n].copy())    # noqa: E731

    def good():
        return dict(views=vm.objects([vol(), vol()]), dims=vm.longs([4, 3, 2, 2, 3, 4]), m12=mats(), out_min=vm.longs([0, 0, 0]),
                    out_dim=vm.longs([4, 3, 2]))

    bad = [dict(views=None), dict(dims=None), dict(m12=None), dict(out_min=None), dict(out_dim=None), dict(views=vm.objects([])),
           dict(views=vm.objects([vol()] * 33)), dict(dims=vm.longs([4, 3, 2])), dict(dims=vm.longs([4, 3, 2, 0, 3, 4])),
           dict(out_min=vm.longs([0, 0])), dict(out_dim=vm.longs([4, 3])), dict(out_dim=vm.longs([4, 0, 2])), dict(m12=mats(23)),
           dict(m12=vm.heap_buffer(24)), dict(views=vm.objects([vol(), vol(23)])), dict(views=vm.objects([vol(), None])),
           dict(views=vm.objects([vm.heap_buffer(24), vol()]))]
    for kw in bad:
        for call, outs in ((call_fuse, dict(fused=vol())), (call_align, dict(aligned=vm.objects([vol(), vol()])))):
            args = good()
            args.update(outs)
            args.update(kw)
            call(0, **args)                                      # a null context: the C ABI would refuse it with another message
            exc = vm.exception()
            assert exc is not None and exc[0] == IAE, kw
            assert "ctx" not in exc[1], (kw, exc)
    status = lambda n=2: _buffer(vm, np.zeros(n, np.int32))          # noqa: E731
    for outs in (dict(fused=None), dict(fused=vol(23)), dict(fused=vm.heap_buffer(24)), dict(fused=vol(), sum_weights=vol(23)),
                 dict(fused=vol(), status=status(1))):
        call_fuse(0, **good(), **outs)
        exc = vm.exception()
        assert exc is not None and exc[0] == IAE and "ctx" not in exc[1], outs
    for outs in (dict(aligned=None), dict(aligned=vm.objects([vol()])), dict(aligned=vm.objects([vol(), vol(23)])),
                 dict(aligned=vm.objects([vol(), vol()]), weights=vm.objects([vol()])),
                 dict(aligned=vm.objects([vol(), None]), weights=vm.objects([vol(5), None])),
                 dict(aligned=vm.objects([vol(), vol()]), status=status(1))):
        call_align(0, **good(), **outs)
        exc = vm.exception()
        assert exc is not None and exc[0] == IAE and "ctx" not in exc[1], outs
    # what the C ABI refuses arrives as the same exception, with its message
    call_fuse(0, **good(), fused=vol(), blend=(8.0, -1.0, 8.0))
    exc = vm.exception()
    assert exc is not None and exc[0] == IAE and "blend" in exc[1]
    # good arguments get as far as the context
    call_fuse(0, **good(), fused=vol(), sum_weights=vol(), status=status())
    exc = vm.exception()
    assert exc is not None and "ctx" in exc[1]
    call_align(0, **good(), aligned=vm.objects([vol(), None]), weights=vm.objects([None, vol()]), status=status())
    exc = vm.exception()
    assert exc is not None and "ctx" in exc[1]


@pytest.mark.gpu
def test_native_equals_the_c_abi(vm, ctx, mvs):
    call_fuse, call_align = _bind(vm)
    rng = np.random.default_rng(3)
    views = [rng.uniform(0, 900, (17, 33, 40)).astype(np.float32), rng.uniform(0, 900, (3, 4, 5)).astype(np.float32)]
    mats = [R.rotation(0, 33, (19.5, 16.0, 8.0)), R.translation((10.25, 9.5, 4.75))]
    out_min, out_dim, n = (-6, -6, -3), (70, 50, 24), 70 * 50 * 24
    p = mvs.fuse_params(blend=(3.5, 2.0, 0.0), background=-2.0)
    want = ctx.fuse_views(views, mats, out_min, out_dim, p, sum_weights=True, status=True)
    assert R.same_bits(want[0], R.fuse(views, mats, out_min, out_dim, (3.5, 2.0, 0.0), -2.0)[0])

    def args():
        return dict(views=vm.objects([_buffer(vm, v.copy()) for v in views]), dims=vm.longs([40, 33, 17, 5, 4, 3]),
                    m12=_buffer(vm, np.concatenate([np.asarray(m, F64).reshape(12) for m in mats])), out_min=vm.longs(list(out_min)),
                    out_dim=vm.longs(list(out_dim)))

    fused, sw = np.full(n + 8, -777.0, np.float32), np.full(n + 8, -777.0, np.float32)
    st = np.full(4, 77, np.int32)
    call_fuse(ctx._h.value, **args(), fused=_buffer(vm, fused, n), sum_weights=_buffer(vm, sw, n), status=_buffer(vm, st, 2),
              blend=(3.5, 2.0, 0.0), background=-2.0)
    assert vm.exception() is None
    assert R.same_bits(fused[:n].reshape(want[0].shape), want[0]) and R.same_bits(sw[:n].reshape(want[1].shape), want[1])
    assert list(st) == [0, 0, 77, 77] and np.all(fused[n:] == -777.0) and np.all(sw[n:] == -777.0), "bytes past the outputs were written"
    fused2 = np.zeros(n, np.float32)
    call_fuse(ctx._h.value, **args(), fused=_buffer(vm, fused2), blend=(3.5, 2.0, 0.0), background=-2.0)          # without the optional outputs
    assert vm.exception() is None and R.same_bits(fused2.reshape(want[0].shape), want[0])
    # aligned views, with null entries
    wal, wwt = ctx.align_views(views, mats, out_min, out_dim, p)
    al0, wt1 = np.zeros(n, np.float32), np.zeros(n, np.float32)
    call_align(ctx._h.value, **args(), aligned=vm.objects([_buffer(vm, al0), None]), weights=vm.objects([None, _buffer(vm, wt1)]),
               blend=(3.5, 2.0, 0.0))
    assert vm.exception() is None
    assert R.same_bits(al0.reshape(wal[0].shape), wal[0]) and R.same_bits(wt1.reshape(wwt[1].shape), wwt[1])
    # uint16 views
    u16 = [v.astype(np.uint16) for v in views]
    a = args()
    a["views"] = vm.objects([_buffer(vm, v.copy()) for v in u16])
    call_fuse(ctx._h.value, **a, fused=_buffer(vm, fused2), blend=(3.5, 2.0, 0.0), background=-2.0, u16=1)
    p.src_type = mvs._lib.MVSIM_SRC_U16
    assert vm.exception() is None and R.same_bits(fused2.reshape(want[0].shape), ctx.fuse_views(u16, mats, out_min, out_dim, p))
    call_fuse(ctx._h.value, **args(), fused=_buffer(vm, fused2), blend=(np.nan, 2.0, 0.0))
    exc = vm.exception()
    assert exc[0] == IAE and "blend" in exc[1]
