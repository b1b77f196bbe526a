"""MvsimNative.traceRays / drawSimpleImage / sandboxRayStarts through the fake JNIEnv of tests/test_jni_shim.py: the same bytes as the
C ABI."""
import ctypes as C

import numpy as np
import pytest

from tests import raytrace_restatement as T
from tests import aberrations_restatement as R
from tests import trace_rays_cases as TC
from tests.test_jni_shim import IAE, PREFIX, jvm, vm  # noqa: F401  (fixtures)

i32, i64, f32, f64, u8, ptr = C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_ubyte, C.c_void_p


def _bind(vm):
    trace = getattr(vm.lib, PREFIX + "traceRays")
    trace.restype = i64
    trace.argtypes = [ptr, ptr, i64, ptr, ptr, ptr, ptr, ptr, ptr, i64, f64, f64, f64, i64, i32, u8, f64, ptr, ptr]
    wedge = getattr(vm.lib, PREFIX + "drawSimpleImage")
    wedge.restype = None
    wedge.argtypes = [ptr, ptr, i64, ptr, ptr, f32, f32]
    starts = getattr(vm.lib, PREFIX + "sandboxRayStarts")
    starts.restype = None
    starts.argtypes = [ptr, ptr, i64, ptr, ptr, i32, i32, i64, ptr, ptr]
    return trace, wedge, starts


def _double_buffer(vm, array, capacity=None):
    """A direct DoubleBuffer over a float64 numpy array (kept alive until reset)."""
    assert array.dtype == np.float64 and array.flags.c_contiguous
    vm._keep.append(array)
    return vm.lib.fake_buffer(array.ctypes.data, array.size if capacity is None else capacity)


def test_natives_check_their_buffers_before_the_c_abi(vm):
    trace, wedge, starts = _bind(vm)
    vol = np.ones(8 * 8 * 8, np.float32)
    small = np.ones(8 * 8 * 8 - 1, np.float32)
    rays = np.zeros(6)
    dim = lambda: vm.longs([8, 8, 8])
    fb = vm.float_buffer
    db = lambda a, capacity=None: _double_buffer(vm, a, capacity)
    args = (0.0, 1.0, 0.01, 96, 0, 0, 1.0)
    assert trace(vm.env, None, 0, fb(small), None, dim(), db(rays), db(rays), None, 2, *args, None, None) == 0
    assert vm.exception()[0] == IAE
    trace(vm.env, None, 0, fb(vol), fb(small), dim(), db(rays), db(rays), None, 2, *args, None, None)
    assert vm.exception()[0] == IAE
    trace(vm.env, None, 0, fb(vol), None, dim(), db(rays, 5), db(rays), None, 2, *args, None, None)
    assert vm.exception()[0] == IAE
    trace(vm.env, None, 0, fb(vol), None, dim(), db(rays), None, None, 2, *args, None, None)
    assert vm.exception()[0] == IAE
    trace(vm.env, None, 0, fb(vol), None, dim(), db(rays), db(rays), fb(vol, capacity=1), 2, *args, None, None)
    assert vm.exception()[0] == IAE
    trace(vm.env, None, 0, fb(vol), None, dim(), db(rays), db(rays), None, 2, *args, fb(vol), fb(small))
    assert vm.exception()[0] == IAE
    trace(vm.env, None, 0, fb(vol), None, dim(), db(rays), db(rays), None, -1, *args, None, None)
    assert vm.exception()[0] == IAE
    trace(vm.env, None, 0, fb(vol), None, vm.longs([8, 8]), db(rays), db(rays), None, 2, *args, None, None)
    assert vm.exception()[0] == IAE
    # a status of the C ABI (max_moves = 0; checked before a device is touched) becomes an exception
    trace(vm.env, None, 0, fb(vol), None, dim(), db(rays), db(rays), None, 2, 0.0, 1.0, 0.01, 0, 0, 0, 1.0, None, None)
    assert vm.exception()[0] == IAE
    wedge(vm.env, None, 0, fb(small), dim(), 1.0, 1.33)
    assert vm.exception()[0] == IAE
    starts(vm.env, None, 0, vm.longs([1]), dim(), 4, 4, 2, db(rays, 5), db(rays))
    assert vm.exception()[0] == IAE
    starts(vm.env, None, 0, None, dim(), 4, 4, 2, db(rays), db(rays))
    assert vm.exception()[0] == IAE
    starts(vm.env, None, 0, vm.longs([1]), dim(), 4, 4, -2, db(rays), db(rays))
    assert vm.exception()[0] == IAE


@pytest.mark.gpu
def test_natives_through_the_shim_equal_the_c_abi(vm, ctx, mvs):
    trace, wedge, starts = _bind(vm)
    shape = TC.SHAPES[1]
    dim = [shape[2], shape[1], shape[0]]
    n = 500
    img = np.zeros(shape, np.float32)
    wedge(vm.env, None, ctx._h.value, vm.float_buffer(img.reshape(-1)), vm.longs(dim), 1.0, 1.33)
    assert vm.exception() is None
    assert np.array_equal(img.view(np.uint32), ctx.draw_simple_image(shape, 1.0, 1.33).view(np.uint32))
    pos, vec = np.zeros((n, 3)), np.zeros((n, 3))
    state = vm.longs([R.seed_state(234345)])
    starts(vm.env, None, ctx._h.value, state, vm.longs(dim), TC.bundle_x(shape), 16, n, _double_buffer(vm, pos), _double_buffer(vm, vec))
    assert vm.exception() is None
    rnd = mvs.JavaRandom(234345)
    want_pos, want_vec = ctx.sandbox_ray_starts(shape, TC.bundle_x(shape), 16, n, rnd)
    assert np.array_equal(pos.view(np.uint64), want_pos.view(np.uint64)) and np.array_equal(vec, want_vec) and vm.read_longs(state, 1) == [rnd._s]
    ri_img = TC.field_b(shape)
    image, weight = np.zeros(ri_img.size, np.float32), np.zeros(ri_img.size, np.float32)
    capped = trace(vm.env, None, ctx._h.value, vm.float_buffer(ri_img.reshape(-1)), None, vm.longs(dim), _double_buffer(vm, pos),
                   _double_buffer(vm, vec), None, n, 0.0, 1.0, 0.01, T.default_max_moves(shape), 0, 0, 1.0, vm.float_buffer(image),
                   vm.float_buffer(weight))
    assert vm.exception() is None and capped == 0
    want = ctx.trace_rays(ri_img, pos, vec)
    assert np.array_equal(image.view(np.uint32), want["image"].reshape(-1).view(np.uint32))
    assert np.array_equal(weight.view(np.uint32), want["weight"].reshape(-1).view(np.uint32)) and weight.max() > 0
    # the other value sources and the reflect policy reach the C ABI as given
    inten = np.linspace(0.5, 2.0, n).astype(np.float32)
    fa = TC.field_a(shape)
    trace(vm.env, None, ctx._h.value, vm.float_buffer(fa.reshape(-1)), None, vm.longs(dim), _double_buffer(vm, pos), _double_buffer(vm, vec),
          vm.float_buffer(inten), n, 1.0, 1.33, 0.01, T.default_max_moves(shape), 1, 1, 1.0, vm.float_buffer(image), vm.float_buffer(weight))
    assert vm.exception() is None
    want = ctx.trace_rays(fa, pos, vec, intensity=inten, n_a=1.0, n_b=1.33, total_reflection="reflect", normalize_dirs=True)
    assert np.array_equal(image.view(np.uint32), want["image"].reshape(-1).view(np.uint32))
    # a zero direction never leaves: counted, not an exception of the native
    zero = np.zeros((1, 3))
    capped = trace(vm.env, None, ctx._h.value, vm.float_buffer(ri_img.reshape(-1)), None, vm.longs(dim), _double_buffer(vm, pos[:1].copy()),
                   _double_buffer(vm, zero), None, 1, 0.0, 1.0, 0.01, 50, 0, 0, 1.0, None, None)
    assert vm.exception() is None and capped == 1
