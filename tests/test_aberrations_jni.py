"""MvsimNative.refract3d / projectToCamera through the fake JNIEnv of tests/test_jni_shim.py: the same bytes as the C ABI."""
import ctypes as C

import numpy as np
import pytest

from tests import aberrations_cases as cases
from tests import aberrations_restatement as R
from tests.test_jni_shim import IAE, PREFIX, jvm, vm  # noqa: F401  (fixtures)

i32, i64, f64, u8, ptr = C.c_int32, C.c_int64, C.c_double, C.c_ubyte, C.c_void_p


def _bind(vm):
    refract = getattr(vm.lib, PREFIX + "refract3d")
    refract.restype = None
    refract.argtypes = [ptr, ptr, i64, ptr, ptr, ptr, u8, i32, f64, f64, f64, i64, ptr, ptr, ptr]
    camera = getattr(vm.lib, PREFIX + "projectToCamera")
    camera.restype = None
    camera.argtypes = [ptr, ptr, i64, ptr, ptr, ptr, i32, i32, ptr, ptr]
    return refract, camera


def test_natives_check_their_buffers_before_the_c_abi(vm):
    refract, camera = _bind(vm)
    vol = np.zeros(8 * 8 * 8, np.float32)
    small = np.zeros(8 * 8 * 8 - 1, np.float32)
    plane = np.zeros(8 * 8, np.float32)
    dim = lambda: vm.longs([8, 8, 8])
    fb = vm.float_buffer
    refract(vm.env, None, 0, fb(vol), fb(small), dim(), 0, 4, 1.0, 3.0, 1.1, 10, vm.longs([1]), fb(vol), fb(vol))
    assert vm.exception()[0] == IAE
    refract(vm.env, None, 0, fb(vol), fb(vol), dim(), 0, 4, 1.0, 3.0, 1.1, 10, vm.longs([1]), fb(vol), fb(small))
    assert vm.exception()[0] == IAE
    refract(vm.env, None, 0, fb(vol), fb(vol), dim(), 0, 4, 1.0, 3.0, 1.1, 10, None, fb(vol), fb(vol))
    assert vm.exception()[0] == IAE                            # no generator state
    refract(vm.env, None, 0, fb(vol), fb(vol), vm.longs([8, 8]), 0, 4, 1.0, 3.0, 1.1, 10, vm.longs([1]), fb(vol), fb(vol))
    assert vm.exception()[0] == IAE
    camera(vm.env, None, 0, fb(vol), fb(vol), dim(), 4, 5, vm.longs([1]), fb(plane, capacity=63))
    assert vm.exception()[0] == IAE
    camera(vm.env, None, 0, fb(small), fb(vol), dim(), 4, 5, vm.longs([1]), fb(plane))
    assert vm.exception()[0] == IAE
    camera(vm.env, None, 0, fb(vol), fb(vol), dim(), 4, 5, vm.longs([]), fb(plane))
    assert vm.exception()[0] == IAE


@pytest.mark.gpu
def test_natives_through_the_shim_equal_the_c_abi(vm, ctx, mvs):
    refract, camera = _bind(vm)
    shape = cases.TRACE_SHAPES[1]
    img, ri_img = cases.trace_inputs(shape)
    dim = [shape[2], shape[1], shape[0]]
    image, weight = np.zeros(img.size, np.float32), np.zeros(img.size, np.float32)
    state = vm.longs([R.seed_state(2423)])
    refract(vm.env, None, ctx._h.value, vm.float_buffer(img.reshape(-1)), vm.float_buffer(ri_img.reshape(-1)), vm.longs(dim), 1, 16,
            cases.LS_MIDDLE, cases.LS_EDGE, cases.RI, 1000, state, vm.float_buffer(image), vm.float_buffer(weight))
    assert vm.exception() is None
    rnd = mvs.JavaRandom(2423)
    want = ctx.refract3d(img, ri_img, True, 16, cases.LS_MIDDLE, cases.LS_EDGE, cases.RI, 1000, rnd)
    assert np.array_equal(image.view(np.uint32), want["image"].reshape(-1).view(np.uint32))
    assert np.array_equal(weight.view(np.uint32), want["weight"].reshape(-1).view(np.uint32))
    assert vm.read_longs(state, 1) == [rnd._s]
    proj = np.zeros(shape[1] * shape[2], np.float32)
    state = vm.longs([R.seed_state(464232194)])
    camera(vm.env, None, ctx._h.value, vm.float_buffer(ri_img.reshape(-1)), vm.float_buffer(want["image"].reshape(-1)), vm.longs(dim), 16, 5,
           state, vm.float_buffer(proj))
    assert vm.exception() is None
    rnd = mvs.JavaRandom(464232194)
    want_proj = ctx.project_to_camera(ri_img, want["image"], 16, 5, rnd)
    assert np.array_equal(proj.view(np.uint32), want_proj.reshape(-1).view(np.uint32)) and vm.read_longs(state, 1) == [rnd._s]
    # a status from the C ABI becomes an exception and leaves the state alone
    state = vm.longs([7])
    camera(vm.env, None, ctx._h.value, vm.float_buffer(ri_img.reshape(-1)), vm.float_buffer(ri_img.reshape(-1)), vm.longs(dim), 16, 0, state,
           vm.float_buffer(proj))
    assert vm.exception()[0] == IAE and vm.read_longs(state, 1) == [7]
