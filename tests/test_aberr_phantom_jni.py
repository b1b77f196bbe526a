"""MvsimNative.riNoise / multiSpheres / sphereWalkGeometry through the fake JNIEnv of tests/test_jni_shim.py: the same bytes as the C ABI,
the generator state in and out through long[1]."""
import ctypes as C

import numpy as np
import pytest

from tests import aberr_phantom_restatement as R
from tests.test_jni_shim import IAE, PREFIX, jvm, vm  # noqa: F401  (fixtures)

i32, i64, ptr = C.c_int32, C.c_int64, C.c_void_p


def _bind(vm):
    noise = getattr(vm.lib, PREFIX + "riNoise")
    noise.restype = None
    noise.argtypes = [ptr, ptr, i64, ptr, i64, ptr]
    multi = getattr(vm.lib, PREFIX + "multiSpheres")
    multi.restype = i64
    multi.argtypes = [ptr, ptr, i64, ptr, ptr, ptr, i32, ptr]
    geometry = getattr(vm.lib, PREFIX + "sphereWalkGeometry")
    geometry.restype = None
    geometry.argtypes = [ptr, ptr, ptr]
    return noise, multi, geometry


def test_natives_check_their_arguments_before_the_c_abi(vm, mvs):
    noise, multi, geometry = _bind(vm)
    vol = np.zeros(8 * 8 * 8, np.float32)
    small = np.zeros(8 * 8 * 8 - 1, np.float32)
    fb = vm.float_buffer
    noise(vm.env, None, 0, fb(small), 512, vm.longs([1]))
    assert vm.exception()[0] == IAE                            # fewer floats than the count
    noise(vm.env, None, 0, fb(vol), -1, vm.longs([1]))
    assert vm.exception()[0] == IAE
    noise(vm.env, None, 0, fb(vol), 512, None)
    assert vm.exception()[0] == IAE                            # no generator state
    multi(vm.env, None, 0, fb(vol), fb(small), vm.longs([8, 8, 8]), 1, vm.longs([1]))
    assert vm.exception()[0] == IAE
    multi(vm.env, None, 0, fb(vol), fb(vol), vm.longs([8, 8]), 1, vm.longs([1]))
    assert vm.exception()[0] == IAE
    multi(vm.env, None, 0, fb(vol), fb(vol), vm.longs([8, 8, 8]), 1, vm.longs([]))
    assert vm.exception()[0] == IAE
    geometry(vm.env, None, vm.longs([0]))
    assert vm.exception()[0] == IAE                            # long[2] expected
    out = vm.longs([0, 0])
    geometry(vm.env, None, out)
    assert vm.exception() is None
    chunk, entries = C.c_int64(0), C.c_int(0)
    assert mvs._lib.load().mvsim_sphere_walk_geometry(C.byref(chunk), C.byref(entries)) == 0
    assert vm.read_longs(out, 2) == [chunk.value, entries.value] and chunk.value > 0


@pytest.mark.gpu
def test_natives_through_the_shim_equal_the_c_abi(vm, ctx, mvs):
    noise, multi, _ = _bind(vm)
    rng = np.random.default_rng(9)
    ri0 = (0.03 + 0.02 * rng.standard_normal(21 * 17 * 13)).astype(np.float32)
    got = ri0.copy()
    state = vm.longs([R.scramble(11)])
    noise(vm.env, None, ctx._h.value, vm.float_buffer(got), got.size, state)
    assert vm.exception() is None
    want = ri0.copy()
    rnd = mvs.JavaRandom(11)
    ctx.ri_noise(want, rnd)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and vm.read_longs(state, 1) == [rnd._s]
    noise(vm.env, None, ctx._h.value, None, 0, state)             # n = 0: nothing drawn
    assert vm.exception() is None and vm.read_longs(state, 1) == [rnd._s]

    shape = (160, 160, 160)
    ri = np.full(shape, 1.05, np.float32)
    ri[60:101, 50:90, 70:125] = np.float32(5.0)
    img = np.zeros(shape, np.float32)
    w_img, w_ri = img.copy(), ri.copy()
    state = vm.longs([R.scramble(28)])
    n = multi(vm.env, None, ctx._h.value, vm.float_buffer(img.reshape(-1)), vm.float_buffer(ri.reshape(-1)), vm.longs([160, 160, 160]), 1, state)
    assert vm.exception() is None
    rnd = mvs.JavaRandom(28)
    assert ctx.multi_spheres(w_img, w_ri, 1, rnd) == n >= 1
    assert vm.read_longs(state, 1) == [rnd._s]
    assert np.array_equal(img.view(np.uint32), w_img.view(np.uint32)) and np.array_equal(ri.view(np.uint32), w_ri.view(np.uint32))
    # a status from the C ABI becomes an exception and leaves the state alone
    tiny = np.zeros(64 ** 3, np.float32)
    state = vm.longs([7])
    multi(vm.env, None, ctx._h.value, vm.float_buffer(tiny), vm.float_buffer(tiny.copy()), vm.longs([64, 64, 64]), 1, state)
    assert vm.exception()[0] == IAE and vm.read_longs(state, 1) == [7]
