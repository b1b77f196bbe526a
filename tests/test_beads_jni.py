"""MvsimNative.renderBeads through the fake JNIEnv of tests/test_jni_shim.py: the same bytes as the C ABI."""
import ctypes as C

import numpy as np
import pytest

from tests.test_jni_shim import IAE, PREFIX, jvm, vm  # noqa: F401  (fixtures)

i32, i64, f64, ptr = C.c_int32, C.c_int64, C.c_double, C.c_void_p


def _bind(vm):
    fn = getattr(vm.lib, PREFIX + "renderBeads")
    fn.restype = None
    fn.argtypes = [ptr, ptr, i64, ptr, i64, ptr, ptr, i32, ptr, f64, f64, f64, ptr, ptr]
    return fn


def test_render_beads_checks_its_buffers_before_the_c_abi(vm):
    fn = _bind(vm)
    pts = np.zeros(5, dtype=np.float64)                        # fewer than 3 n doubles
    out = np.zeros(8 * 8 * 8, dtype=np.float32)
    fn(vm.env, None, 0, vm.lib.fake_buffer(pts.ctypes.data, 5), 2, None, None, 1, vm.longs([0, 0, 0, 8, 8, 8]), 1.0, 1.0, 1.0,
       vm.objects([vm.float_buffer(out)]), None)
    assert vm.exception()[0] == IAE
    fn(vm.env, None, 0, None, 0, None, None, 1, vm.longs([0, 0, 0, 8, 8]), 1.0, 1.0, 1.0, vm.objects([vm.float_buffer(out)]), None)
    assert vm.exception()[0] == IAE
    fn(vm.env, None, 0, None, 0, None, None, 1, vm.longs([0, 0, 0, 8, 8, 9]), 1.0, 1.0, 1.0, vm.objects([vm.float_buffer(out)]), None)
    assert vm.exception()[0] == IAE                            # 8 x 8 x 9 voxels do not fit


@pytest.mark.gpu
def test_render_beads_through_the_shim_equals_the_c_abi(vm, ctx, mvs):
    fn = _bind(vm)
    rng = np.random.default_rng(4)
    interval = ((-2, 1, 0), (40, 30, 20))
    pts = rng.random((500, 3)) * 44 - 3
    mats = np.stack([mvs.SimulateMultiViewDataset.axisRotation((43, 30, 21), 0, a) for a in (0, 40)]).reshape(2, 12)
    nv = 42 * 29 * 20
    f = [np.zeros(nv, np.float32) for _ in range(2)]
    u = [np.zeros(nv, np.uint16) for _ in range(2)]
    fn(vm.env, None, ctx._h.value, vm.lib.fake_buffer(pts.ctypes.data, pts.size), len(pts), None, vm.lib.fake_buffer(mats.ctypes.data, 24), 2,
       vm.longs(list(interval[0]) + list(interval[1])), 1.0, 1.0, 3.0, vm.objects([vm.float_buffer(x) for x in f]),
       vm.objects([vm.lib.fake_buffer(x.ctypes.data, nv) for x in u]))
    assert vm.exception() is None
    want = ctx.render_beads(pts, interval, (1, 1, 3), matrices=mats, f32=True, u16=True)
    for v in range(2):
        assert np.array_equal(f[v].reshape(want["f32"][v].shape).view(np.uint32), want["f32"][v].view(np.uint32))
        assert np.array_equal(u[v].reshape(want["u16"][v].shape), want["u16"][v])
