"""MvsimNative.detectBeads through the fake JNIEnv of tests/test_jni_shim.py: every length, null and capacity is refused before the C
ABI is reached, and one small run returns the bytes of Context.detect_beads."""
import ctypes as C

import numpy as np
import pytest

from tests import dog_reference as R
from tests.test_jni_shim import IAE, PREFIX, jvm, vm  # noqa: F401  (fixtures)

i32, i64, f32, f64, u8, ptr = C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_ubyte, C.c_void_p
F32 = np.float32
ITEM = R.PEAK_DTYPE.itemsize


def _bind(vm):
    fn = getattr(vm.lib, PREFIX + "detectBeads")
    fn.restype = i64
    fn.argtypes = [ptr, ptr, i64, ptr, u8, ptr, f64, f64, f64, f64, f64, f64, f32, i32, i64, ptr]

    def call(h, img, dim, peaks, u16=0, sigma1=R.DEFAULT_SIGMA1, sigma2=R.DEFAULT_SIGMA2, threshold=5.0, max_moves=4, capacity=8):
        return fn(vm.env, None, h, img, u16, dim, *sigma1, *sigma2, threshold, max_moves, capacity, peaks)
    return call


def _buffer(vm, array, capacity=None):
    """A direct buffer over any numpy array; capacity in elements of the array's type."""
    vm._keep.append(array)
    return vm.lib.fake_buffer(array.ctypes.data, array.size if capacity is None else capacity)


def test_native_checks_its_arguments_before_the_c_abi(vm):
    call = _bind(vm)
    n = 6 * 5 * 4
    img = lambda: _buffer(vm, np.ones(n, F32))
    out = lambda cap=8: _buffer(vm, np.zeros(ITEM * cap, np.uint8))
    dim = vm.longs([6, 5, 4])
    bad = [
        dict(img=None), dict(peaks=None), dict(dim=None), dict(dim=vm.longs([6, 5])), dict(dim=vm.longs([6, 0, 4])),
        dict(img=_buffer(vm, np.ones(n - 1, F32))), dict(img=_buffer(vm, np.ones(n - 1, np.uint16)), u16=1), dict(img=vm.heap_buffer(n)),
        dict(peaks=out(7)), dict(peaks=_buffer(vm, np.zeros(ITEM * 8 - 1, np.uint8))), dict(peaks=vm.heap_buffer(ITEM * 8)),
        dict(capacity=0), dict(capacity=-1), dict(capacity=(1 << 31) + 1), dict(capacity=1 << 40),
    ]
    for kw in bad:
        args = dict(img=img(), dim=dim, peaks=out())
        args.update(kw)
        assert call(0, **args) == 0                              # a null context: the C ABI would refuse it with another message
        exc = vm.exception()
        assert exc is not None and exc[0] == IAE, kw
        assert "ctx" not in exc[1], (kw, exc)
    # what the C ABI refuses arrives as the same exception, with its message
    for kw, word in ((dict(sigma1=(0.0, 1.0, 1.0)), "sigma"), (dict(sigma2=(1.0, 1.0, 11.0)), "taps"), (dict(threshold=float("nan")), "threshold"),
                     (dict(max_moves=-1), "max_moves"), (dict(dim=vm.longs([6, 1, 4]), img=img()), "extent")):
        args = dict(img=img(), dim=dim, peaks=out())
        args.update(kw)
        assert call(0, **args) == 0
        exc = vm.exception()
        assert exc is not None and exc[0] == IAE and word in exc[1], (kw, exc)


@pytest.mark.gpu
def test_native_equals_the_c_abi(vm, ctx, mvs):
    call = _bind(vm)
    rng = np.random.default_rng(9)
    shape = (30, 28, 34)
    pts = R.draw_positions(shape, 4, rng)
    img = R.add_poisson(R.render_beads(shape, pts), rng)
    dim = vm.longs(list(shape[::-1]))
    for kind, cap in ((F32, 8), (np.uint16, 8), (F32, 2)):
        a = np.ascontiguousarray(img.astype(kind))
        want, n_want = ctx.detect_beads(a, cap, mvs.dog_params(threshold=5.0))
        assert n_want == 4
        raw = np.full(ITEM * cap + 8, 0xAB, np.uint8)
        found = call(ctx._h.value, _buffer(vm, a.reshape(-1)), dim, _buffer(vm, raw, ITEM * cap), u16=int(kind is np.uint16), capacity=cap)
        assert vm.exception() is None
        listed = min(4, cap)
        assert found == 4 and R.same_bits(raw[:ITEM * listed].view(R.PEAK_DTYPE), want)
        assert np.all(raw[ITEM * listed:] == 0xAB), "bytes past min(found, capacity) records were written"
    call(ctx._h.value, _buffer(vm, img.reshape(-1)), dim, _buffer(vm, np.zeros(ITEM * 8, np.uint8)), sigma1=(1.0, 1.0, -1.0))
    exc = vm.exception()
    assert exc[0] == IAE and "sigma" in exc[1]
