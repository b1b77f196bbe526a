"""MvsimNative.extractPsf through the fake JNIEnv of tests/test_jni_shim.py: every length, null and capacity is refused before the C ABI
is reached, and one small run returns the bytes of Context.extract_psf."""
import ctypes as C

import numpy as np
import pytest

from tests import fuse_reference as FR
from tests import psf_reference as R
from tests.test_jni_shim import IAE, PREFIX, jvm, vm  # noqa: F401  (fixtures)

i64, f64, u8, ptr = C.c_int64, C.c_double, C.c_ubyte, C.c_void_p
F64 = np.float64


def _bind(vm):
    fn = getattr(vm.lib, PREFIX + "extractPsf")
    fn.restype = i64
    fn.argtypes = [ptr, ptr, i64, ptr, u8, ptr, ptr, i64, ptr, ptr, ptr, f64, f64, f64, u8, u8, ptr, ptr, ptr]

    def call(h, img, dim, pos, n, kdim, psf, result, use=None, m12=None, status=None, sep=(0.0, 0.0, 0.0), subtract_min=1, normalize=1, u16=0):
        return fn(vm.env, None, h, img, u16, dim, pos, n, use, m12, kdim, sep[0], sep[1], sep[2], subtract_min, normalize, psf, result, status)
    return call


def _buffer(vm, array, capacity=None):
    """A direct buffer over any numpy array; capacity in elements of the array's type."""
    vm._keep.append(array)
    return vm.lib.fake_buffer(array.ctypes.data, array.size if capacity is None else capacity)


def test_native_checks_its_arguments_before_the_c_abi(vm):
    call = _bind(vm)
    vol = lambda n=24: _buffer(vm, np.ones(n, np.float32))          # noqa: E731
    dbl = lambda n=6: _buffer(vm, np.full(n, 1.0))                   # noqa: E731
    raw = lambda n=72: _buffer(vm, np.zeros(n, np.uint8))            # noqa: E731

    def good():
        return dict(img=vol(), dim=vm.longs([4, 3, 2]), pos=dbl(), n=2, kdim=vm.longs([3, 1, 1]), psf=vol(3), result=raw())

    bad = [dict(img=None), dict(dim=None), dict(pos=None), dict(kdim=None), dict(psf=None), dict(result=None), dict(n=-1), dict(n=65537),
           dict(dim=vm.longs([4, 3])), dict(dim=vm.longs([4, 0, 2])), dict(kdim=vm.longs([3, 1])), dict(kdim=vm.longs([2, 1, 1])),
           dict(kdim=vm.longs([65, 1, 1])), dict(kdim=vm.longs([0, 1, 1])), dict(img=vol(23)), dict(img=vm.heap_buffer(24)), dict(pos=dbl(5)),
           dict(psf=vol(2)), dict(psf=vm.heap_buffer(3)), dict(result=raw(71)), dict(use=raw(1)), dict(m12=dbl(11)), dict(status=raw(1))]
    for kw in bad:
        args = good()
        args.update(kw)
        call(0, **args)                                          # a null context: the C ABI would refuse it with another message
        exc = vm.exception()
        assert exc is not None and exc[0] == IAE, kw
        assert "ctx" not in exc[1], (kw, exc)
    # what the C ABI refuses arrives as the same exception, with its message
    call(0, **good(), sep=(1.0, -1.0, 1.0))
    exc = vm.exception()
    assert exc is not None and exc[0] == IAE and "min_separation" in exc[1]
    # good arguments get as far as the context
    call(0, **good(), use=raw(2), m12=dbl(12), status=raw(2))
    exc = vm.exception()
    assert exc is not None and "ctx" in exc[1]


@pytest.mark.gpu
def test_native_equals_the_c_abi(vm, ctx, mvs):
    call = _bind(vm)
    rng = np.random.default_rng(3)
    img = rng.uniform(0, 900, (17, 33, 40)).astype(np.float32)
    pos = np.vstack([rng.uniform(4, 12, (40, 3)) * (2.5, 2.0, 1.0), [[np.nan, 5, 5], [-30, 5, 5]]])
    use = (rng.uniform(size=len(pos)) > 0.2).astype(np.uint8)
    m = FR.rotation(0, 33, (19.5, 16.0, 8.0))
    kdim, sep, n, taps = (5, 3, 7), (2.0, 2.0, 2.0), len(pos), 105
    p = mvs.psf_params(kdim=kdim, min_separation=sep, subtract_min=1, normalize=0)
    want = ctx.extract_psf(img, pos, m, use, p, status=True)
    ref = R.extract(img, pos, m, use, kdim, sep, 1, 0)
    assert R.same_bits(want[0], ref[0]) and want[1]["n_used"] > 5 and want[1]["n_nonfinite"] == 1

    psf, res, st = np.full(taps + 8, -777.0, np.float32), np.full(80, 77, np.uint8), np.full(n + 8, 77, np.uint8)
    used = call(ctx._h.value, _buffer(vm, img.copy()), vm.longs([40, 33, 17]), _buffer(vm, pos.copy()), n, vm.longs(list(kdim)), _buffer(vm, psf, taps),
                _buffer(vm, res, 72), use=_buffer(vm, use.copy()), m12=_buffer(vm, np.asarray(m, F64).reshape(12).copy()), status=_buffer(vm, st, n),
                sep=sep, subtract_min=1, normalize=0)
    assert vm.exception() is None and used == want[1]["n_used"]
    assert R.same_bits(psf[:taps].reshape(want[0].shape), want[0]) and np.array_equal(st[:n], want[2])
    assert res[:72].tobytes() == want[1].tobytes()
    assert np.all(psf[taps:] == -777.0) and np.all(res[72:] == 77) and np.all(st[n:] == 77), "bytes past the outputs were written"
    # without the optional arguments: the identity, every bead, no status; uint16 voxels
    u16 = img.astype(np.uint16)
    p16 = mvs.psf_params(kdim=kdim, min_separation=0, src_type=mvs._lib.MVSIM_SRC_U16)
    want16 = ctx.extract_psf(u16, pos, None, None, p16)
    psf2 = np.zeros(taps, np.float32)
    call(ctx._h.value, _buffer(vm, u16.copy()), vm.longs([40, 33, 17]), _buffer(vm, pos.copy()), n, vm.longs(list(kdim)), _buffer(vm, psf2),
         _buffer(vm, res, 72), u16=1)
    assert vm.exception() is None and R.same_bits(psf2.reshape(want16[0].shape), want16[0])
    assert res[:72].tobytes() == want16[1].tobytes()
    call(ctx._h.value, _buffer(vm, img.copy()), vm.longs([40, 33, 17]), _buffer(vm, pos.copy()), n, vm.longs(list(kdim)), _buffer(vm, psf2),
         _buffer(vm, res, 72), sep=(np.nan, 0.0, 0.0))
    exc = vm.exception()
    assert exc[0] == IAE and "min_separation" in exc[1]
