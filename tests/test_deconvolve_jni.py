"""MvsimNative.deconvolve through the fake JNIEnv of tests/test_jni_shim.py: every length and capacity is refused before the C ABI is
reached, and one small run returns the bytes of Context.deconvolve."""
import ctypes as C

import numpy as np
import pytest

from tests import decon_reference as R
from tests.test_jni_shim import IAE, PREFIX, jvm, vm  # noqa: F401  (fixtures)

i32, i64, f32, f64, u8, ptr = C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_ubyte, C.c_void_p
F32 = np.float32


def _bind(vm):
    fn = getattr(vm.lib, PREFIX + "deconvolve")
    fn.restype = None
    fn.argtypes = [ptr, ptr, i64, ptr, ptr, ptr, ptr, ptr, i32, i32, u8, f32, f32, f32, f64, ptr]

    def call(h, views, weights, psfs, kdims, dim, psi, iterations=1, method=0, init_from_psi=0, init_value=0.0, min_value=1e-4, eps=1e-6, lam=0.0):
        fn(vm.env, None, h, views, weights, psfs, kdims, dim, iterations, method, init_from_psi, init_value, min_value, eps, lam, psi)
    return call


def test_native_checks_its_arguments_before_the_c_abi(vm):
    call = _bind(vm)
    fb, n = vm.float_buffer, 4 * 5 * 6
    vol = lambda: fb(np.ones(n, F32))
    small = lambda: fb(np.ones(n - 1, F32))
    psf = lambda: fb(np.ones(27, F32))
    dim, k1 = vm.longs([6, 5, 4]), vm.longs([3, 3, 3])
    bad = [
        dict(views=None), dict(psfs=None), dict(kdims=None), dict(dim=None), dict(psi=None),
        dict(dim=vm.longs([6, 5])), dict(dim=vm.longs([6, 0, 4])),
        dict(views=vm.objects([])), dict(views=vm.objects([vol() for _ in range(33)])),
        dict(psfs=vm.objects([psf(), psf()])), dict(kdims=vm.longs([3, 3])), dict(kdims=vm.longs([3, 3, 3, 3, 3, 3])),
        dict(weights=vm.objects([vol(), vol()])),
        dict(kdims=vm.longs([3, 0, 3])), dict(kdims=vm.longs([3, 3, 4])),                 # a PSF buffer of 27 floats for 36 taps
        dict(views=vm.objects([small()])), dict(weights=vm.objects([small()])), dict(psi=small()),
        dict(views=vm.objects([None])), dict(psfs=vm.objects([None])), dict(weights=vm.objects([None])),
    ]
    for kw in bad:
        args = dict(views=vm.objects([vol()]), weights=vm.objects([vol()]), psfs=vm.objects([psf()]), kdims=k1, dim=dim, psi=vol())
        args.update(kw)
        call(0, **args)                                         # a null context: the C ABI would refuse it with another message
        exc = vm.exception()
        assert exc is not None and exc[0] == IAE, kw
        assert "ctx" not in exc[1], (kw, exc)


@pytest.mark.gpu
def test_native_equals_the_c_abi(vm, ctx, mvs):
    call = _bind(vm)
    c = R.make_case(shape_zyx=(6, 10, 12), psf_shapes=((3, 5, 4), (5, 3, 3)))
    views, weights, psfs = c["views"], c["weights"], [p.copy() for p in c["psfs"]]
    kd = [e for p in psfs for e in p.shape[::-1]]
    fb = vm.float_buffer
    for w, lam in ((weights, 0.006), (None, 0.0)):
        p = mvs.decon_params(iterations=2, method=0, min_value=0.5, lambda_=lam)
        want = ctx.deconvolve(views, psfs, w, p)
        got = np.zeros(want.size, F32)
        call(ctx._h.value, vm.objects([fb(v.reshape(-1)) for v in views]), vm.objects([fb(x.reshape(-1)) for x in w]) if w else None,
             vm.objects([fb(q.reshape(-1)) for q in psfs]), vm.longs(kd), vm.longs([12, 10, 6]), fb(got), iterations=2, min_value=0.5, lam=lam)
        assert vm.exception() is None
        assert R.same_bits(got, want)
        assert all(np.array_equal(a, b) for a, b in zip(psfs, c["psfs"]))
    # continuing from an estimate, and a status from the C ABI as an exception
    one = ctx.deconvolve(views, psfs, weights, mvs.decon_params(iterations=1, min_value=0.5))
    two = ctx.deconvolve(views, psfs, weights, mvs.decon_params(iterations=2, min_value=0.5))
    got = one.reshape(-1).copy()
    call(ctx._h.value, vm.objects([fb(v.reshape(-1)) for v in views]), vm.objects([fb(x.reshape(-1)) for x in weights]),
         vm.objects([fb(q.reshape(-1)) for q in psfs]), vm.longs(kd), vm.longs([12, 10, 6]), fb(got), iterations=1, init_from_psi=1, min_value=0.5)
    assert vm.exception() is None and R.same_bits(got, two)
    call(ctx._h.value, vm.objects([fb(v.reshape(-1)) for v in views]), None, vm.objects([fb(q.reshape(-1)) for q in psfs]), vm.longs(kd),
         vm.longs([12, 10, 6]), fb(got), iterations=0)
    exc = vm.exception()
    assert exc[0] == IAE and "iterations" in exc[1]
