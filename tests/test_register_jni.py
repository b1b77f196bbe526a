"""MvsimNative.registerBeads through the fake JNIEnv of tests/test_jni_shim.py: every length, null and capacity is refused before the C
ABI is reached, and one small run returns the bytes of Context.register_beads."""
import ctypes as C

import numpy as np
import pytest

from tests import register_reference as R
from tests.test_jni_shim import IAE, PREFIX, jvm, vm  # noqa: F401  (fixtures)
from tests.test_register_host import rotated_cloud

i32, i64, f64, ptr = C.c_int32, C.c_int64, C.c_double, C.c_void_p
F64 = np.float64


def _bind(vm):
    fn = getattr(vm.lib, PREFIX + "registerBeads")
    fn.restype = i64
    fn.argtypes = [ptr, ptr, i64, ptr, i64, ptr, i64, i32, f64, f64, f64, i64, i32, i32, i32, ptr, ptr, ptr]

    def call(h, pos_a, n_a, pos_b, n_b, result, candidates=None, mask=None, **kw):
        p = R.params(**kw)
        return fn(vm.env, None, h, pos_a, n_a, pos_b, n_b, p["redundancy"], p["ratio"], p["max_epsilon"], p["min_inlier_ratio"], p["seed"],
                  p["hypotheses"], p["max_refits"], p["min_inliers"], result, candidates, mask)
    return call


def _buffer(vm, array, capacity=None):
    """A direct buffer over any numpy array; capacity in elements of the array's type."""
    vm._keep.append(array)
    return vm.lib.fake_buffer(array.ctypes.data, array.size if capacity is None else capacity)


def test_native_checks_its_arguments_before_the_c_abi(vm):
    call = _bind(vm)
    pos = lambda n=8: _buffer(vm, np.ones(3 * n, F64))
    res = lambda nbytes=160: _buffer(vm, np.zeros(nbytes, np.uint8))
    bad = [
        dict(pos_a=None), dict(pos_b=None), dict(result=None), dict(n_a=-1), dict(n_b=-1), dict(n_a=R.MAX_POINTS + 1), dict(n_b=1 << 40),
        dict(pos_a=pos(7)), dict(pos_b=_buffer(vm, np.ones(23, F64))), dict(pos_a=vm.heap_buffer(24)), dict(result=res(159)),
        dict(result=vm.heap_buffer(160)), dict(candidates=res(24 * 8 - 1)), dict(mask=res(7)), dict(candidates=vm.heap_buffer(24 * 8)),
        dict(mask=vm.heap_buffer(8)),
    ]
    for kw in bad:
        args = dict(pos_a=pos(), n_a=8, pos_b=pos(), n_b=8, result=res())
        args.update(kw)
        assert call(0, **args) == 0                              # a null context: the C ABI would refuse it with another message
        exc = vm.exception()
        assert exc is not None and exc[0] == IAE, kw
        assert "ctx" not in exc[1], (kw, exc)
    # what the C ABI refuses arrives as the same exception, with its message
    for kw, word in ((dict(redundancy=3), "redundancy"), (dict(ratio=0.5), "ratio"), (dict(max_epsilon=0.0), "max_epsilon"),
                     (dict(hypotheses=0), "hypotheses"), (dict(max_refits=-1), "max_refits"), (dict(min_inliers=3), "min_inliers"),
                     (dict(min_inlier_ratio=float("nan")), "min_inlier_ratio")):
        assert call(0, pos(), 8, pos(), 8, res(), **kw) == 0
        exc = vm.exception()
        assert exc is not None and exc[0] == IAE and word in exc[1], (kw, exc)
    # good arguments get as far as the context
    assert call(0, pos(), 8, pos(), 8, res(), res(24 * 8), res(8)) == 0
    exc = vm.exception()
    assert exc is not None and "ctx" in exc[1]


@pytest.mark.gpu
def test_native_equals_the_c_abi(vm, ctx, mvs):
    call = _bind(vm)
    A, B, _ = rotated_cloud()
    kw = dict(max_epsilon=1.0, hypotheses=200, min_inliers=4, redundancy=2, seed=5)
    want, want_cand, want_mask = ctx.register_beads(A, B, mvs.match_params(**kw))
    assert want["flags"] == 0 and len(want_cand) >= 8
    res, cand, mask = np.full(160 + 8, 0xAB, np.uint8), np.full(24 * len(A) + 8, 0xAB, np.uint8), np.full(len(A) + 8, 0xAB, np.uint8)
    n = call(ctx._h.value, _buffer(vm, A.reshape(-1).copy()), len(A), _buffer(vm, B.reshape(-1).copy()), len(B), _buffer(vm, res, 160),
             _buffer(vm, cand, 24 * len(A)), _buffer(vm, mask, len(A)), **kw)
    assert vm.exception() is None
    assert n == len(want_cand) == want["n_candidates"]
    assert R.same_bits(res[:160].view(R.REGISTRATION_DTYPE)[0], want)
    assert R.same_bits(cand[:24 * n].view(R.MATCH_DTYPE), want_cand) and np.array_equal(mask[:n], want_mask)
    assert np.all(res[160:] == 0xAB) and np.all(cand[24 * n:] == 0xAB) and np.all(mask[n:] == 0xAB), "bytes past the records were written"
    # without the optional outputs; an empty list
    res2 = np.zeros(160, np.uint8)
    assert call(ctx._h.value, _buffer(vm, A.reshape(-1).copy()), len(A), _buffer(vm, B.reshape(-1).copy()), len(B), _buffer(vm, res2), **kw) == n
    assert vm.exception() is None and R.same_bits(res2.view(R.REGISTRATION_DTYPE)[0], want)
    assert call(ctx._h.value, _buffer(vm, np.zeros(3, F64)), 0, _buffer(vm, B.reshape(-1).copy()), len(B), _buffer(vm, res2)) == 0
    assert vm.exception() is None and res2.view(R.REGISTRATION_DTYPE)[0]["flags"] == R.FEW_CANDIDATES | R.NO_MODEL | R.FEW_INLIERS
    call(ctx._h.value, _buffer(vm, A.reshape(-1).copy()), len(A), _buffer(vm, B.reshape(-1).copy()), len(B), _buffer(vm, res2), ratio=0.0)
    exc = vm.exception()
    assert exc[0] == IAE and "ratio" in exc[1]
