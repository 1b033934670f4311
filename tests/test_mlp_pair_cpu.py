"""Argument validation of the two fused entry points (lse_mlp_fwd_pair, lse_ray_grad_from_dx01) happens before any launch, so the
error paths run without a GPU: null pointers and descriptors outside the pair's shapes come back as the library's error codes with a
text behind ``lse_last_error``."""
import ctypes

LSE_E_INVALID, LSE_E_UNSUPPORTED = -1, -3


def _descs():
    from lsenerf_amd import _lib
    base = _lib.MlpDesc(32, 64, 1, _lib.LSE_ACT_NONE, _lib.LSE_IN_LEVELMAJOR)
    head = _lib.MlpDesc(16, 64, 2, _lib.LSE_ACT_SIGMOID, _lib.LSE_IN_ROWMAJOR, 64, 15, 1)
    return base, head


def _pair(lib, base, head, n=8, ptr=None, out_cols=4):
    return lib.lse_mlp_fwd_pair(ctypes.byref(base) if base is not None else None, ptr, ptr, None, 1.0,
                                ctypes.byref(head) if head is not None else None, ptr, None, None, ptr, ptr, ptr, out_cols, n,
                                None, None)


def test_mlp_fwd_pair_refuses_bad_arguments_without_gpu():
    from lsenerf_amd import _lib
    lib = _lib.load()
    base, head = _descs()
    assert _pair(lib, base, head) == LSE_E_INVALID and b"null pointer" in lib.lse_last_error()
    assert _pair(lib, None, head) == LSE_E_INVALID and b"null desc" in lib.lse_last_error()
    assert _pair(lib, base, None) == LSE_E_INVALID and b"null desc" in lib.lse_last_error()
    assert _pair(lib, base, head, n=-1) == LSE_E_INVALID and b"n < 0" in lib.lse_last_error()
    assert _pair(lib, base, head, out_cols=8) == LSE_E_INVALID and b"out_cols" in lib.lse_last_error()
    assert _pair(lib, base, head, n=0) == 0          # zero-sized work is a no-op, not an error
    # a descriptor no kernel exists for at all: the usual check_desc text
    bad = _lib.MlpDesc(24, 64, 1, 0, 0)
    assert _pair(lib, bad, head) == LSE_E_INVALID and b"n_in" in lib.lse_last_error()
    # valid descriptors that lse_mlp_fwd serves but the pair does not: LSE_E_UNSUPPORTED, the caller launches twice
    unsupported = [
        (_lib.MlpDesc(32, 64, 2, _lib.LSE_ACT_NONE, _lib.LSE_IN_LEVELMAJOR), head),                      # base with two hidden layers
        (_lib.MlpDesc(32, 32, 1, _lib.LSE_ACT_NONE, _lib.LSE_IN_LEVELMAJOR), head),                      # narrow base
        (_lib.MlpDesc(32, 64, 1, _lib.LSE_ACT_SIGMOID, _lib.LSE_IN_LEVELMAJOR), head),                   # activated base output
        (base, _lib.MlpDesc(16, 64, 1, _lib.LSE_ACT_SIGMOID, _lib.LSE_IN_ROWMAJOR, 64, 15, 1)),          # head with one hidden layer
        (base, _lib.MlpDesc(64, 64, 2, _lib.LSE_ACT_SIGMOID, _lib.LSE_IN_ROWMAJOR)),                     # head with a 64-wide input
        (_lib.MlpDesc(32, 64, 1, _lib.LSE_ACT_NONE, _lib.LSE_IN_LEVELMAJOR, 0, 0, 0, _lib.LSE_MLP_ARITH_F32_MFMA), head),
    ]
    for b, h in unsupported:
        assert _pair(lib, b, h) == LSE_E_UNSUPPORTED, (b.n_in, b.width, h.n_in)
        assert b"lse_mlp_fwd_pair" in lib.lse_last_error() and b"lse_mlp_fwd twice" in lib.lse_last_error()
    # the binding raises with the same text
    import pytest
    with pytest.raises(_lib.LseHipError, match="lse_mlp_fwd_pair"):
        _lib.call("lse_mlp_fwd_pair", ctypes.byref(unsupported[0][0]), None, None, None, 1.0, ctypes.byref(head), None, None, None,
                  None, None, None, 4, 8, None, None)


def test_ray_grad_from_dx01_refuses_bad_arguments_without_gpu():
    from lsenerf_amd import _lib
    lib = _lib.load()
    f = lib.lse_ray_grad_from_dx01
    assert f(None, None, None, None, None, 4, 1, None, None, None, None, None) == LSE_E_INVALID
    assert b"lse_ray_grad_from_dx01: null pointer" in lib.lse_last_error()
    assert f(None, None, None, None, None, -1, 1, None, None, None, None, None) == LSE_E_INVALID
    assert b"n_rays < 0" in lib.lse_last_error()
    assert f(None, None, None, None, None, 0, 1, None, None, None, None, None) == 0
    # aabb normalisation without a box (the pointers are never dereferenced on the host)
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert f(p, p, p, p, p, 2, 0, None, p, p, p, None) == LSE_E_INVALID and b"h_aabb" in lib.lse_last_error()
    # nothing asked for: no launch, no error
    assert f(p, p, p, p, p, 2, 1, None, p, None, None, None) == 0
