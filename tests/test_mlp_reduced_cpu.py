"""Host side of the reduced-piece MLP forwards (bf16x3 / bf16x1), without a GPU: the numpy twin's piece rule and error bound, the two
constants in the header and the binding, the refusals of the library and of ``ops`` (they run before anything touches the device),
and the model option."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from tests import mlp_pieces_ref as twin
from tests.test_host_cpu import _exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED = -3


def test_piece_rule():
    """A route keeps exactly the products a_i b_j with i + j < NP: 257 = 256 + 1 in two pieces."""
    assert [twin.piece_product(257.0, 257.0, n) for n in (1, 2, 3)] == [65536.0, 66048.0, 66049.0]
    # round-to-nearest-even on the bit pattern: ties go to the even 8-bit significand, the second piece carries the sign
    assert twin.bf16_rn(np.float32([257.0, 259.0, 258.5, -257.0, 1.0])).tolist() == [256.0, 260.0, 258.0, -256.0, 1.0]
    p = twin.pieces(np.float32([259.0, 4097.0, 0.1]), 3)
    assert p[0].tolist()[:2] == [260.0, 4096.0] and p[1].tolist()[:2] == [-1.0, 1.0]
    assert np.float32(p[0][2] + p[1][2]) + p[2][2] == np.float32(0.1)          # three pieces are the whole f32 value
    t = twin.pieces(np.float32([259.0]), 2, twin.bf16_trunc)
    assert [float(v[0]) for v in t] == [258.0, 1.0]


@pytest.mark.parametrize("head", [True, False])
@pytest.mark.parametrize("n_pieces", [1, 2])
def test_twin_stays_inside_its_bound(head, n_pieces):
    net = twin.random_network(head, 2000)
    bias = net["bias_rows"][net["ridx"]] if head else None
    got = twin.forward(net["x"], net["weights"], n_pieces, bias, sigmoid=head)
    ref, E = twin.exact_and_bound(net["x"], net["weights"], n_pieces, bias, sigmoid=head)
    ratio = float((np.abs(got - ref) / E).max())
    print(f"head={head} NP={n_pieces}: worst |err| / E = {ratio:.3f}, max err / scale = {np.abs(got - ref).max() / np.abs(ref).max():.2e}")
    assert ratio < 1.0
    # and the ladder is a ladder: each route is at least 50 times tighter than the one below it
    errs = [float(np.abs(twin.forward(net["x"], net["weights"], n, bias, sigmoid=head) - ref).max()) for n in (1, 2, 3)]
    assert errs[0] > 50 * errs[1] > 2500 * errs[2], errs


def test_header_binding_and_symbols():
    from lsenerf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lse_hip.h")).read()
    defs = dict(re.findall(r"#define (LSE_MLP_ARITH_\w+) (\d+)", hdr))
    assert defs == {"LSE_MLP_ARITH_AUTO": "0", "LSE_MLP_ARITH_F32_MFMA": "1", "LSE_MLP_ARITH_BF16X3": "2", "LSE_MLP_ARITH_BF16X1": "3"}
    assert (_lib.LSE_MLP_ARITH_BF16X3, _lib.LSE_MLP_ARITH_BF16X1) == (2, 3)
    assert "i + j < NP" in hdr
    assert _lib.LSE_ABI_VERSION == 6 and _lib.load().lse_abi_version() == 6           # additive: no new version
    names = _exported(_lib.LIB_PATH)                                                   # ... and no new symbol
    assert names == set(_lib.SIGNATURES) | {"lse_abi_version", "lse_last_error", "lse_hash_bwd_default_opts",
                                            "lse_hash_bwd_workspace_bytes"}
    assert not [n for n in names if "x3" in n or "x1" in n or "reduced" in n]
    from lsenerf_amd import ops
    assert ops.MLP_ARITH_ROUTES == {"bf16x6": 0, "bf16x3": 2, "bf16x1": 3}


def _metas():
    from lsenerf_amd import _lib, ops
    head = ops.MlpMeta(16, 64, 2, _lib.LSE_ACT_SIGMOID, _lib.LSE_IN_ROWMAJOR, w0_ld=64, w0_col=15, w0_mask_col0=1)
    base = ops.MlpMeta(32, 64, 1, _lib.LSE_ACT_NONE, _lib.LSE_IN_LEVELMAJOR)
    return head, base


@pytest.mark.parametrize("route", ["bf16x3", "bf16x1"])
def test_library_refusals_need_no_device(route):
    from lsenerf_amd import _lib, ops
    lib = _lib.load()
    arith = ops.MLP_ARITH_ROUTES[route]
    one = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    head, base = (dataclasses.replace(m, arith=arith) for m in _metas())

    def fwd(meta, act=None, act_tiled=0):
        d = meta.desc()
        return lib.lse_mlp_fwd(ctypes.byref(d), one, one, None, None, one, 16, act, act_tiled, None, None, 0.0, 8, None, None)

    refused = {
        "width 32": fwd(dataclasses.replace(base, width=32)),
        "64 inputs": fwd(dataclasses.replace(head, n_in=64, w0_ld=0, w0_col=0, w0_mask_col0=0)),
        "level-major 16 inputs": fwd(ops.MlpMeta(16, 64, 2, in_layout=_lib.LSE_IN_LEVELMAJOR, arith=arith)),
        "one hidden layer on 16 inputs": fwd(ops.MlpMeta(16, 64, 1, arith=arith)),
        "two hidden layers on 32 inputs": fwd(ops.MlpMeta(32, 64, 2, arith=arith)),
        "saved activations, row-major": fwd(head, act=one, act_tiled=0),
        "saved activations, tiled": fwd(base, act=one, act_tiled=1),
        "saved activations, first layer recomputed": fwd(head, act=one, act_tiled=2),
    }
    for what, rc in refused.items():
        assert rc == UNSUPPORTED, what
    assert b"reduced-piece" in lib.lse_last_error()

    def pair(bm, hm):
        bd, hd = bm.desc(), hm.desc()
        return lib.lse_mlp_fwd_pair(ctypes.byref(bd), one, one, None, 1.0, ctypes.byref(hd), one, None, None, one, one, one, 4, 8, None, None)

    other = _lib.LSE_MLP_ARITH_BF16X1 if route == "bf16x3" else _lib.LSE_MLP_ARITH_BF16X3
    for what, (bm, hm) in {"base bf16x6": (dataclasses.replace(base, arith=0), head), "head bf16x6": (base, dataclasses.replace(head, arith=0)),
                           "two reduced routes": (base, dataclasses.replace(head, arith=other)),
                           "f32 MFMA head": (base, dataclasses.replace(head, arith=_lib.LSE_MLP_ARITH_F32_MFMA)),
                           "head shape": (base, dataclasses.replace(head, n_hidden_layers=1))}.items():
        assert pair(bm, hm) == UNSUPPORTED, what
        assert b"lse_mlp_fwd_pair" in lib.lse_last_error(), what

    d = head.desc()
    assert lib.lse_mlp_bwd(ctypes.byref(d), one, one, None, 3, one, 4, one, None, None, 0.0, None, None, None, one, one, None, None,
                           None, 8, None, None) == UNSUPPORTED
    assert b"lse_mlp_bwd" in lib.lse_last_error() and b"reduced-piece" in lib.lse_last_error()
    assert lib.lse_mlp_bwd_input(ctypes.byref(d), one, one, one, 4, one, None, None, 0.0, one, None, None, None, 8, None, None) == UNSUPPORTED
    assert b"lse_mlp_bwd_input" in lib.lse_last_error()
    plain = dataclasses.replace(head, w0_ld=0, w0_col=0, w0_mask_col0=0).desc()
    assert lib.lse_mlp_wgrad(ctypes.byref(plain), one, one, one, one, one, 8, None) == UNSUPPORTED
    assert b"lse_mlp_wgrad" in lib.lse_last_error()
    bad = dataclasses.replace(head, arith=4).desc()
    assert lib.lse_mlp_fwd(ctypes.byref(bad), one, one, None, None, one, 16, None, 0, None, None, 0.0, 8, None, None) == -1      # bad arith


@pytest.mark.parametrize("route", ["bf16x3", "bf16x1"])
def test_ops_refusals_come_before_any_launch(route):
    """ValueError, raised on CPU tensors: a launch would have raised LseHipError ("must live on the GPU") instead."""
    from lsenerf_amd import ops
    arith = ops.MLP_ARITH_ROUTES[route]
    head, base = (dataclasses.replace(m, arith=arith) for m in _metas())
    x = torch.zeros(8, 16)
    p = torch.zeros(head.n_params, requires_grad=True)
    with pytest.raises(ValueError, match="forward only"):
        ops.fused_mlp(p, x, head, 8)
    with pytest.raises(ValueError, match="forward only"):
        ops.fused_mlp(p.detach(), x.clone().requires_grad_(), head, 8)
    with pytest.raises(ValueError, match="forward only"):
        ops.fused_mlp(p.detach(), x, head, 8, torch.zeros(2, 64, requires_grad=True), torch.zeros(8, dtype=torch.int32))
    for bad in (dataclasses.replace(base, width=32), ops.MlpMeta(64, 64, 2, arith=arith), ops.MlpMeta(16, 64, 1, arith=arith)):
        with torch.no_grad(), pytest.raises(ValueError, match="serve the"):
            ops.fused_mlp(torch.zeros(bad.n_params), torch.zeros(8, bad.n_in), bad, 8)
    bp = torch.zeros(base.n_params, requires_grad=True)
    with pytest.raises(ValueError, match="forward only"):
        ops.fused_mlp_pair(bp, torch.zeros(16, 8, 2), None, 1.0, base, p.detach(), head, 8)
    with torch.no_grad(), pytest.raises(ValueError, match="same route"):
        ops.fused_mlp_pair(bp, torch.zeros(16, 8, 2), None, 1.0, base, p, dataclasses.replace(head, arith=0), 8)
    # the pair is usable for a reduced route only where nothing needs a gradient, and only with the same route in both
    y = torch.zeros(16, 8, 2)
    assert not ops.mlp_pair_usable(bp, y, base, p, head, None, None, None)
    with torch.no_grad():
        assert ops.mlp_pair_usable(bp, y, base, p, head, None, None, None)
        assert not ops.mlp_pair_usable(bp, y, base, p, dataclasses.replace(head, arith=0), None, None, None)
        assert not ops.mlp_pair_usable(bp, y, dataclasses.replace(base, arith=0), p, head, None, None, None)
        assert ops.mlp_pair_usable(bp, y, dataclasses.replace(base, arith=0), p, dataclasses.replace(head, arith=0), None, None, None)
    assert not ops.mlp_input_only_shape(head) and not ops.mlp_input_only_shape(base)       # no backward serves a reduced route


def test_config_and_field_option():
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig, ops
    aabb = torch.tensor([[-1.0, -1, -1], [1, 1, 1]])
    small = dict(grid_levels=1, grid_resolution=16, log2_hashmap_size=12)
    assert LSENeRFModelConfig().eval_mlp_arith == "bf16x6"
    m = LSENeRFModel(LSENeRFModelConfig(**small), aabb, 4)
    assert m.field.inference_arith == "bf16x6"
    for route in ("bf16x3", "bf16x1"):
        m = LSENeRFModel(LSENeRFModelConfig(eval_mlp_arith=route, **small), aabb, 4)
        fld = m.field
        assert fld.inference_arith == route
        meta = fld.mlp_base_mlp.meta()
        assert fld._routed(meta) is meta                                   # training mode: ignored
        fld.eval()
        assert fld._routed(meta) is meta                                   # eval mode with gradients recorded: ignored
        with torch.no_grad():
            assert fld._routed(meta).arith == ops.MLP_ARITH_ROUTES[route]
            fld.train()
            assert fld._routed(meta) is meta
    with pytest.raises(ValueError, match="eval_mlp_arith"):
        LSENeRFModel(LSENeRFModelConfig(eval_mlp_arith="fp16", **small), aabb, 4)
    with pytest.raises(ValueError, match="inference_arith"):
        m.field.inference_arith = "bf16"
    # a field whose MLPs are not the production shapes ignores the option: a narrower head, the small-grid base MLP
    for kw in (dict(hidden_dim_color=32), dict(hidden_dim=32), dict(num_levels=4)):
        f2 = LSENeRFModel(LSENeRFModelConfig(eval_mlp_arith="bf16x1", **small, **kw), aabb, 4).field.eval()
        with torch.no_grad():
            meta = f2.mlp_base_mlp.meta()
            assert f2._routed(meta) is meta, kw
