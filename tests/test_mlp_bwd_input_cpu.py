"""Host side of the input-gradient-only MLP backward, without a GPU: ``lse_mlp_bwd_input`` in the header, the libraries and the
binding; its argument checks (they run before anything touches the device); ``freeze_field``'s opt-in keyword."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from tests.test_host_cpu import _exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_libraries_and_binding_agree():
    from lsenerf_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lse_hip.h")).read(), flags=re.S)
    m = re.search(r"\blse_mlp_bwd_input\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, "include/lse_hip.h does not declare lse_mlp_bwd_input"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 16 == len(_lib.SIGNATURES["lse_mlp_bwd_input"])
    assert args[-2] == "const int64_t *n_dev" and args[-3] == "int64_t n" and args[-1] == "lse_stream_t stream"
    assert "d_params" not in m.group(1)                                   # nothing parameter-sized is written
    assert "lse_mlp_bwd_input" in _exported(_lib.LIB_PATH) and "lse_mlp_bwd_input" in _exported(_lib.DEV_LIB_PATH)
    assert hasattr(_lib.load(), "lse_mlp_bwd_input")
    hdr = open(os.path.join(ROOT, "include", "lse_hip.h")).read()
    assert "BIT-EQUAL" in hdr[hdr.index("for FROZEN parameters (test-time refinement): d_in"):hdr.index("int lse_mlp_bwd_input(")]
    assert _lib.LSE_ABI_VERSION == 6                                      # additive


def test_argument_checks_need_no_device():
    from lsenerf_amd import _lib, ops
    lib = _lib.load()
    one = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    head = ops.MlpMeta(16, 64, 2, _lib.LSE_ACT_SIGMOID, _lib.LSE_IN_ROWMAJOR, w0_ld=64, w0_col=15, w0_mask_col0=1)
    base = ops.MlpMeta(32, 64, 1, _lib.LSE_ACT_NONE, _lib.LSE_IN_LEVELMAJOR)

    def rc_of(meta, d_in=one, idx=one, d_rb=None, n=8, out_cols=4, params=one):
        d = meta.desc()
        return lib.lse_mlp_bwd_input(ctypes.byref(d), params, one, one, out_cols, one, None, None, 0.0, d_in, one, idx, d_rb, n, None, None)

    for meta in (head, base):
        assert rc_of(meta, n=0) == 0                                      # nothing to do: no launch, no error
    import dataclasses
    refused = {
        "width 32": (dict(meta=dataclasses.replace(base, width=32)), -3),
        "64 inputs": (dict(meta=ops.MlpMeta(64, 64, 2)), -3),
        "level-major head": (dict(meta=ops.MlpMeta(16, 64, 2, _lib.LSE_ACT_NONE, _lib.LSE_IN_LEVELMAJOR)), -3),
        "two hidden layers on 32 inputs": (dict(meta=ops.MlpMeta(32, 64, 2)), -3),
        "f32 arithmetic": (dict(meta=dataclasses.replace(head, arith=_lib.LSE_MLP_ARITH_F32_MFMA)), -3),
        "both outputs null": (dict(meta=head, d_in=None), -1),
        "both outputs null, no samples": (dict(meta=head, d_in=None, n=0), -1),
        "d_row_bias without row_bias_idx": (dict(meta=head, d_rb=one, idx=None), -1),
        "negative n": (dict(meta=head, n=-1), -1),
        "out_cols": (dict(meta=head, out_cols=8), -1),
        "null params": (dict(meta=head, params=None), -1),
    }
    for what, (kw, code) in refused.items():
        assert rc_of(**kw) == code, what
        assert b"lse_mlp_bwd_input" in lib.lse_last_error(), what
    assert lib.lse_mlp_bwd_input(None, one, one, one, 4, one, None, None, 0.0, one, one, one, None, 8, None, None) == -1
    with pytest.raises(_lib.LseHipError, match="lse_mlp_bwd_input"):
        _lib.call("lse_mlp_bwd_input", ctypes.byref(head.desc()), one, one, one, 4, one, None, None, 0.0, None, None, None, None, 8,
                  None, None)


def test_the_ops_wrapper_has_no_cpu_path():
    from lsenerf_amd import _lib, ops
    meta = ops.MlpMeta(32, 64, 1)
    x = torch.zeros(8, 32)
    with pytest.raises(_lib.LseHipError, match="must live on the GPU"):
        ops.mlp_bwd_input(torch.zeros(meta.n_params), x, meta, 8, torch.zeros(8, 16), 16, torch.zeros(8, 16), d_in=torch.zeros_like(x))
    assert ops.mlp_input_only_shape(meta) and ops.mlp_input_only_shape(ops.MlpMeta(16, 64, 2))
    assert not ops.mlp_input_only_shape(ops.MlpMeta(16, 64, 1)) and not ops.mlp_input_only_shape(ops.MlpMeta(32, 32, 1))
    assert not ops.mlp_input_only_shape(ops.MlpMeta(32, 64, 1, arith=_lib.LSE_MLP_ARITH_F32_MFMA))


def test_the_switch_is_off_unless_asked_for():
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig, ops
    assert inspect.signature(LSENeRFModel.freeze_field).parameters["input_only_mlp"].default is False
    assert inspect.signature(ops.fused_mlp).parameters["input_only"].default is False
    assert inspect.signature(ops.fused_mlp_pair).parameters["input_only"].default is False
    m = LSENeRFModel(LSENeRFModelConfig(grid_levels=1, grid_resolution=16, log2_hashmap_size=12),
                     torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 4)
    mlps = (m.field.mlp_base_mlp, m.field.mlp_head)
    assert not any(x.input_only_bwd for x in mlps)
    m.freeze_field()
    assert not any(x.input_only_bwd for x in mlps) and not any(x.params.requires_grad for x in mlps)
    m.unfreeze_field()
    m.freeze_field(input_only_mlp=True)
    assert all(x.input_only_bwd for x in mlps) and not any(hasattr(x.params, "_lse_wgrad_scratch") for x in mlps)
    m.unfreeze_field()
    assert not any(x.input_only_bwd for x in mlps) and all(x.params.requires_grad for x in mlps)
