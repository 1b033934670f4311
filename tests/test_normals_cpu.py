"""Analytic normals without a GPU: the float64 twin (tests/normals_ref.py) against central differences, its compositing edge cases,
the two new entry points in the header, the libraries and the binding, the config field, and the ops' refusal of CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import hash_geometry_cases as hg
from tests import normals_ref as nr
from tests.test_host_cpu import _exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRY = "b2_m2048"        # 16 levels x 2 features = the base network's 32 inputs; the smallest table of the 16-level geometries
STEP = 1e-7


def test_twin_gradient_against_central_differences():
    """The twin's analytic g = d h0 / d x01 against float64 central differences of step 1e-7 on 2000 uniform points.  Inside a grid
    cell the interpolation is linear along each axis and the network is piecewise linear, so the difference quotient is exact up to
    rounding (1e-16 |h0| / 1e-7) wherever the bracket crosses neither a cell face nor a ReLU gate; those points are left out, and
    they are few: a face lies within two steps with probability 3 * 4e-7 * sum(scales) = 0.7 % for this geometry."""
    meta_o = hg.oracle_meta(GEOMETRY)
    assert meta_o.n_levels * meta_o.n_features == 32
    g = torch.Generator().manual_seed(2024)
    table = ((torch.rand(meta_o.n_params, generator=g, dtype=torch.float64) * 2 - 1) * 0.1)
    params = nr.base_weights()
    x = torch.rand(2000, 3, generator=g, dtype=torch.float64) * 0.998 + 0.001
    grad, _, pre0 = nr.field_logit_grad64(x, table, meta_o, params)
    near_face = torch.zeros(x.shape[0], dtype=torch.bool)
    for sc in meta_o.scales:
        p = x * float(np.float32(sc)) + 0.5
        near_face |= ((p - p.round()).abs() <= 2 * STEP * float(np.float32(sc))).any(-1)
    gate_moves = torch.zeros(x.shape[0], dtype=torch.bool)
    fd = torch.zeros_like(grad)
    with torch.no_grad():
        for k in range(3):
            e = torch.zeros(3, dtype=torch.float64)
            e[k] = STEP
            hp, pp = nr.field_logit64(x + e, table, meta_o, params)
            hm, pm = nr.field_logit64(x - e, table, meta_o, params)
            fd[:, k] = (hp - hm) / (2 * STEP)
            gate_moves |= ((pp > 0) != (pm > 0)).any(1) | ((pp > 0) != (pre0 > 0)).any(1)
    excluded = near_face | gate_moves
    share = float(excluded.float().mean())
    keep = ~excluded
    err = float((grad[keep] - fd[keep]).abs().max() / grad.abs().max())
    print("NORMALS_TWIN excluded share", share, "near a face", int(near_face.sum()), "gate moves", int(gate_moves.sum()),
          "max |g|", float(grad.abs().max()), "error / max |g|", err)
    assert share <= 0.05, share
    assert err < 1e-6, err


def test_twin_compositing_edge_cases():
    """Exactly zero for a ray without samples, for zero-gradient samples and for a ray whose weights are all zero."""
    rng = np.random.default_rng(0)
    lens = [0, 5, 7, 3]
    n = sum(lens)
    packed = np.array([[sum(lens[:i]), c] for i, c in enumerate(lens)], dtype=np.int64)
    ts = np.concatenate([np.arange(c) * 0.1 + 0.5 for c in lens])
    te = ts + 0.1
    sigma = rng.uniform(0.5, 5.0, n)
    g = rng.normal(size=(n, 3))
    g[5:12] = 0.0                        # ray 2: zero gradients
    sigma[12:15] = 0.0                   # ray 3: zero weights
    for renorm in (True, False):
        N = nr.composite_normals(ts, te, sigma, g, packed, renormalize=renorm)
        assert np.all(N[0] == 0.0) and np.all(N[2] == 0.0) and np.all(N[3] == 0.0)
        assert np.all(np.isfinite(N))
    N = nr.composite_normals(ts, te, sigma, g, packed)
    assert abs(np.linalg.norm(N[1]) - 1.0) < 1e-9
    assert np.all(nr.sample_normals(np.zeros((2, 3))) == 0.0)
    # world space through an aabb: the Jacobian is diag(1 / extent), and a sample outside the box contributes nothing
    aabb = [-1.0, -2.0, -4.0, 1.0, 2.0, 4.0]
    gw = nr.world_gradient64(np.array([[0.1, 0.2, 0.3], [5.0, 0.0, 0.0]]), np.ones((2, 3)), False, aabb)
    assert np.allclose(gw[0], [0.5, 0.25, 0.125]) and np.all(gw[1] == 0.0)
    # ... and through the contraction: identity / 4 inside the unit ball
    gw = nr.world_gradient64(np.array([[0.1, 0.2, 0.3]]), np.array([[1.0, 2.0, 3.0]]), True, None)
    assert np.allclose(gw[0], [0.25, 0.5, 0.75])


def _declared(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lse_hip.h")).read(), flags=re.S)
    m = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
    assert m, f"include/lse_hip.h does not declare {name}"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_libraries_and_binding_agree():
    from lsenerf_amd import _lib
    args = _declared("lse_density_logit_grad")
    assert len(args) == 7 == len(_lib.SIGNATURES["lse_density_logit_grad"])
    assert args[-3:] == ["int64_t n", "const int64_t *n_dev", "lse_stream_t stream"]
    assert not any("d_out" in a or a.endswith("*out") for a in args)          # no seed, no forward output
    args = _declared("lse_eval_composite_normals")
    assert len(args) == 13 == len(_lib.SIGNATURES["lse_eval_composite_normals"])
    assert args[-1] == "lse_stream_t stream" and args[-2] == "float *out_normals" and args[3] == "const float *d_x01"
    for name in ("lse_density_logit_grad", "lse_eval_composite_normals"):
        assert name in _exported(_lib.LIB_PATH) and name in _exported(_lib.DEV_LIB_PATH), name
        assert hasattr(_lib.load(), name)
    assert (_lib.LSE_NORMALS_WORLD, _lib.LSE_NORMALS_RENORMALIZE) == (1, 2)
    hdr = open(os.path.join(ROOT, "include", "lse_hip.h")).read()
    assert "#define LSE_NORMALS_WORLD 1" in hdr and "#define LSE_NORMALS_RENORMALIZE 2" in hdr
    assert _lib.LSE_ABI_VERSION == 6                                          # additive


def test_argument_checks_need_no_device():
    import dataclasses
    from lsenerf_amd import _lib, ops
    lib = _lib.load()
    one = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    base = ops.MlpMeta(32, 64, 1, _lib.LSE_ACT_NONE, _lib.LSE_IN_LEVELMAJOR)

    def rc_of(meta, n=8, params=one):
        d = meta.desc()
        return lib.lse_density_logit_grad(ctypes.byref(d), params, one, one, n, None, None)

    assert rc_of(base, n=0) == 0 and rc_of(dataclasses.replace(base, in_layout=_lib.LSE_IN_ROWMAJOR), n=0) == 0
    refused = {
        "width 32": (dict(meta=dataclasses.replace(base, width=32)), -3),
        "the head": (dict(meta=ops.MlpMeta(16, 64, 2)), -3),
        "two hidden layers": (dict(meta=dataclasses.replace(base, n_hidden_layers=2)), -3),
        "sigmoid output": (dict(meta=dataclasses.replace(base, out_activation=_lib.LSE_ACT_SIGMOID)), -3),
        "bf16x3": (dict(meta=dataclasses.replace(base, arith=_lib.LSE_MLP_ARITH_BF16X3)), -3),
        "bf16x1": (dict(meta=dataclasses.replace(base, arith=_lib.LSE_MLP_ARITH_BF16X1)), -3),
        "f32 arithmetic": (dict(meta=dataclasses.replace(base, arith=_lib.LSE_MLP_ARITH_F32_MFMA)), -3),
        "refused even without samples": (dict(meta=dataclasses.replace(base, width=32), n=0), -3),
        "negative n": (dict(meta=base, n=-1), -1),
        "null params": (dict(meta=base, params=None), -1),
    }
    for what, (kw, code) in refused.items():
        assert rc_of(**kw) == code, what
        assert b"lse_density_logit_grad" in lib.lse_last_error(), what
    assert ops.density_logit_shape(base) and not ops.density_logit_shape(ops.MlpMeta(16, 64, 2))
    # the compositing entry point: flags and pointers
    call = lambda flags, n=4, o=None, d=None, out=one: lib.lse_eval_composite_normals(one, one, one, one, one, n, o, d, 1, None, flags,
                                                                                     out, None)
    assert call(0, n=0) == 0
    assert call(4) == -1 and b"unknown flags" in lib.lse_last_error()
    assert call(_lib.LSE_NORMALS_WORLD) == -1 and b"rays_o" in lib.lse_last_error()
    assert call(0, n=-1) == -1 and call(0, out=None) == -1
    assert lib.lse_eval_composite_normals(one, one, one, one, one, 4, one, one, 0, None, _lib.LSE_NORMALS_WORLD, one, None) == -1
    assert b"h_aabb" in lib.lse_last_error()


def test_config_field():
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig
    from lsenerf_amd.field import FieldHeadNames
    assert LSENeRFModelConfig().eval_normals == "off"
    assert FieldHeadNames.NORMALS.value == "normals"
    box = torch.tensor([[-1.0, -1, -1], [1, 1, 1]])
    small = dict(grid_levels=1, grid_resolution=16, log2_hashmap_size=12)
    for mode in ("field", "world"):
        with pytest.raises(ValueError, match="eval_normals"):
            LSENeRFModel(LSENeRFModelConfig(eval_normals=mode, eval_early_stop_eps=1e-4, **small), box, 4)
    with pytest.raises(ValueError, match="eval_normals"):
        LSENeRFModel(LSENeRFModelConfig(eval_normals="camera", **small), box, 4)
    m = LSENeRFModel(LSENeRFModelConfig(eval_normals="field", **small), box, 4)
    assert not m.eval_normals_on()                  # training mode never computes normals
    assert m.eval().eval_normals_on()
    assert not LSENeRFModel(LSENeRFModelConfig(**small), box, 4).eval().eval_normals_on()


def test_normals_colormap():
    from lsenerf_amd.evaluation import normals_colormap
    n = torch.tensor([[[1.0, 0.0, -1.0], [0.0, 0.0, 0.0]]])
    acc = torch.tensor([[[1.0], [0.0]]])
    assert torch.equal(normals_colormap(n, acc), torch.tensor([[[1.0, 0.5, 0.0], [1.0, 1.0, 1.0]]]))


def test_the_ops_have_no_cpu_path():
    from lsenerf_amd import _lib, ops
    meta = ops.MlpMeta(32, 64, 1)
    with pytest.raises(_lib.LseHipError, match="must live on the GPU"):
        ops.density_logit_grad(torch.zeros(meta.n_params), torch.zeros(8, 32), meta, 8)
    z = torch.zeros(4)
    with pytest.raises(_lib.LseHipError, match="must live on the GPU"):
        ops.eval_composite_normals(z, z, z, torch.zeros(4, 3), torch.tensor([[0, 4]]), torch.zeros(1, 3))
    with pytest.raises(_lib.LseHipError, match="must live on the GPU"):
        ops.hash_bwd_input(torch.zeros(4, 3), torch.zeros(16, 4, 2), torch.zeros(64), ops.make_grid_meta(log2_hashmap_size=4))
