"""``lse_density_logit_grad`` (csrc/mlp_x6.h: the one-hot-seeded instance of ``mlp_bwd_input_kernel``): d out[:, 0] / d in of the base
network against the float64 twin (tests/normals_ref.py) and against the route it replaces -- ``lse_mlp_bwd_input`` fed a seed of
(1, 0, .., 0) -- whose own error against float64 is the yardstick: e_new <= max(2 e_old, 1e-6) and e_new < TOL_GRAD."""
import ctypes
import dataclasses
import functools

import pytest
import torch

from tests import normals_ref as nr
from tests.util import TOL_GRAD, nmax_err

pytestmark = pytest.mark.gpu

SIZES = (1, 5, 16, 17, 32, 33, 100, 2049)      # column tiles of 16, wave tiles of 32, workgroups of 128 samples; 2049: 17 workgroups
LAYOUTS = ("lm", "rm")
SENTINEL = -12345.0


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _meta(layout, **kw):
    from lsenerf_amd import _lib, ops
    return ops.MlpMeta(32, 64, 1, _lib.LSE_ACT_NONE, _lib.LSE_IN_LEVELMAJOR if layout == "lm" else _lib.LSE_IN_ROWMAJOR, **kw)


def _to_rows(layout, x):
    return x.permute(1, 0, 2).reshape(x.shape[1], 32) if layout == "lm" else x


@functools.lru_cache(maxsize=None)
def _params():
    return nr.base_weights().cuda()


@functools.lru_cache(maxsize=None)
def _case(layout, n):
    """Inputs of one (layout, sample count), the float64 gradient, the gate-band mask and the seeded old route's result; computed
    once, never modified."""
    from lsenerf_amd import ops
    g = torch.Generator(device="cuda").manual_seed(500 + n + 7 * LAYOUTS.index(layout))
    x = torch.randn((16, n, 2) if layout == "lm" else (n, 32), generator=g, device="cuda") * 0.5
    ref, near = nr.logit_grad_of_features64(_to_rows(layout, x).cpu(), _params().cpu())
    seed = torch.zeros(n, 16, device="cuda")
    seed[:, 0] = 1.0
    old = torch.full_like(x, SENTINEL)
    ops.mlp_bwd_input(_params(), x, _meta(layout), n, None, 16, seed, d_in=old)
    return dict(layout=layout, n=n, x=x, ref=ref, near=near, old=old)


def _new(c, n_dev=None, params=None):
    from lsenerf_amd import ops
    d_in = torch.full_like(c["x"], SENTINEL)
    got = ops.density_logit_grad(_params() if params is None else params, c["x"], _meta(c["layout"]), c["n"], d_in=d_in, n_dev=n_dev)
    assert got is d_in
    return d_in


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", SIZES)
def test_against_float64_and_the_seeded_route(layout, n):
    c = _case(layout, n)
    d_in = _new(c)
    assert not bool((d_in == SENTINEL).any()), "a row below the count was not written"
    keep = ~c["near"]                                    # a float64 gate may differ from the float32 one inside the band
    rows, old = _to_rows(layout, d_in).cpu()[keep], _to_rows(layout, c["old"]).cpu()[keep]
    ref = c["ref"][keep]
    assert int(keep.sum()) >= (n + 1) // 2, "the seeded inputs should leave most samples outside the gate band"
    e_new, e_old = nmax_err(rows, ref, 1e-12), nmax_err(old, ref, 1e-12)
    print("DENSITY_LOGIT_GRAD", layout, n, "inside the gate band:", int(c["near"].sum()), "vs float64: new", e_new, "seeded", e_old)
    assert float(ref.abs().max()) > 0
    assert e_new < TOL_GRAD, (layout, n, e_new)
    assert e_new <= max(2.0 * e_old, 1e-6), (layout, n, e_new, e_old)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("short", [0, 1, 33, 2048])
def test_device_side_count(layout, short):
    """Capacity 2049 with a count below it: the prefix as in the full call, every row at or beyond the count keeps its sentinel."""
    c = _case(layout, 2049)
    full = _to_rows(layout, _new(c))
    rows = _to_rows(layout, _new(c, n_dev=torch.tensor([short], dtype=torch.int64, device="cuda")))
    assert torch.equal(rows[:short].view(torch.int32), full[:short].view(torch.int32))
    assert bool((rows[short:] == SENTINEL).all())


@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_calls_give_the_same_bits(layout):
    c = _case(layout, 2049)
    assert torch.equal(_new(c).view(torch.int32), _new(c).view(torch.int32))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_dead_hidden_layer_gives_exact_zeros(layout):
    """W0 <= 0 on positive inputs: every ReLU is closed, the gradient is exactly zero (and written: no sentinel is left)."""
    c = dict(_case(layout, 100))
    c["x"] = c["x"].abs() + 0.1
    params = _params().clone()
    params[:2048] = -params[:2048].abs() - 0.01
    d_in = _new(c, params=params)
    assert bool((d_in == 0.0).all())


def test_refusals_launch_nothing():
    from lsenerf_amd import _lib, ops
    lib = _lib.load()
    big = torch.zeros(1 << 16, device="cuda")                      # stands in for params and input: nothing may be read
    d_in = torch.full((64, 64), SENTINEL, device="cuda")
    base = _meta("lm")
    cases = {
        "width 32": dataclasses.replace(base, width=32),
        "16 inputs": ops.MlpMeta(16, 64, 1, _lib.LSE_ACT_NONE, _lib.LSE_IN_ROWMAJOR),
        "the head": ops.MlpMeta(16, 64, 2, _lib.LSE_ACT_SIGMOID, _lib.LSE_IN_ROWMAJOR),
        "two hidden layers": dataclasses.replace(base, n_hidden_layers=2),
        "sigmoid output": dataclasses.replace(base, out_activation=_lib.LSE_ACT_SIGMOID),
        "f32 arithmetic": dataclasses.replace(base, arith=_lib.LSE_MLP_ARITH_F32_MFMA),
        "bf16x3": dataclasses.replace(base, arith=_lib.LSE_MLP_ARITH_BF16X3),
        "bf16x1": dataclasses.replace(_meta("rm"), arith=_lib.LSE_MLP_ARITH_BF16X1),
    }
    for what, meta in cases.items():
        d = meta.desc()
        rc = lib.lse_density_logit_grad(ctypes.byref(d), _P(big), _P(big), _P(d_in), 64, None, ops._stream())
        msg = lib.lse_last_error().decode()
        assert rc == -3 and "lse_density_logit_grad" in msg, (what, rc, msg)          # LSE_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((d_in == SENTINEL).all())
    x = torch.zeros(16, 64, 2, device="cuda")
    with pytest.raises(_lib.LseHipError, match="lse_density_logit_grad"):
        ops.density_logit_grad(big, x, dataclasses.replace(base, arith=_lib.LSE_MLP_ARITH_BF16X3), 64)
