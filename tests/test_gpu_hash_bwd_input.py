"""``lse_hash_bwd_input``: the hash grid's input gradient alone, for a frozen table (no table gradient, no workspace, no atomics).
Inputs and comparison are those of tests/hash_geometry_cases.py against oracle/hashgrid.py, tolerances of tests/util.py unchanged:
every kind of geometry (dense, hashed, non-power-of-two sizes, more than 16 levels, levels that start off 64-byte lines),
device-side sample counts into sentinel-filled outputs, positions outside the unit cube, bit-identical repeat calls, agreement
with the d(x) of ``lse_hash_bwd_ex``, and a table that the call leaves bit-unchanged."""
import ctypes

import pytest
import torch

from tests import hash_geometry_cases as hc
from tests.util import TOL_GRAD, nmax_err

pytestmark = pytest.mark.gpu

GEOMS = [hc.DEFAULT, "L1", "b2_m2048", "b64_m4096", "T4_L4", "b16_m128_L8_T22", "L24_T14", "b16_m16_L4"]


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _meta(name):
    from lsenerf_amd import ops
    return ops.make_grid_meta(**hc.geometry_kwargs(name))


def _bwd_input(meta, x, dy, table, dx=None, cap=None, cnt=None):
    from lsenerf_amd import _lib, ops
    desc = meta.desc()
    if dx is None:
        dx = torch.full_like(x, 7.0)
    _lib.call("lse_hash_bwd_input", ctypes.byref(desc), _P(x), _P(dy), _P(table), _P(dx), x.shape[0] if cap is None else cap,
              _P(cnt), ops._stream())
    return dx


def _report(tag, res):
    print("HASHBWDIN " + tag + " " + " ".join(f"{k}={v:.3e}" for k, v in res.items()))


@pytest.mark.parametrize("name", GEOMS)
def test_input_gradient_every_geometry(name):
    """d(x) against the oracle; the same call twice gives the same bits; the table is not written; and the d(x) of the full
    backward (lse_hash_bwd_ex) on the same inputs agrees within TOL_GRAD."""
    from lsenerf_amd import _lib, ops
    ref = hc.reference(name)
    meta, meta_o = _meta(name), ref["meta_o"]
    assert list(meta.offsets) == meta_o.offsets
    xg, tg = ref["x"].cuda(), ref["table"].cuda()
    dy = hc.level_major(ref["w"]).cuda()
    t_before = tg.clone()
    dx = _bwd_input(meta, xg, dy, tg)
    res = hc.check_against_oracle(None, None, dx, ref, meta_o)
    dx2 = _bwd_input(meta, xg, dy, tg)
    assert torch.equal(dx, dx2)                                   # fixed summation order, no atomics
    assert torch.equal(tg.view(torch.int32), t_before.view(torch.int32))
    # the full backward's d(x): same cells, same formula, another summation order
    desc = meta.desc()
    dt, dx_ex = torch.zeros_like(tg), torch.full_like(xg, 7.0)
    opts = ops.hash_bwd_opts_with_workspace(desc, xg.device)
    _lib.call("lse_hash_bwd_ex", ctypes.byref(desc), _P(xg), _P(dy), _P(tg), _P(dt), _P(dx_ex), 0, 0, meta.n_levels, xg.shape[0],
              None, ctypes.byref(opts), ops._stream())
    res["vs_ex"] = nmax_err(dx, dx_ex)
    _report(name, res)
    assert res["vs_ex"] < TOL_GRAD, res


@pytest.mark.parametrize("name", GEOMS)
def test_input_gradient_device_side_counts(name):
    """Arrays of capacity N (the level stride of dy), the count on the device: rows below the count against the oracle on the
    truncated arrays, rows at or beyond it still hold the sentinel."""
    ref = hc.reference(name)
    meta, meta_o = _meta(name), ref["meta_o"]
    cap = ref["x"].shape[0]
    xg, tg = ref["x"].cuda(), ref["table"].cuda()
    dy = hc.level_major(ref["w"]).cuda()
    assert not bool(ref["on_face"][0])
    for n_dev in (0, 1, cap - 777, cap, cap + 5):
        cnt = torch.tensor([n_dev], dtype=torch.int64, device="cuda")
        dx = _bwd_input(meta, xg, dy, tg, cap=cap, cnt=cnt)
        m = min(n_dev, cap)
        assert bool((dx[m:] == 7.0).all()), n_dev
        if m == 0:
            continue
        sub = ref if m == cap else {**ref, "dx": ref["dx"][:m], "on_face": ref["on_face"][:m]}      # d(x) is per sample
        _report(f"{name} n_dev={n_dev}", hc.check_against_oracle(None, None, dx[:m], sub, meta_o))


@pytest.mark.parametrize("name", [hc.DEFAULT, "T4_L4"])
def test_input_gradient_out_of_range_positions(name):
    """Outside the unit cube the cell is the one the forward picks: wrapping integer coordinates, exact modulo."""
    ref = hc.reference_out_of_range(name)
    meta = _meta(name)
    xg, tg = ref["x"].cuda(), ref["table"].cuda()
    dx = _bwd_input(meta, xg, hc.level_major(ref["w"]).cuda(), tg)
    _report(f"{name} out of range", hc.check_against_oracle(None, None, dx, ref, ref["meta_o"]))


def test_frozen_table_through_autograd_takes_the_input_kernel(monkeypatch):
    """ops.hash_encode with a table that does not require a gradient: one lse_hash_bwd_input, no scatter, no table-sized tensor
    handed back; with neither input requiring one, no backward at all."""
    from lsenerf_amd import _lib, ops
    ref = hc.reference(hc.DEFAULT)
    meta = _meta(hc.DEFAULT)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    xg = ref["x"].cuda().requires_grad_(True)
    tg = ref["table"].cuda()
    y = hc.sample_major(ops.hash_encode(xg, tg, meta))
    (y * ref["w"].cuda()).sum().backward()
    assert calls.count("lse_hash_bwd_input") == 1 and not [c for c in calls if c in ("lse_hash_bwd", "lse_hash_bwd_levels", "lse_hash_bwd_ex")]
    assert tg.grad is None
    hc.check_against_oracle(y.detach(), None, xg.grad, ref, ref["meta_o"])
