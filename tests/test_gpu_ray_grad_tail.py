"""lse_ray_grad_from_dx01 (d(pos) formed per sample and summed per ray in one launch) against lse_positions_bwd ->
lse_ray_grad_reduce: d_o and d_d bit for bit, for rays that are empty, shorter than, exactly and longer than a wave, with the
contraction (inside and beyond |p| = 1) and with aabb normalisation (samples inside and outside the box), and with either output
left out."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 63, 64, 65, 200, 0, 130, 2)      # samples per ray: nine rays = three workgroups of four waves, the last one ragged


def _case(seed):
    g = torch.Generator().manual_seed(seed)
    cnt = torch.tensor(COUNTS, dtype=torch.int64)
    R, n = len(COUNTS), int(cnt.sum())
    packed = torch.stack([torch.cumsum(cnt, 0) - cnt, cnt], dim=1)
    ri = torch.repeat_interleave(torch.arange(R, dtype=torch.int32), cnt)
    o = torch.rand(R, 3, generator=g) - 0.5
    d = torch.randn(R, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    ts = torch.rand(n, generator=g) * 3.0          # mid-points up to 3 units along the ray: |p| from < 0.5 to > 3
    te = ts + 0.01 + 0.05 * torch.rand(n, generator=g)
    dx01 = torch.randn(n, 3, generator=g)
    return tuple(t.cuda().contiguous() for t in (o, d, ri, ts, te, packed, dx01)), R, n


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("mode", ["contraction", "aabb"])
def test_ray_grad_from_dx01_equals_the_two_launches(mode):
    from lsenerf_amd import _lib, ops
    (o, d, ri, ts, te, packed, dx01), R, n = _case(7 if mode == "contraction" else 8)
    contraction = int(mode == "contraction")
    aabb = None if contraction else (ctypes.c_float * 6)(-1.0, -0.8, -1.2, 1.0, 1.1, 0.9)
    # the cases the kernel branches on are all present
    p = o[ri.long()] + d[ri.long()] * ((ts + te) / 2)[:, None]
    mag = p.abs().amax(-1)
    assert int((mag < 1).sum()) > 20 and int((mag > 1).sum()) > 20
    if not contraction:
        lo, hi = torch.tensor(list(aabb)[:3]).cuda(), torch.tensor(list(aabb)[3:]).cuda()
        inside = ((p > lo) & (p < hi)).all(-1)
        assert int(inside.sum()) > 20 and int((~inside).sum()) > 20
    st = ops._stream()
    d_pos = torch.empty(n, 3, device="cuda")
    _lib.call("lse_positions_bwd", _P(o), _P(d), _P(ri), _P(ts), _P(te), n, None, contraction, aabb, _P(dx01), _P(d_pos), st)
    ref_o, ref_d = torch.full((R, 3), 7.0, device="cuda"), torch.full((R, 3), 7.0, device="cuda")
    _lib.call("lse_ray_grad_reduce", _P(d_pos), _P(ts), _P(te), _P(packed), R, _P(ref_o), _P(ref_d), st)
    assert float(d_pos.abs().max()) > 0 and (contraction or bool((d_pos == 0).all(-1).any()))
    for want_o, want_d in ((True, True), (True, False), (False, True)):
        got_o = torch.full((R, 3), -3.0, device="cuda") if want_o else None
        got_d = torch.full((R, 3), -3.0, device="cuda") if want_d else None
        _lib.call("lse_ray_grad_from_dx01", _P(o), _P(d), _P(ts), _P(te), _P(packed), R, contraction, aabb, _P(dx01), _P(got_o),
                  _P(got_d), st)
        if want_o:
            assert torch.equal(got_o, ref_o), (mode, "d_o", (got_o - ref_o).abs().max())
        if want_d:
            assert torch.equal(got_d, ref_d), (mode, "d_d", (got_d - ref_d).abs().max())
    empty = [r for r, c in enumerate(COUNTS) if c == 0]
    assert float(ref_o[empty].abs().max()) == 0.0 and float(ref_d[empty].abs().max()) == 0.0


def test_positions_backward_takes_the_fused_tail_on_the_ray_path(monkeypatch):
    """ops.positions: with rays the backward is the one launch (same d_o / d_d as with the switch off); direct positions keep
    lse_positions_bwd."""
    from lsenerf_amd import _lib, ops
    (o, d, ri, ts, te, packed, dx01), R, n = _case(9)
    calls = []
    real_call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    res = []
    for on in (False, True):
        monkeypatch.setattr(ops, "FUSED_RAY_GRAD", on)
        oo, dd = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
        x01, _ = ops.positions(oo, dd, ri, ts, te, packed, contraction=True)
        del calls[:]
        (x01 * dx01).sum().backward()
        assert calls == (["lse_ray_grad_from_dx01"] if on else ["lse_positions_bwd", "lse_ray_grad_reduce"]), calls
        res.append((oo.grad, dd.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    pos = (o[ri.long()] + d[ri.long()] * ((ts + te) / 2)[:, None]).contiguous().requires_grad_(True)
    x01, _ = ops.positions(pos, None, None, None, None, None, contraction=True)
    del calls[:]
    (x01 * dx01).sum().backward()
    assert calls == ["lse_positions_bwd"] and pos.grad.shape == (n, 3)
