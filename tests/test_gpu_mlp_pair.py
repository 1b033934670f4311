"""lse_mlp_fwd_pair (base MLP + density head and head MLP on the same samples in one launch, csrc/mlp_x6.h) against the two
lse_mlp_fwd launches it replaces: h, sigma and the head output bit for bit at the tile edges, past one tile per wave, with a
device-side count on poison-filled outputs; gradients through ``ops.fused_mlp_pair`` against the two-function path; and a model
rendered with the switch on and off."""
import ctypes
import functools

import pytest
import torch

from tests.util import TOL_GRAD, TOL_GRAD_BLOCK, blockwise_nmax_err, nmax_err, random_binaries, random_rays, row_bounds

pytestmark = pytest.mark.gpu

SCALE = 0.7                                     # density scale (average_init_density)
RAY_LENGTHS = (1, 3, 40, 64, 200, 7, 33, 31)    # samples per row of row_bias, cycled: rows straddle the 32-sample tiles
POISON = -12345.0


def _metas(layout):
    from lsenerf_amd import _lib, ops
    base = ops.MlpMeta(32, 64, 1, _lib.LSE_ACT_NONE, layout)
    head = ops.MlpMeta(16, 64, 2, _lib.LSE_ACT_SIGMOID, _lib.LSE_IN_ROWMAJOR, w0_ld=64, w0_col=15, w0_mask_col0=1)
    return base, head


@functools.lru_cache(maxsize=None)
def _weights():
    g = torch.Generator().manual_seed(11)
    u = lambda m, fan: ((torch.rand(m, generator=g) * 2 - 1) * (6.0 / fan) ** 0.5).cuda()
    base = torch.cat([u(64 * 32, 96), u(16 * 64, 80)])
    head = torch.cat([u(64 * 64, 128), u(64 * 64, 128), u(16 * 64, 80)])
    return base, head


@functools.lru_cache(maxsize=None)
def _inputs(n: int, levelmajor: bool):
    """Inputs of one sample count and their reference outputs (two lse_mlp_fwd launches), computed once and never modified."""
    from lsenerf_amd import _lib, ops
    g = torch.Generator().manual_seed(1000 + n)
    y_rows = torch.randn(n, 32, generator=g) * 0.5
    y = (y_rows.view(n, 16, 2).permute(1, 0, 2).contiguous() if levelmajor else y_rows).cuda()
    sel = (torch.rand(n, generator=g) < 0.7).to(torch.uint8).cuda()
    lens, total = [], 0
    while total < n:
        lens.append(min(RAY_LENGTHS[len(lens) % len(RAY_LENGTHS)], n - total))
        total += lens[-1]
    cnt = torch.tensor(lens, dtype=torch.int64)
    packed = torch.stack([torch.cumsum(cnt, 0) - cnt, cnt], dim=1).cuda()
    idx = torch.repeat_interleave(torch.arange(len(lens), dtype=torch.int32), cnt).cuda()
    row_bias = (torch.randn(len(lens), 64, generator=g) * 0.3).cuda()
    base_meta, head_meta = _metas(_lib.LSE_IN_LEVELMAJOR if levelmajor else _lib.LSE_IN_ROWMAJOR)
    bp, hp = _weights()
    ref = {}
    with torch.no_grad():
        for name, s in (("sel", sel), ("nosel", None)):
            h, sigma = ops.fused_mlp(bp, y, base_meta, n, density=(s, SCALE))
            out = ops.fused_mlp(hp, h, head_meta, n, row_bias, idx, packed, out_cols=4)
            ref[name] = (h, sigma, out)
    return dict(y=y, sel=sel, idx=idx, packed=packed, row_bias=row_bias, base_meta=base_meta, head_meta=head_meta, ref=ref)


# 1 .. 95: the edges of the 16-sample column tiles and the 32-sample wave tiles; 4113: many workgroups, ragged last tile;
# 262189: the forward grid caps at 512 workgroups x 8 waves, so more than 4096 tiles make a wave walk more than one (prefetch path)
@pytest.mark.parametrize("n", [1, 16, 31, 32, 33, 95, 4113, 262189])
def test_pair_equals_two_launches_bitwise(n):
    from lsenerf_amd import ops
    bp, hp = _weights()
    for levelmajor in (True, False):
        inp = _inputs(n, levelmajor)
        for name, s in (("sel", inp["sel"]), ("nosel", None)):
            with torch.no_grad():
                h, sigma, out = ops.fused_mlp_pair(bp, inp["y"], s, SCALE, inp["base_meta"], hp, inp["head_meta"], n,
                                                   inp["row_bias"], inp["idx"], inp["packed"], out_cols=4)
            rh, rs, ro = inp["ref"][name]
            assert h.shape == (n, 16) and sigma.shape == (n,) and out.shape == (n, 4)
            assert torch.equal(h, rh), (n, levelmajor, name, "h")
            assert torch.equal(sigma, rs), (n, levelmajor, name, "sigma")
            assert torch.equal(out, ro), (n, levelmajor, name, "head output")
    # the other store layout and bias addressing of the head epilogue / prologue: padded 16-column output, one bias row per sample
    inp = _inputs(n, True)
    rb = inp["row_bias"][inp["idx"].long()].contiguous()
    with torch.no_grad():
        h, sigma, out = ops.fused_mlp_pair(bp, inp["y"], inp["sel"], SCALE, inp["base_meta"], hp, inp["head_meta"], n, rb, None, None,
                                           out_cols=16)
        ro = ops.fused_mlp(hp, inp["ref"]["sel"][0], inp["head_meta"], n, rb, None, None, out_cols=16)
    assert torch.equal(h, inp["ref"]["sel"][0]) and torch.equal(sigma, inp["ref"]["sel"][1]) and torch.equal(out, ro)
    assert torch.equal(out[:, :4], inp["ref"]["sel"][2])


@pytest.mark.parametrize("short", [37, None])
def test_device_side_count_leaves_the_tail_alone(short):
    """Capacity n with n_dev = n - 37 and n_dev = 0: the prefix equals the reference path, everything at or beyond the count keeps
    its poison."""
    from lsenerf_amd import ops
    n = 4113
    m = n - short if short is not None else 0
    bp, hp = _weights()
    for levelmajor in (True, False):
        inp = _inputs(n, levelmajor)
        n_dev = torch.tensor([m], dtype=torch.int64, device="cuda")
        h = torch.full((n, 16), POISON, device="cuda")
        sigma = torch.full((n,), POISON, device="cuda")
        out = torch.full((n, 4), POISON, device="cuda")
        bdesc, hdesc = inp["base_meta"].desc(), inp["head_meta"].desc()
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        ops._call_n("lse_mlp_fwd_pair", n_dev, ctypes.byref(bdesc), P(bp), P(inp["y"]), P(inp["sel"]), SCALE, ctypes.byref(hdesc),
                    P(hp), P(inp["row_bias"]), P(inp["idx"]), P(h), P(sigma), P(out), 4, n, ops._stream())
        rh, rs, ro = inp["ref"]["sel"]
        assert torch.equal(h[:m], rh[:m]) and torch.equal(sigma[:m], rs[:m]) and torch.equal(out[:m], ro[:m])
        assert bool((h[m:] == POISON).all()) and bool((sigma[m:] == POISON).all()) and bool((out[m:] == POISON).all())


def test_backward_through_the_pair_equals_the_two_function_path():
    """One backward at n = 4113.  The pair's backward issues the same two lse_mlp_bwd launches on the same inputs.  Found bitwise
    equal on MI355X: d_y (atomic-free per sample).  d_row_bias is reduced per row inside the kernel and the weight gradients over
    all samples, both with float atomics whose order varies from launch to launch: held to the bars of tests/util.py."""
    from lsenerf_amd import ops
    n = 4113
    inp = _inputs(n, True)
    g = torch.Generator().manual_seed(5)
    g_out, g_sigma = torch.randn(n, 4, generator=g).cuda(), torch.randn(n, generator=g).cuda()
    res = []
    for pair in (False, True):
        bp, hp = (w.clone().requires_grad_(True) for w in _weights())
        y, rb = inp["y"].clone().requires_grad_(True), inp["row_bias"].clone().requires_grad_(True)
        if pair:
            assert ops.mlp_pair_usable(bp, y, inp["base_meta"], hp, inp["head_meta"], rb, inp["idx"], inp["packed"])
            h, sigma, out = ops.fused_mlp_pair(bp, y, inp["sel"], SCALE, inp["base_meta"], hp, inp["head_meta"], n, rb, inp["idx"],
                                               inp["packed"], out_cols=4)
        else:
            h, sigma = ops.fused_mlp(bp, y, inp["base_meta"], n, density=(inp["sel"], SCALE))
            out = ops.fused_mlp(hp, h, inp["head_meta"], n, rb, inp["idx"], inp["packed"], out_cols=4)
        ((out * g_out).sum() + (sigma * g_sigma).sum()).backward()
        res.append(dict(bp=bp.grad, hp=hp.grad, y=y.grad, rb=rb.grad, out=out.detach(), sigma=sigma.detach()))
    ref, got = res
    assert torch.equal(got["out"], ref["out"]) and torch.equal(got["sigma"], ref["sigma"])
    assert torch.equal(got["y"], ref["y"]), "d_y: atomic-free per sample"
    print("d_row_bias bitwise equal:", torch.equal(got["rb"], ref["rb"]), " d_base_params:", torch.equal(got["bp"], ref["bp"]),
          " d_head_params:", torch.equal(got["hp"], ref["hp"]))
    bounds = {"bp": row_bounds(64, 32)[:-1] + [64 * 32 + r * 64 for r in range(17)],
              "hp": row_bounds(64 + 64 + 16, 64), "rb": row_bounds(inp["row_bias"].shape[0], 64)}
    for k in ("bp", "hp", "rb"):
        e, eb = nmax_err(got[k], ref[k], 1e-12), blockwise_nmax_err(got[k], ref[k], bounds[k])
        print(f"d_{k}: nmax {e:.3e} blockwise {eb:.3e}")
        assert e < TOL_GRAD and eb < TOL_GRAD_BLOCK, (k, e, eb)
    # head columns outside the first-layer view [15, 31) receive nothing from either path
    w0 = got["hp"][: 64 * 64].view(64, 64)
    assert float(w0[:, :16].abs().max()) == 0.0 and float(w0[:, 31:].abs().max()) == 0.0


def _model():
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig
    torch.manual_seed(96)
    cfg = LSENeRFModelConfig(grid_levels=2, grid_resolution=32, log2_hashmap_size=15)
    m = LSENeRFModel(cfg, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 16)
    with torch.no_grad():
        m.field.mlp_base_grid.params.mul_(300.0)
    m = m.cuda().train()
    m.occupancy_grid.binaries.copy_(random_binaries(2, 32, 0.5, 3).cuda())
    m.occupancy_grid.occs.copy_(m.occupancy_grid.binaries.flatten().float() * 0.5)
    return m


def test_model_renders_the_same_with_the_switch_on_and_off(monkeypatch):
    """A 64-ray model through render_packed: eager counts, deferred counts and evaluation, pair on and off."""
    from lsenerf_amd import RayBundle, _lib, ops
    m = _model()
    R = 64
    o, d = random_rays(R, seed=4)
    g = torch.Generator().manual_seed(1)
    rb = RayBundle(origins=o.cuda(), directions=d.cuda(), camera_indices=torch.zeros(R, 1, dtype=torch.long, device="cuda"),
                   metadata={"appearance_id": torch.randint(0, 16, (R,), generator=g).cuda()})
    jit = torch.rand(R, generator=g).cuda()
    calls = []
    real_call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    for mode in ("eager", "deferred", "eval"):
        m.train(mode != "eval")
        m.deferred_counts = mode == "deferred"
        outs = []
        for on in (False, True):
            monkeypatch.setattr(ops, "MLP_FWD_PAIR", on)
            del calls[:]
            if mode == "eval":
                with torch.no_grad():
                    out = m.exec_get_outputs(rb)
            else:
                out = m.exec_get_outputs(rb, jitter=jit)
            assert ("lse_mlp_fwd_pair" in calls) == on, (mode, on, calls)
            outs.append({k: v.detach().clone() for k, v in out.items()})
        assert int(outs[0]["num_samples_per_ray"].sum()) > 20 * R
        for k in ("rgb", "accumulation", "depth", "num_samples_per_ray"):
            assert torch.equal(outs[0][k], outs[1][k]), (mode, k)
    m.occupancy_grid.check_deferred_overflow()
