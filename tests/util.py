"""Shared helpers for the parity tests: seeded inputs, HIP-model/oracle pairs with identical parameters, error metrics.

The oracle (``oracle/``) is the checker only; everything named ``hip_*`` runs through the C-ABI on the GPU.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

# stated tolerances (normalised max error: max|a-b| / max(floor, max|b|))
TOL_FWD = 2e-5     # forward activations / renders, fp32 with different summation orders
TOL_GRAD = 3e-4    # gradients: long sums (N up to 1e5 terms) in different orders, float atomics
TOL_GRAD_BLOCK = 1e-3   # the same per block (hash level / MLP row / embedding row), each scaled by its OWN maximum


def nmax_err(a: torch.Tensor, b: torch.Tensor, floor: float = 1e-6) -> float:
    a = a.detach().double().cpu().reshape(-1)
    b = b.detach().double().cpu().reshape(-1)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.numel() == 0:
        return 0.0
    return float((a - b).abs().max() / max(floor, float(b.abs().max())))


def rel_l2(a: torch.Tensor, b: torch.Tensor, floor: float = 1e-30) -> float:
    """||a - b||_2 / ||b||_2 in float64."""
    a = a.detach().double().cpu().reshape(-1)
    b = b.detach().double().cpu().reshape(-1)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).norm() / max(floor, float(b.norm())))


def per_ray_grad_check(got: torch.Tensor, ref: torch.Tensor, tol: float = None, max_outliers: int = 1, outlier_tol: float = 1e-2):
    """Per-ray gradients [R, 3]: every ray within ``tol`` of the reference (error of the ray's worst component over the global
    maximum), except at most ``max_outliers`` rays which may be off by up to ``outlier_tol``.
    Why outliers exist at all: a ReLU gate is a step function of its pre-activation h.  Two correct float32 evaluations of h
    differ in the last bits, so when |h| < ~1e-7 * scale for some (sample, neuron) one of them opens the gate and the other does
    not, and that ONE ray's gradient changes by an O(1e-3) amount while every other ray agrees to 1e-5.  With ~1e7
    (sample, neuron) pairs per test this happens to about one pair per seed; which pair depends on the summation order of the
    implementation (f32 MFMA chain, bf16-piece products, torch's GEMM), not on its correctness."""
    tol = TOL_GRAD if tol is None else tol
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    e = (got - ref).abs().amax(-1) / ref.abs().max().clamp_min(1e-30)
    bad = int((e > tol).sum())
    assert bad <= max_outliers, f"{bad} of {e.numel()} rays beyond {tol}: worst {float(e.max()):.3e}"
    assert float(e.max()) < outlier_tol, f"outlier ray error {float(e.max()):.3e} >= {outlier_tol}"
    return float(e.max()), bad


def blockwise_nmax_err(a: torch.Tensor, b: torch.Tensor, bounds, rel_floor: float = 1e-4) -> float:
    """max over blocks [bounds[i], bounds[i+1]) of  max|a - b| / max(max|b| in the block, rel_floor * max|b| overall).

    The global-max normalisation of ``nmax_err`` lets a block whose values sit orders of magnitude below the tensor's
    maximum (a fine hash level, an MLP row, an embedding row) be entirely wrong and still pass; this one scales every block
    by its own magnitude.  ``rel_floor`` keeps blocks that are numerically empty from amplifying summation noise."""
    a = a.detach().double().cpu().reshape(-1)
    b = b.detach().double().cpu().reshape(-1)
    assert a.shape == b.shape, (a.shape, b.shape)
    gmax = float(b.abs().max()) if b.numel() else 0.0
    if gmax == 0.0:
        return float(a.abs().max()) if a.numel() else 0.0
    worst = 0.0
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        if hi <= lo:
            continue
        scale = max(float(b[lo:hi].abs().max()), rel_floor * gmax)
        worst = max(worst, float((a[lo:hi] - b[lo:hi]).abs().max()) / scale)
    return worst


def hash_level_bounds(meta, n_features: int = 2):
    """Flat-parameter boundaries of the hash-grid levels (tcnn layout: level after level, F floats per entry)."""
    return [int(o) * n_features for o in meta.offsets]


def row_bounds(n_rows: int, row_len: int):
    return [r * row_len for r in range(n_rows + 1)]


def mlp_row_bounds(mlp):
    """Row boundaries of a tcnn-layout MLP parameter vector: every output neuron of every layer is one block."""
    out, pos = [0], 0
    for (o, i) in mlp.shapes:
        for _ in range(o):
            pos += i
            out.append(pos)
    return out


def grad_errors(name: str, got: torch.Tensor, ref: torch.Tensor, bounds=None) -> Dict[str, float]:
    """The three views of a gradient comparison used throughout the GPU tests."""
    res = {f"d_{name}": nmax_err(got, ref, 1e-12), f"d_{name}_l2": rel_l2(got, ref)}
    if bounds is not None:
        res[f"d_{name}_blk"] = blockwise_nmax_err(got, ref, bounds)
    return res


def random_rays(n: int, seed: int = 0, inside: bool = False, device="cpu"):
    """origins on the radius-1.5 sphere aimed at random targets in [-0.5,0.5]^3
    (``inside``: origins uniformly in [-0.5,0.5]^3, random unit directions)."""
    g = torch.Generator().manual_seed(seed)
    if inside:
        o = torch.rand(n, 3, generator=g) - 0.5
        d = torch.randn(n, 3, generator=g)
    else:
        o = torch.randn(n, 3, generator=g)
        o = 1.5 * o / o.norm(dim=-1, keepdim=True)
        tgt = torch.rand(n, 3, generator=g) - 0.5
        d = tgt - o
    d = d / d.norm(dim=-1, keepdim=True)
    return o.to(device).contiguous(), d.to(device).contiguous()


def random_binaries(levels: int, res: int, frac: float, seed: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.rand((levels, res, res, res), generator=g) < frac


def make_model_pair(grid_levels=4, grid_resolution=128, seed=96, occupied_frac=0.3, num_levels=16, hidden=64,
                    emb_type="global_emb", num_train_data=8, contraction=True, alpha_thre=0.01, cone_angle=0.004,
                    log2_hashmap_size=19, param_scale: float = 1.0, emb_dim: int = 32):
    """(HIP model on cuda:0, ModelOracle on CPU) sharing parameters, occupancy grid and hyper-parameters."""
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig, LSEEmbeddingConfig
    from oracle.field import FieldOracle
    from oracle.model import ModelOracle

    torch.manual_seed(seed)
    cfg = LSENeRFModelConfig(grid_levels=grid_levels, grid_resolution=grid_resolution, num_levels=num_levels,
                             hidden_dim=hidden, hidden_dim_color=hidden, alpha_thre=alpha_thre, cone_angle=cone_angle,
                             log2_hashmap_size=log2_hashmap_size, disable_scene_contraction=not contraction,
                             embed_config=LSEEmbeddingConfig(embedding_type=emb_type, emb_dim=emb_dim))
    aabb = torch.tensor([[-1.0, -1, -1], [1, 1, 1]])
    hip = LSENeRFModel(cfg, aabb, num_train_data)
    if param_scale != 1.0:   # larger table values make the hash contribution visible above fp32 noise
        with torch.no_grad():
            hip.field.mlp_base_grid.params.mul_(param_scale)
    hip = hip.cuda()
    n_emb = hip.field.embedding_appearance.embedding.weight.shape[0]
    f = FieldOracle("tcnn", num_levels=num_levels, hidden_dim=hidden, hidden_dim_color=hidden,
                    log2_hashmap_size=log2_hashmap_size, num_embeddings=n_emb, contraction=contraction, aabb=aabb,
                    seed=seed, appearance_embedding_dim=emb_dim)
    sync_params_to_oracle(hip, f)
    orc = ModelOracle(f, grid_resolution=grid_resolution, grid_levels=grid_levels, alpha_thre=alpha_thre,
                      cone_angle=cone_angle)
    b = random_binaries(grid_levels, grid_resolution, occupied_frac, seed)
    occs = b.float().flatten() * 0.5
    hip.occupancy_grid.binaries.copy_(b.cuda())
    hip.occupancy_grid.occs.copy_(occs.cuda())
    hip.occupancy_grid._occ_mean_host = None
    orc.grid.binaries = b.clone()
    orc.grid.occs = occs.clone()
    assert abs(orc.render_step_size - cfg.render_step_size) < 1e-12
    return hip, orc


def sync_params_to_oracle(hip, field_oracle):
    fld = hip.field
    src = {"grid": fld.mlp_base_grid.params, "base": fld.mlp_base_mlp.params, "head": fld.mlp_head.params,
           "embedding": fld.embedding_appearance.embedding.weight}
    for k, v in src.items():
        assert field_oracle.params[k].shape == v.shape, (k, field_oracle.params[k].shape, v.shape)
        field_oracle.params[k] = v.detach().cpu().clone().requires_grad_(True)
    # the oracle's own level table must agree with the product's (independent restatements of tcnn's constructor)
    m, mo = fld.mlp_base_grid.meta, field_oracle.meta
    assert list(m.offsets) == list(mo.offsets) and list(m.resolutions) == list(mo.resolutions)
    assert np.allclose(np.float32(m.scales), np.float32(mo.scales), rtol=0, atol=0)


def compare_model_outputs(hip, orc, o, d, appearance_id: Optional[torch.Tensor], check_grads=True,
                          jitter: Optional[torch.Tensor] = None) -> Dict[str, float]:
    """Runs hip.exec_get_outputs on the GPU, re-renders THE SAME packed samples through the oracle, compares renders
    and (optionally) every parameter gradient + ray gradients.  Sampler parity is tested separately (bit-exact)."""
    from lsenerf_amd import RayBundle
    hip.train()
    orc.training = True
    R = o.shape[0]
    og = o.clone().cuda().requires_grad_(True)
    dg = d.clone().cuda().requires_grad_(True)
    meta = {}
    if appearance_id is not None:
        meta["appearance_id"] = appearance_id.cuda()
    rb = RayBundle(origins=og, directions=dg, camera_indices=torch.zeros(R, 1, dtype=torch.long, device="cuda"),
                   metadata=meta)
    if jitter is None:
        jitter = torch.rand(R, generator=torch.Generator().manual_seed(7))
    # sampler on the GPU; the same samples go to the oracle
    rs, li = hip.sampler(ray_bundle=rb, near_plane=hip.config.near_plane, far_plane=hip.config.far_plane,
                         render_step_size=hip.config.render_step_size, alpha_thre=hip.config.alpha_thre,
                         cone_angle=hip.config.cone_angle, jitter=jitter.cuda())
    ts, te = rs.frustums.starts[..., 0].contiguous(), rs.frustums.ends[..., 0].contiguous()
    out = hip.render_packed(rb, rs.ray_indices, ts, te, rs.packed_info)

    oc = o.clone().requires_grad_(True)
    dc = d.clone().requires_grad_(True)
    for p in orc.field.parameters():
        p.grad = None
    ref = orc.render_samples(oc, dc, li.cpu(), ts.cpu(), te.cpu(), appearance_id)
    res = {
        "n_samples": float(ts.shape[0]),
        "rgb": nmax_err(out["rgb"], ref["rgb"], 1e-3),
        "acc": nmax_err(out["accumulation"], ref["accumulation"], 1e-3),
        "depth": nmax_err(out["depth"], ref["depth"], 1e-3),
    }
    assert torch.equal(out["num_samples_per_ray"].cpu(), ref["num_samples_per_ray"])
    assert res["rgb"] < TOL_FWD * 5 and res["acc"] < TOL_FWD * 5 and res["depth"] < TOL_FWD * 5, res
    if check_grads:
        g = torch.Generator().manual_seed(3)
        wr = torch.rand(R, 3, generator=g)
        wa = torch.rand(R, 1, generator=g)
        wd = torch.rand(R, 1, generator=g)
        for p in hip.parameters():
            p.grad = None
        loss = (out["rgb"] * wr.cuda()).sum() + (out["accumulation"] * wa.cuda()).sum() + (out["depth"] * wd.cuda()).sum()
        loss.backward()
        lref = (ref["rgb"] * wr).sum() + (ref["accumulation"] * wa).sum() + (ref["depth"] * wd).sum()
        lref.backward()
        fld = hip.field
        pairs = {"grid": fld.mlp_base_grid.params, "base": fld.mlp_base_mlp.params, "head": fld.mlp_head.params,
                 "embedding": fld.embedding_appearance.embedding.weight}
        emb_w = fld.embedding_appearance.embedding.weight
        bounds = {"grid": hash_level_bounds(fld.mlp_base_grid.meta), "base": mlp_row_bounds(fld.mlp_base_mlp),
                  "head": mlp_row_bounds(fld.mlp_head), "embedding": row_bounds(emb_w.shape[0], emb_w.shape[1])}
        for k, p in pairs.items():
            gref = orc.field.params[k].grad
            assert p.grad is not None and gref is not None, k
            # global-max normalised, relative L2, and per hash level / per MLP row / per embedding row
            res.update(grad_errors(k, p.grad, gref, bounds[k]))
            assert res["d_" + k] < TOL_GRAD and res[f"d_{k}_l2"] < TOL_GRAD and res[f"d_{k}_blk"] < TOL_GRAD_BLOCK, (k, res)
        res["d_origins"] = nmax_err(og.grad, oc.grad, 1e-12)
        res["d_directions"] = nmax_err(dg.grad, dc.grad, 1e-12)
        assert res["d_origins"] < TOL_GRAD and res["d_directions"] < TOL_GRAD, res
    return res


# ----------------------------------------------------------------------------------------------------
# per-ray compositing: float64 reference, float32 lane-exact emulation, trained-scene input generator
# (tests/test_compositing_ref_cpu.py holds these against each other; tests/test_gpu_compositing.py holds the kernels against them)
# ----------------------------------------------------------------------------------------------------
SURFACE_SIGMAS = (30.0, 1e3, 1e4, 1e5, 1e6, float(np.exp(15.0)), 1e10, 3e38, float("inf"))
AUTO_STEP = float(np.float32(2.0 * np.sqrt(3.0) / 1000.0))       # the constant automatic render step


def ray_exclusive_sum(x: torch.Tensor, packed_info: torch.Tensor) -> torch.Tensor:
    """Exclusive prefix sum INSIDE each ray: torch.cumsum over the ray's own samples, shifted by one.  Unlike the global
    cumsum-minus-offset of oracle/volrend.py nothing is subtracted, so an infinite sample stays inside its ray (nerfacc's
    exclusive_sum semantics).  Differentiable.  Rays must be packed gaplessly in order (what every sampler here produces)."""
    parts, pos = [], 0
    for s, c in packed_info.tolist():
        assert s == pos or c == 0, "rays must be packed in order without gaps"
        if c:
            cs = torch.cumsum(x[s:s + c], 0)
            parts.append(torch.cat([x.new_zeros(1), cs[:-1]]))
            pos = s + c
    return torch.cat(parts) if parts else x.new_zeros(0)


def composite_ref(ts, te, sigma, packed_info, rgb=None) -> Dict[str, torch.Tensor]:
    """float64 per-ray reference of the compositing chain (differentiable w.r.t. ``sigma`` and ``rgb``):
    weights / trans / alphas [N], rgb [R,3] (from rgb[:, :3]), acc [R], num [R] = sum w (ts+te)/2,
    depth [R] = clip(num / (acc + 1e-10), global min mid-point, global max mid-point) (clip skipped without samples)."""
    ts, te, sigma = ts.double(), te.double(), sigma.double()
    R = packed_info.shape[0]
    n = int(packed_info[:, 1].sum())
    ts, te, sigma = ts[:n], te[:n], sigma[:n]
    ri = torch.repeat_interleave(torch.arange(R), packed_info[:, 1])
    sd = sigma * (te - ts)
    alphas = 1.0 - torch.exp(-sd)
    trans = torch.exp(-ray_exclusive_sum(sd, packed_info))
    w = trans * alphas
    mid = (ts + te) / 2
    out = {"weights": w, "trans": trans, "alphas": alphas, "ray_indices": ri,
           "acc": torch.zeros(R, dtype=torch.float64).index_add(0, ri, w),
           "num": torch.zeros(R, dtype=torch.float64).index_add(0, ri, w * mid)}
    if rgb is not None:
        out["rgb"] = torch.zeros(R, 3, dtype=torch.float64).index_add(0, ri, w[:, None] * rgb[:n, :3].double())
    raw = out["num"] / (out["acc"] + 1e-10)
    out["depth_raw"] = raw
    if n > 0:
        out["range"] = (float(mid.min()), float(mid.max()))
        raw = torch.clip(raw, mid.min().detach(), mid.max().detach())
    out["depth"] = raw
    return out


def visibility_ref(ref: Dict[str, torch.Tensor], early_stop_eps: float, alpha_thre: float, band: float = 1e-5):
    """(mask, undecided): float64 visibility of ``composite_ref`` output and the samples whose transmittance or alpha lies
    within ``band`` (relative) of its threshold -- the only ones on which a correct float32 kernel may differ."""
    T, a = ref["trans"].detach(), ref["alphas"].detach()
    vis = T >= early_stop_eps
    und = (T / early_stop_eps - 1).abs() < band
    if alpha_thre > 0:
        vis = vis & (a >= alpha_thre)
        und = und | ((a / alpha_thre - 1).abs() < band)
    return vis, und


def emulate_composite_f32(ts, te, sigma, packed_info, shifted: bool = True):
    """float32 emulation of the per-ray walk of volrend_fwd_kernel in numpy, lane for lane: 64-sample chunks, Hillis-Steele
    inclusive scan of sd = sigma * dt, a scalar carry between chunks, exp in float32.  ``shifted``: the exclusive prefix is the
    inclusive one moved up a lane (+ carry); otherwise ``(incl - sd) + carry``, the form that cancels.  Does not model FMA
    contraction or the device's expf.  Returns float32 (weights, trans, alphas)."""
    f = np.float32
    ts, te, sg = (np.asarray(t, dtype=f) for t in (ts, te, sigma))
    n = int(packed_info[:, 1].sum())
    w, T, A = np.zeros(n, f), np.zeros(n, f), np.zeros(n, f)
    with np.errstate(over="ignore", invalid="ignore"):
        for s0, cnt in packed_info.tolist():
            carry = f(0)
            for base in range(0, cnt, 64):
                m = min(64, cnt - base)
                sd = np.zeros(64, f)
                i0 = s0 + base
                sd[:m] = sg[i0:i0 + m] * (te[i0:i0 + m] - ts[i0:i0 + m])
                incl = sd.copy()
                off = 1
                while off < 64:
                    nxt = incl.copy()
                    nxt[off:] = incl[off:] + incl[:-off]
                    incl, off = nxt, off * 2
                if shifted:
                    excl = np.concatenate([np.zeros(1, f), incl[:-1]]) + carry
                else:
                    excl = (incl - sd) + carry
                t = np.exp(-excl).astype(f)
                a = (f(1) - np.exp(-sd)).astype(f)
                w[i0:i0 + m], T[i0:i0 + m], A[i0:i0 + m] = (t * a)[:m], t[:m], a[:m]
                carry = f(carry + incl[63])
    return torch.from_numpy(w), torch.from_numpy(T), torch.from_numpy(A)


FIXED_RAY_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1024, 2000)
SURFACE_OFFSETS = (0, 1, 62, 63, 64, 65, -1)      # -1: the ray's last sample


def trained_scene_rays(surface_sigma: float, seed: int = 0, step: str = "const", onset: str = "abrupt", n_random: int = 40,
                       max_random: int = 400, rgb_stride: int = 3, lengths=None, t0=None) -> Dict[str, torch.Tensor]:
    """Seeded ragged rays as a trained scene produces them (all float32, on the CPU).

    Lengths: ``FIXED_RAY_LENGTHS`` + ``n_random`` random ones in [0, max_random] (or ``lengths``).  Intervals are contiguous
    (te[i] == ts[i+1] bitwise: both are entries of one edge array), either the constant automatic step or growing with t as
    the cone marcher makes them, dt = clamp(0.02 t, 0.003, 0.1).  Density: haze in [0, 0.5) with a quarter of it exactly 0, then
    a surface of ``surface_sigma``: one to three samples (``onset == "ramp"``: sigma/1000, sigma, sigma) at ray offsets
    ``SURFACE_OFFSETS`` in turn, so it sits first in the ray, on both sides of the 64-lane chunk border, and last.  Every
    5th ray has a second surface further back, every 7th none; a ray without surface gets sigma = 3 on its first sample so that
    no ray's peak weight is below 1e-3 -- 1 - expf(-x) carries an absolute error of half an ulp of ONE however small x is, and
    the per-ray metric of the tests divides by the ray's own peak (float32's limit there, not the kernel's).
    dt > 0 everywhere (sigma = inf with dt = 0 is NaN in any arithmetic and is left out).
    Returns ts, te, sigma [N], rgb [N, rgb_stride] in [0, 1], packed_info [R, 2], ray_indices [N], has_surface [R] (bool),
    surface_at [R] (offset at which the ray's first surface begins, -1 without one)."""
    rng = np.random.default_rng(seed)
    if lengths is None:
        lengths = list(FIXED_RAY_LENGTHS) + [int(v) for v in rng.integers(0, max_random + 1, n_random)]
    lengths = [int(v) for v in lengths]
    R, lmax = len(lengths), max(lengths + [1])
    if step == "const":
        master = AUTO_STEP * np.arange(lmax + 512, dtype=np.float64)
    else:
        assert step == "cone", step
        e, tcur = [], 0.1
        for _ in range(lmax + 512):
            e.append(tcur)
            tcur += min(max(0.02 * tcur, 0.003), 0.1)
        master = np.asarray(e) - e[0]
    ts, te, sg, has = [], [], [], np.zeros(R, bool)
    at = np.full(R, -1, np.int64)
    turn = 0              # counts the rays that get a surface: the offsets go round over THEM, whichever rays have none
    for r, c in enumerate(lengths):
        if c == 0:
            continue
        k0 = int(rng.integers(0, 500))
        start = (0.05 + 0.5 * rng.random()) if t0 is None else float(t0[r])
        edges = (start + master[k0:k0 + c + 1] - (master[k0] if step == "const" else 0.0)).astype(np.float32)
        s = (rng.random(c) * 0.5 * (rng.random(c) >= 0.25)).astype(np.float32)
        if r % 7 == 6:
            s[0] = 3.0
        else:
            has[r] = True
            offs = [SURFACE_OFFSETS[turn % len(SURFACE_OFFSETS)]]
            turn += 1
            if r % 5 == 4:
                offs.append(int(rng.integers(0, c)))
            for j, o in enumerate(offs):
                prof = [surface_sigma / 1000.0, surface_sigma, surface_sigma] if onset == "ramp" \
                    else [surface_sigma] * int(rng.integers(1, 4))
                prof = prof[-c:]                  # a ray shorter than the surface keeps the surface's dense end
                if o < 0:
                    o = c - len(prof)             # "last": the surface ends with the ray
                elif j == 0 and c > 66 and o >= 62:
                    prof = prof[:min(len(prof), c - o)]      # at the chunk border the onset stays where it was asked for
                o = min(o % c, c - len(prof))
                s[o:o + len(prof)] = np.asarray(prof, dtype=np.float32)
                if j == 0:
                    at[r] = o
        ts.append(edges[:-1]); te.append(edges[1:]); sg.append(s)
    cat = lambda parts: torch.from_numpy(np.concatenate(parts) if parts else np.zeros(0, np.float32))   # noqa: E731
    cnt = torch.tensor(lengths, dtype=torch.int64)
    n = int(cnt.sum())
    rgb = torch.from_numpy(rng.random((n, rgb_stride)).astype(np.float32))
    return {"ts": cat(ts), "te": cat(te), "sigma": cat(sg), "rgb": rgb,
            "packed_info": torch.stack([torch.cumsum(cnt, 0) - cnt, cnt], -1).contiguous(),
            "ray_indices": torch.repeat_interleave(torch.arange(R), cnt), "has_surface": torch.from_numpy(has),
            "surface_at": torch.from_numpy(at)}


def select_rays(inp: Dict[str, torch.Tensor], keep: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The same inputs with only the rays ``keep`` [R] (bool) marks, re-packed (ray isolation checks)."""
    ks = keep[inp["ray_indices"]]
    cnt = inp["packed_info"][:, 1][keep]
    out = {k: inp[k][ks].contiguous() for k in ("ts", "te", "sigma", "rgb")}
    out["packed_info"] = torch.stack([torch.cumsum(cnt, 0) - cnt, cnt], -1).contiguous()
    out["ray_indices"] = torch.repeat_interleave(torch.arange(cnt.shape[0]), cnt)
    out["has_surface"] = inp["has_surface"][keep]
    out["surface_at"] = inp["surface_at"][keep]
    return out


def ray_bounds(packed_info: torch.Tensor, width: int = 1):
    """Block boundaries of the rays of a packed per-sample array with ``width`` values per sample (blockwise_nmax_err)."""
    s = packed_info[:, 0].tolist()
    return [int(v) * width for v in s] + [int(packed_info[-1, 0] + packed_info[-1, 1]) * width]


def emulate_composite_bwd_f32(ts, te, packed_info, weights, g_rgb=None, g_acc=None, g_dep=None, rgb=None, g_w=None, t_end_shift=0.0):
    """float32 emulation of volrend_bwd_kernel's recurrence, lane for lane (numpy; no FMA contraction):
    wtot by per-lane partial sums + butterfly, t_end = 1 - wtot, then the chunks in reverse with Hillis-Steele suffix scans of
    w and dw * w,  d_sigma = (dw (t_end + sum_{i>k} w_i) - sum_{i>k} dw_i w_i) dt.  ``weights``: the forward's float32 weights;
    g_rgb [R,3] / g_acc [R] / g_dep [R] (gradient of the depth NUMERATOR) / g_w [N], each optional.  ``t_end_shift`` is added to
    t_end (see ``emulate_render_grad_f32``).  Returns d_sigma (float32)."""
    f = np.float32
    ts, te, w_all = (np.asarray(t, dtype=f) for t in (ts, te, weights))
    R = packed_info.shape[0]
    zero = np.zeros(R, f)
    ga = zero if g_acc is None else np.asarray(g_acc, dtype=f)
    gd = zero if g_dep is None else np.asarray(g_dep, dtype=f)
    gc = None if g_rgb is None or rgb is None else np.asarray(g_rgb, dtype=f)
    c_all = None if gc is None else np.asarray(rgb, dtype=f)
    gw_all = None if g_w is None else np.asarray(g_w, dtype=f)
    out = np.zeros(w_all.shape[0], f)
    lanes = np.arange(64)

    def suffix_scan(v):
        off = 1
        while off < 64:
            nxt = v.copy()
            nxt[:-off] = v[:-off] + v[off:]
            v, off = nxt, off * 2
        return v

    for r, (s0, cnt) in enumerate(packed_info.tolist()):
        if cnt == 0:
            continue
        part = np.zeros(64, f)
        for base in range(0, cnt, 64):
            m = min(64, cnt - base)
            part[:m] = part[:m] + w_all[s0 + base:s0 + base + m]
        for off in (32, 16, 8, 4, 2, 1):
            part = part + part[lanes ^ off]
        t_end = f(f(1) - part[0]) + f(t_end_shift)
        carry_w = carry_g = f(0)
        for base in range(((cnt - 1) // 64) * 64, -1, -64):
            m = min(64, cnt - base)
            i0 = s0 + base
            w, dw, dt = np.zeros(64, f), np.zeros(64, f), np.zeros(64, f)
            a, b = ts[i0:i0 + m], te[i0:i0 + m]
            w[:m], dt[:m] = w_all[i0:i0 + m], b - a
            d = ga[r] + gd[r] * ((a + b) * f(0.5))
            if gw_all is not None:
                d = d + gw_all[i0:i0 + m]
            if gc is not None:
                c = c_all[i0:i0 + m]
                d = d + ((gc[r, 0] * c[:, 0] + gc[r, 1] * c[:, 1]) + gc[r, 2] * c[:, 2])
            dw[:m] = d
            gw = dw * w
            incl_w, incl_g = suffix_scan(w), suffix_scan(gw)
            sw, sg = (incl_w - w) + carry_w, (incl_g - gw) + carry_g
            out[i0:i0 + m] = ((dw * (t_end + sw) - sg) * dt)[:m]
            carry_w, carry_g = f(carry_w + incl_w[0]), f(carry_g + incl_g[0])
    return torch.from_numpy(out)


def emulate_depth_chain_f32(ts, te, packed_info, weights, g_depth, g_acc=None):
    """float32 restatement of the O(R) chain rule of ops._VolRendFn.backward through depth = clip(num / (acc + 1e-10), lo, hi):
    (g_acc, g_dep) to hand to ``emulate_composite_bwd_f32`` for an upstream gradient ``g_depth`` on the clipped depth."""
    ts, te, w = ts.float(), te.float(), weights.float()
    R = packed_info.shape[0]
    ri = torch.repeat_interleave(torch.arange(R), packed_info[:, 1])
    mid = (ts + te) * 0.5
    acc = torch.zeros(R).index_add(0, ri, w)
    num = torch.zeros(R).index_add(0, ri, w * mid)
    den = acc + 1e-10
    raw = num / den
    g = torch.where((raw >= mid.min()) & (raw <= mid.max()), g_depth.float(), torch.zeros(R))
    extra = -g * raw / den
    return (extra if g_acc is None else g_acc.float() + extra), g / den


def emulate_render_grad_f32(inp: Dict[str, torch.Tensor], depth_epilogue: bool, g_rgb=None, g_acc=None, g_depth=None, t_end_shift=0.0):
    """d_sigma as a float32 implementation of the product's recurrences gives it (forward by shifted scan, backward as
    volrend_bwd_kernel) for upstream gradients on rgb [R,3], accumulation [R] and depth [R] (the clipped expected depth with
    ``depth_epilogue``, else the depth numerator), each optional.  ``t_end_shift``: on an opaque ray the float32 sum of the
    weights is 1 to within an ulp, so t_end = 1 - sum w is 0 or +-2^-24 depending on the last bit of every expf -- numpy's exp and
    the device's differ there.  A bound derived from this emulation takes the worst of shift 0, +2^-24 and -2^-24."""
    w = emulate_composite_f32(inp["ts"], inp["te"], inp["sigma"], inp["packed_info"])[0]
    g_dep = g_depth
    if depth_epilogue and g_depth is not None:
        g_acc, g_dep = emulate_depth_chain_f32(inp["ts"], inp["te"], inp["packed_info"], w, g_depth, g_acc)
    return emulate_composite_bwd_f32(inp["ts"], inp["te"], inp["packed_info"], w, g_rgb, g_acc, g_dep, inp["rgb"], t_end_shift=t_end_shift)


def emulated_per_ray_grad_error(inp, depth_epilogue, ref_d_sigma, g_rgb=None, g_acc=None, g_depth=None) -> float:
    """Worst per-ray error of ``emulate_render_grad_f32`` against ``ref_d_sigma`` over t_end shifts of 0 and +-2^-24."""
    bounds = ray_bounds(inp["packed_info"])
    return max(blockwise_nmax_err(emulate_render_grad_f32(inp, depth_epilogue, g_rgb, g_acc, g_depth, sh), ref_d_sigma, bounds)
               for sh in (0.0, 2.0 ** -24, -(2.0 ** -24)))
