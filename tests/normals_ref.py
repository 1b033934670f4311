"""float64 twin of the analytic-normals chain (tests/test_normals_cpu.py and the GPU tests of the normals kernels).  Not a test file.

Three parts, everything on the CPU in float64:
* the field: tcnn grid interpolation (``oracle.hashgrid.hash_encode_tcnn`` evaluated in float64) -> base network 32 -> 64 -> 16,
  with torch autograd for ``g = d h[0] / d x01``;
* the compositing formulas in numpy: n = -g / max(|g|, 1e-12) per sample, N = sum w n per ray over the render weights,
  N / (|N| + 1e-10); the world-space variant takes g through the transposed Jacobian of the position map first (autograd through a
  float64 restatement of the map, selector-masked as ``lse_positions_bwd`` masks it);
* the ReLU-gate band: the samples on which a float32 and a float64 gate may disagree.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from oracle import hashgrid as ohg

BAND = 1e-5          # |pre-activation| below which a float32 and a float64 ReLU gate may disagree (tests/test_gpu_mlp_bwd_input.py)


# ---------------------------------------------------------------------------------------------------- field
def base_weights(seed: int = 11) -> torch.Tensor:
    """tcnn-layout parameters of the 32 -> 64 -> 16 base network: W0 [64, 32] then Wo [16, 64], float32 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    u = lambda m, fan: (torch.rand(m, generator=g) * 2 - 1) * (6.0 / fan) ** 0.5
    return torch.cat([u(64 * 32, 96), u(16 * 64, 80)])


def base_net64(y_rows: torch.Tensor, params: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(output [n, 16], layer-0 pre-activation [n, 64]) of the base network in float64 from row-major inputs [n, 32]."""
    w = params.double()
    pre0 = y_rows.double() @ w[:2048].view(64, 32).T
    return torch.relu(pre0) @ w[2048:3072].view(16, 64).T, pre0


def gate_band(pre0: torch.Tensor, band: float = BAND) -> torch.Tensor:
    """[n] bool: samples with a hidden pre-activation inside ``band`` of zero."""
    return pre0.abs().amin(1) < band


def logit_grad_of_features64(y_rows: torch.Tensor, params: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(d out[:, 0] / d y [n, 32], gate-band mask [n]) by autograd in float64."""
    y = y_rows.detach().double().requires_grad_(True)
    out, pre0 = base_net64(y, params)
    out[:, 0].sum().backward()
    return y.grad, gate_band(pre0.detach())


def field_logit64(x01: torch.Tensor, table: torch.Tensor, meta_o: ohg.TcnnGridMeta, params: torch.Tensor):
    """(h0 [n], pre0 [n, 64]) of the density logit at float64 positions ``x01`` [n, 3] (differentiable w.r.t. ``x01``)."""
    y = ohg.hash_encode_tcnn(x01, table.double(), meta_o)
    out, pre0 = base_net64(y, params)
    return out[:, 0], pre0


def field_logit_grad64(x01: torch.Tensor, table: torch.Tensor, meta_o: ohg.TcnnGridMeta, params: torch.Tensor):
    """(g = d h0 / d x01 [n, 3], h0 [n], pre0 [n, 64]) by autograd through the interpolation and the network, float64."""
    x = x01.detach().double().requires_grad_(True)
    h0, pre0 = field_logit64(x, table, meta_o, params)
    h0.sum().backward()
    return x.grad, h0.detach(), pre0.detach()


# ---------------------------------------------------------------------------------------------------- position map
def unit_cube64(p: torch.Tensor, contraction: bool, aabb6) -> Tuple[torch.Tensor, torch.Tensor]:
    """(x01 [n, 3], selector [n]) of world positions in float64: L-inf contraction -> (c + 2) / 4, or aabb normalisation."""
    if contraction:
        mag = p.abs().amax(-1, keepdim=True)
        safe = mag.clamp_min(1.0)
        c = torch.where(mag < 1.0, p, (2.0 - 1.0 / safe) * (p / safe))
        x = (c + 2.0) / 4.0
    else:
        lo, hi = torch.tensor(aabb6[:3], dtype=torch.float64), torch.tensor(aabb6[3:], dtype=torch.float64)
        x = (p - lo) / (hi - lo)
    return x, ((x > 0) & (x < 1)).all(-1)


def world_gradient64(p: np.ndarray, g: np.ndarray, contraction: bool, aabb6) -> np.ndarray:
    """J^T g per sample: the gradient with respect to the world position of a function whose gradient with respect to x01 is ``g``,
    zero where the selector is false."""
    with torch.enable_grad():
        pt = torch.from_numpy(np.asarray(p, dtype=np.float64)).requires_grad_(True)
        x, sel = unit_cube64(pt, contraction, aabb6)
        (x * torch.from_numpy(np.asarray(g, dtype=np.float64))).sum().backward()
    return (pt.grad * sel[:, None]).numpy()


# ---------------------------------------------------------------------------------------------------- compositing
def sample_normals(g: np.ndarray) -> np.ndarray:
    """n = -g / max(|g|, 1e-12) (F.normalize): a zero gradient gives a zero normal."""
    g = np.asarray(g, dtype=np.float64)
    return -g / np.maximum(np.linalg.norm(g, axis=-1, keepdims=True), 1e-12)


def render_weights(ts: np.ndarray, te: np.ndarray, sigma: np.ndarray) -> np.ndarray:
    """w_i = exp(-sum_{k<i} sigma_k dt_k) (1 - exp(-sigma_i dt_i)) of ONE ray."""
    sd = np.asarray(sigma, dtype=np.float64) * (np.asarray(te, dtype=np.float64) - np.asarray(ts, dtype=np.float64))
    excl = np.concatenate([[0.0], np.cumsum(sd)[:-1]]) if sd.size else sd
    return np.exp(-excl) * (1.0 - np.exp(-sd))


def composite_normals(ts, te, sigma, d_x01, packed_info, world: bool = False, rays_o=None, rays_d=None, contraction: bool = True,
                      aabb6=None, renormalize: bool = True) -> np.ndarray:
    """Rendered normals [R, 3] in float64.  Sample arrays may be longer than the samples ``packed_info`` [R, 2] names."""
    f = lambda t: None if t is None else np.asarray(t.detach().cpu() if torch.is_tensor(t) else t, dtype=np.float64)
    ts, te, sigma, g, rays_o, rays_d = f(ts), f(te), f(sigma), f(d_x01), f(rays_o), f(rays_d)
    pk = np.asarray(packed_info.cpu() if torch.is_tensor(packed_info) else packed_info, dtype=np.int64)
    out = np.zeros((pk.shape[0], 3), dtype=np.float64)
    for r, (s, c) in enumerate(pk.tolist()):
        if c == 0:
            continue
        sl = slice(s, s + c)
        gr = g[sl]
        if world:
            pos = rays_o[r][None, :] + rays_d[r][None, :] * ((ts[sl] + te[sl]) / 2.0)[:, None]
            gr = world_gradient64(pos, gr, contraction, aabb6)
        N = (render_weights(ts[sl], te[sl], sigma[sl])[:, None] * sample_normals(gr)).sum(0)
        out[r] = N / (np.linalg.norm(N) + 1e-10) if renormalize else N
    return out
