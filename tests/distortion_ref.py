"""Twins of the distortion-loss kernels (lse_distortion_fwd / lse_distortion_bwd, include/lse_hip.h) for the tests:

  * ``loss64`` / ``reference``: float64, the O(n^2) double sum per ray with |m_i - m_j| (no sortedness assumed) plus the interval
    term, differentiable by torch autograd -- with ``reference`` down to sigma, through the float64 weights of ``composite_ref``;
  * ``emulate_fwd_f32`` / ``emulate_dw_f32`` / ``emulate_dsigma_f32`` / ``emulate_f32``: float32 numpy restatements of the kernels'
    formulation -- 64-sample groups, Hillis-Steele scans, scalar carries, mid-points relative to the ray's first, T_end from the
    densities.  ``emulate_f32`` also sends the d_weights through ``tests.util.emulate_composite_bwd_f32(g_w=...)``, the recurrence
    of volrend_bwd_kernel with its T_end = 1 - sum w.  ``shifted=False`` is the formulation the contract rules out: absolute
    mid-points, which cancel at the size of t;
  * ``case`` / ``scaled``: the seeded inputs of one (surface sigma, step kind) and their float64 reference, computed once per
    process and shared by tests/test_distortion_cpu.py and tests/test_gpu_distortion.py.
"""
from __future__ import annotations

import functools
from typing import Dict, Optional

import numpy as np
import torch

from tests.util import SURFACE_SIGMAS, composite_ref, emulate_composite_bwd_f32, emulate_composite_f32, trained_scene_rays

F = np.float32


def loss64(w: torch.Tensor, ts, te, packed_info, t_scale: float = 1.0) -> torch.Tensor:
    """[R] float64: sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 delta_i per ray, differentiable with respect to ``w`` (float64)."""
    ts, te = ts.double() * t_scale, te.double() * t_scale
    m, delta = (ts + te) / 2, te - ts
    out = []
    for s, c in packed_info.tolist():
        wr, mr = w[s:s + c], m[s:s + c]
        pair = (wr[:, None] * wr[None, :] * (mr[:, None] - mr[None, :]).abs()).sum()
        out.append(pair + (wr * wr * delta[s:s + c]).sum() / 3.0)
    return torch.stack(out) if out else w.new_zeros(0)


def reference(inp: Dict[str, torch.Tensor], t_scale: float = 1.0, g: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """float64 loss [R] of the rays ``inp`` (tests.util.trained_scene_rays) and, for the upstream gradient ``g`` ([R] or a scalar;
    default 1), d_weights [N] (the weights held fixed as a leaf) and d_sigma [N] (through the weights of ``composite_ref``)."""
    ts, te, packed = inp["ts"], inp["te"], inp["packed_info"]
    R = packed.shape[0]
    g = torch.ones(R, dtype=torch.float64) if g is None else torch.as_tensor(g, dtype=torch.float64).expand(R)
    sigma = inp["sigma"].double().requires_grad_(True)
    w = composite_ref(ts, te, sigma, packed)["weights"]
    loss = loss64(w, ts, te, packed, t_scale)
    d_sigma, = torch.autograd.grad((loss * g).sum(), sigma)
    wl = w.detach().clone().requires_grad_(True)
    d_w, = torch.autograd.grad((loss64(wl, ts, te, packed, t_scale) * g).sum(), wl)
    return {"loss": loss.detach(), "weights": w.detach(), "d_weights": d_w, "d_sigma": d_sigma}


def _prefix_scan(v):
    off = 1
    while off < 64:
        nxt = v.copy()
        nxt[off:] = v[off:] + v[:-off]
        v, off = nxt, off * 2
    return v


def _suffix_scan(v):
    off = 1
    while off < 64:
        nxt = v.copy()
        nxt[:-off] = v[:-off] + v[off:]
        v, off = nxt, off * 2
    return v


def _group(ts, te, w_all, i0, m, a0, b0, t_scale, shifted):
    """(w, mid, delta) of one 64-sample group, padded as the kernels pad an invalid lane (the first interval, zero weight)."""
    a, b, w = np.full(64, a0, F), np.full(64, b0, F), np.zeros(64, F)
    a[:m], b[:m], w[:m] = ts[i0:i0 + m], te[i0:i0 + m], w_all[i0:i0 + m]
    mid = t_scale * (((a - a0) + (b - b0)) * F(0.5)) if shifted else (t_scale * a + t_scale * b) * F(0.5)
    return w, mid.astype(F), (t_scale * (b - a)).astype(F)


def emulate_fwd_f32(ts, te, weights, packed_info, t_scale: float = 1.0, shifted: bool = True):
    """(loss [R], totals [R,2]) as distortion_fwd_kernel forms them, float32, lane for lane (no FMA contraction)."""
    ts, te, w_all = (np.asarray(t, dtype=F) for t in (ts, te, weights))
    t_scale = F(t_scale)
    R = packed_info.shape[0]
    loss, totals = np.zeros(R, F), np.zeros((R, 2), F)
    lanes = np.arange(64)
    for r, (s0, cnt) in enumerate(packed_info.tolist()):
        if cnt == 0:
            continue
        a0, b0 = ts[s0], te[s0]
        carry_w = carry_m = F(0)
        acc = np.zeros(64, F)
        for base in range(0, cnt, 64):
            w, mid, delta = _group(ts, te, w_all, s0 + base, min(64, cnt - base), a0, b0, t_scale, shifted)
            wm = w * mid
            incl_w, incl_m = _prefix_scan(w), _prefix_scan(wm)
            w_lt = np.concatenate([np.zeros(1, F), incl_w[:-1]]) + carry_w
            m_lt = np.concatenate([np.zeros(1, F), incl_m[:-1]]) + carry_m
            acc = acc + ((F(2) * w) * (mid * w_lt - m_lt) + (w * w) * delta * F(1.0 / 3.0))
            carry_w, carry_m = F(carry_w + incl_w[63]), F(carry_m + incl_m[63])
        for off in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[lanes ^ off]
        loss[r], totals[r] = acc[0], (carry_w, carry_m)
    return torch.from_numpy(loss), torch.from_numpy(totals)


def emulate_dw_f32(ts, te, weights, packed_info, totals, g, t_scale: float = 1.0, shifted: bool = True) -> torch.Tensor:
    """d_weights [N] as distortion_bwd_kernel forms it: the reverse walk with suffix scans and the forward's totals.
    ``g``: [R] or a scalar."""
    ts, te, w_all = (np.asarray(t, dtype=F) for t in (ts, te, weights))
    t_scale = F(t_scale)
    R = packed_info.shape[0]
    g = np.broadcast_to(np.asarray(g, dtype=F), (R,))
    tot = np.asarray(totals, dtype=F)
    out = np.zeros(w_all.shape[0], F)
    for r, (s0, cnt) in enumerate(packed_info.tolist()):
        if cnt == 0:
            continue
        a0, b0 = ts[s0], te[s0]
        w_tot, m_tot = tot[r]
        carry_w = carry_m = F(0)
        for base in range(((cnt - 1) // 64) * 64, -1, -64):
            m = min(64, cnt - base)
            w, mid, delta = _group(ts, te, w_all, s0 + base, m, a0, b0, t_scale, shifted)
            wm = w * mid
            incl_w, incl_m = _suffix_scan(w), _suffix_scan(wm)
            w_gt = np.concatenate([incl_w[1:], np.zeros(1, F)]) + carry_w
            m_gt = np.concatenate([incl_m[1:], np.zeros(1, F)]) + carry_m
            w_lt, m_lt = (w_tot - w_gt) - w, (m_tot - m_gt) - wm
            dw = g[r] * (F(2) * (mid * (w_lt - w_gt) - (m_lt - m_gt)) + F(2.0 / 3.0) * w * delta)
            out[s0 + base:s0 + base + m] = dw[:m]
            carry_w, carry_m = F(carry_w + incl_w[0]), F(carry_m + incl_m[0])
    return torch.from_numpy(out)


def emulate_dsigma_f32(ts, te, sigma, weights, packed_info, d_w) -> torch.Tensor:
    """d_sigma [N] as distortion_bwd_kernel forms it from its own d_weights: T_end = exp(-sum sigma dt) from a pass over the
    densities (per-lane partial sums + butterfly), then the reverse walk  d_sigma_k = dt_k (dw_k (T_end + W_>k) - sum_{i>k} dw_i w_i)
    with shifted suffix scans.  ``sigma=None``: T_end = 1 - W_tot, the form that is left with an absolute error of 2^-24."""
    ts, te, w_all, dw_all = (np.asarray(t, dtype=F) for t in (ts, te, weights, d_w))
    sg_all = None if sigma is None else np.asarray(sigma, dtype=F)
    out = np.zeros(w_all.shape[0], F)
    lanes = np.arange(64)
    for s0, cnt in packed_info.tolist():
        if cnt == 0:
            continue
        part = np.zeros(64, F)
        for base in range(0, cnt, 64):
            m, i0 = min(64, cnt - base), s0 + base
            part[:m] = part[:m] + (w_all[i0:i0 + m] if sg_all is None else sg_all[i0:i0 + m] * (te[i0:i0 + m] - ts[i0:i0 + m]))
        for off in (32, 16, 8, 4, 2, 1):
            part = part + part[lanes ^ off]
        t_end = F(F(1) - part[0]) if sg_all is None else np.exp(-part[0]).astype(F)
        carry_w = carry_g = F(0)
        for base in range(((cnt - 1) // 64) * 64, -1, -64):
            m, i0 = min(64, cnt - base), s0 + base
            w, dw, dt = np.zeros(64, F), np.zeros(64, F), np.zeros(64, F)
            w[:m], dw[:m], dt[:m] = w_all[i0:i0 + m], dw_all[i0:i0 + m], te[i0:i0 + m] - ts[i0:i0 + m]
            gw = dw * w
            incl_w, incl_g = _suffix_scan(w), _suffix_scan(gw)
            w_gt = np.concatenate([incl_w[1:], np.zeros(1, F)]) + carry_w
            sg = np.concatenate([incl_g[1:], np.zeros(1, F)]) + carry_g
            out[i0:i0 + m] = ((dw * (t_end + w_gt) - sg) * dt)[:m]
            carry_w, carry_g = F(carry_w + incl_w[0]), F(carry_g + incl_g[0])
    return torch.from_numpy(out)


def emulate_f32(inp: Dict[str, torch.Tensor], t_scale: float = 1.0, g=1.0, shifted: bool = True, exact_t_end: bool = True):
    """The whole float32 chain on the rays ``inp``: weights by ``emulate_composite_f32``, loss and totals, d_weights, d_sigma by
    ``emulate_dsigma_f32`` -- and "d_sigma_1mw", the same d_weights through ``tests.util.emulate_composite_bwd_f32(g_w=...)``, the
    recurrence of volrend_bwd_kernel with its T_end = 1 - sum w."""
    ts, te, packed = inp["ts"], inp["te"], inp["packed_info"]
    with np.errstate(over="ignore", invalid="ignore"):
        w = emulate_composite_f32(ts, te, inp["sigma"], packed)[0]
        loss, totals = emulate_fwd_f32(ts, te, w, packed, t_scale, shifted)
        d_w = emulate_dw_f32(ts, te, w, packed, totals, g, t_scale, shifted)
        d_sigma = emulate_dsigma_f32(ts, te, inp["sigma"] if exact_t_end else None, w, packed, d_w)
        d_sigma_1mw = emulate_composite_bwd_f32(ts, te, packed, w, g_w=d_w)
    return {"loss": loss, "totals": totals, "weights": w, "d_weights": d_w, "d_sigma": d_sigma, "d_sigma_1mw": d_sigma_1mw}


# ----------------------------------------------------------------------------------------------------
# the cases both test files run: every finite-gradient surface density, both step kinds, every (g_stride, t_scale)
# ----------------------------------------------------------------------------------------------------
SIGMAS = tuple(s for s in SURFACE_SIGMAS if s <= 1e10)
STEPS = ("const", "cone")
COMBOS = ((1, 1.0), (0, 1.0), (1, 0.25), (0, 0.25))       # (g_stride, t_scale)
G_SCALAR = 0.75


@functools.lru_cache(maxsize=None)
def case(sigma: float, step: str):
    """(inputs, float64 reference at g = 1 and t_scale = 1, per-ray upstream gradient in [0.5, 1.5]) -- the default
    ``trained_scene_rays`` lengths (rays of 0, 1 and 2 samples, 63 / 64 / 65, two- and many-group rays), ramp onset.  Cached:
    nothing returned here is written to."""
    inp = trained_scene_rays(sigma, seed=0, step=step, onset="ramp")
    R = inp["packed_info"].shape[0]
    g = torch.from_numpy(np.random.default_rng(5).random(R).astype(F) + F(0.5))
    return inp, reference(inp), g


def scaled(ref: Dict[str, torch.Tensor], inp, g, t_scale: float) -> Dict[str, torch.Tensor]:
    """The reference for the upstream gradient ``g`` ([R] or a float) and ``t_scale`` from the one at g = 1, t_scale = 1: the loss
    is linear in t_scale, the gradients in t_scale and in the ray's g."""
    gs = torch.as_tensor(g, dtype=torch.float64).expand(inp["packed_info"].shape[0])[inp["ray_indices"]]
    return {"loss": ref["loss"] * t_scale, "d_weights": ref["d_weights"] * gs * t_scale, "d_sigma": ref["d_sigma"] * gs * t_scale}
