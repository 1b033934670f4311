"""Twins of the quantile-depth kernels (include/lse_hip.h: lse_eval_depth_quantiles), in numpy.

* ``reference`` -- float64: per ray tau = cumsum(sigma * dt) over the ray's own samples, then the definition.  Also ``undecided [R]``:
  a sample boundary's tau lies within relative ``band`` of a ``tau_q`` -- the only rays on which a correct float32 walk may pick
  another sample (the band ``tests/util.visibility_ref`` uses for the same scan).
* ``emulate_f32`` -- the kernel's walk lane for lane in float32, extending ``tests/util.emulate_composite_f32``: 64-sample groups,
  the Hillis-Steele scan of ``group_weights`` (first step fused, as the kernel writes it), a scalar carry, the first crossing per
  group, the interpolation operation by operation.
* ``depth_select`` -- ``depth_sel`` from (depth_q, reached), and ``interp_bound`` -- the error bound of the interpolated depth.
"""
from __future__ import annotations

from typing import Dict

import numpy as np

from tests.util import TOL_FWD

F = np.float32


def taus_of(qs) -> np.ndarray:
    """float32(-ln(1 - q)) per q, the logarithm in double (what ``ops.depth_tau`` returns)."""
    return np.asarray([np.float32(-np.log1p(-np.float64(q))) for q in qs], dtype=F)


def _arrays(ts, te, sigma, packed_info):
    ts, te, sg = (np.asarray(t, dtype=F) for t in (ts, te, sigma))
    return ts, te, sg, [(int(s), int(c)) for s, c in np.asarray(packed_info).tolist()]


def reference(ts, te, sigma, packed_info, tau_q, interpolate: bool = False, band: float = 1e-5) -> Dict[str, np.ndarray]:
    """float64 reference.  Returns depth [R, n_q] (float64; the mid-points are the definition's float32 ``(a + b) * 0.5f``), index
    [R, n_q] (the sample the depth comes from, within the ray; the last sample where the quantile is not reached, -1 on an empty ray),
    reached [R] (uint8 bit mask), undecided [R] (bool), a / b / sigma_at [R, n_q] (the crossing sample's interval and density)."""
    ts, te, sg, rays = _arrays(ts, te, sigma, packed_info)
    tq = np.asarray(tau_q, dtype=np.float64)
    R, nq = len(rays), len(tq)
    out = {"depth": np.zeros((R, nq)), "index": np.full((R, nq), -1, np.int64), "reached": np.zeros(R, np.uint8),
           "undecided": np.zeros(R, bool), "a": np.zeros((R, nq)), "b": np.zeros((R, nq)), "sigma_at": np.zeros((R, nq))}
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for r, (s0, c) in enumerate(rays):
            if c == 0:
                continue
            a, b, s = ts[s0:s0 + c].astype(np.float64), te[s0:s0 + c].astype(np.float64), sg[s0:s0 + c].astype(np.float64)
            mid = ((ts[s0:s0 + c] + te[s0:s0 + c]) * F(0.5)).astype(np.float64)
            behind = np.cumsum(s * (b - a))
            front = np.concatenate([[0.0], behind[:-1]])
            for j, t in enumerate(tq):
                hit = np.flatnonzero(behind >= t)          # a NaN never compares true, +inf does
                k = int(hit[0]) if hit.size else c - 1
                d = mid[k]
                if hit.size:
                    out["reached"][r] |= 1 << j
                    if interpolate:
                        x = (t - front[k]) / s[k]
                        if x == x:
                            d = min(max(a[k] + x, a[k]), b[k])
                out["depth"][r, j], out["index"][r, j] = d, k
                out["a"][r, j], out["b"][r, j], out["sigma_at"][r, j] = a[k], b[k], s[k]
                out["undecided"][r] |= bool(np.any(np.abs(behind / t - 1.0) < band))
    return out


def emulate_f32(ts, te, sigma, packed_info, tau_q, interpolate: bool = False) -> Dict[str, np.ndarray]:
    """float32 lane-for-lane emulation of the kernel's walk.  The fused first scan step fmaf(sigma, dt, neighbour) is formed in
    double and rounded once (the product of two floats is exact there).  Returns depth [R, n_q] (float32), index [R, n_q], reached
    [R] (uint8), carry [R] (the carry behind the last group walked; the kernel stops walking once every quantile is found)."""
    ts, te, sg, rays = _arrays(ts, te, sigma, packed_info)
    tq = np.asarray(tau_q, dtype=F)
    R, nq = len(rays), len(tq)
    depth, index = np.zeros((R, nq), F), np.full((R, nq), -1, np.int64)
    reached, carries = np.zeros(R, np.uint8), np.zeros(R, F)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for r, (s0, c) in enumerate(rays):
            carry, found = F(0), 0
            for base in range(0, c, 64):
                m = min(64, c - base)
                i0 = s0 + base
                a, b, s = np.zeros(64, F), np.zeros(64, F), np.zeros(64, F)
                a[:m], b[:m], s[:m] = ts[i0:i0 + m], te[i0:i0 + m], sg[i0:i0 + m]
                dt = b - a
                incl = s * dt
                nxt = incl.copy()
                nxt[1:] = (s[1:].astype(np.float64) * dt[1:].astype(np.float64) + incl[:-1].astype(np.float64)).astype(F)
                incl, off = nxt, 2
                while off < 64:
                    nxt = incl.copy()
                    nxt[off:] = incl[off:] + incl[:-off]
                    incl, off = nxt, off * 2
                front = np.concatenate([np.zeros(1, F), incl[:-1]]) + carry
                behind = incl + carry
                mid = (a + b) * F(0.5)
                for j in range(nq):
                    if (found >> j) & 1:
                        continue
                    hit = np.flatnonzero(behind[:m] >= tq[j])
                    if hit.size == 0:
                        continue
                    k = int(hit[0])
                    d = mid[k]
                    if interpolate:
                        x = F(tq[j] - front[k]) / s[k]
                        if x == x:
                            d = min(max(F(a[k] + x), a[k]), b[k])
                    depth[r, j], index[r, j] = d, base + k
                    found |= 1 << j
                carry = F(carry + incl[63])
                if found == (1 << nq) - 1:
                    break
            if c > 0:
                last = (ts[s0 + c - 1] + te[s0 + c - 1]) * F(0.5)
                for j in range(nq):
                    if not (found >> j) & 1:
                        depth[r, j], index[r, j] = last, c - 1
            reached[r], carries[r] = found, carry
    return {"depth": depth, "index": index, "reached": reached, "carry": carries}


def depth_select(depth_q: np.ndarray, reached: np.ndarray, sel: int, max_spread=None) -> np.ndarray:
    """``depth_sel`` of the definition, float32 [R]: column ``sel`` where its bit is set and -- with a finite ``max_spread`` -- the
    last bit is set and the last column lies at most ``max_spread`` (as float32) behind the first; NaN elsewhere."""
    dq = np.asarray(depth_q, dtype=F)
    nq = dq.shape[1]
    ok = (np.asarray(reached) >> sel) & 1 == 1
    if max_spread is not None and np.isfinite(max_spread):
        ok = ok & ((np.asarray(reached) >> (nq - 1)) & 1 == 1) & ((dq[:, nq - 1] - dq[:, 0]) <= F(max_spread))
    return np.where(ok, dq[:, sel], F(np.nan)).astype(F)


def interp_bound(ref: Dict[str, np.ndarray], tau_q) -> np.ndarray:
    """[R, n_q]: min(b - a, TOL_FWD * tau_q / sigma) + 2 ulp(b) at the reference's crossing sample.  The scan is good to TOL_FWD
    relative; tau_front <= tau_q, so its absolute error is at most TOL_FWD * tau_q, and the division by sigma turns it into depth;
    the clamp keeps any result inside the sample; the quotient, the sum and the rounding of a + x cost the two ulps."""
    tq = np.asarray(tau_q, dtype=np.float64)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        scan = TOL_FWD * tq / ref["sigma_at"]
    scan = np.where(np.isnan(scan), np.inf, scan)
    return np.minimum(ref["b"] - ref["a"], scan) + 2.0 * np.spacing(ref["b"].astype(F)).astype(np.float64)
