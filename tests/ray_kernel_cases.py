"""Case tables, seeded inputs (all made on the CPU), float64 references and comparison helpers for the small kernels that run once per
ray or once per step around the hash grid and the MLPs:

  sampler bookkeeping (exact integers / bitwise float32)
      lse_pack_info_from_counts, lse_compact_ray_slots, lse_ray_planes, lse_fake_sample_if_empty,
      lse_visibility_mask / _cap / _alpha + lse_compact_samples (ops.visibility_compact_deferred)
  per-ray float kernels (bounded float32 against float64)
      lse_ray_bias_fwd / _bwd (+ emb_grad_kernel), lse_ray_features_fwd / _bwd, lse_linear_fwd, lse_linear_bwd_input, lse_gemm_tn_acc,
      lse_segment_sum_rows, lse_density_fwd / _bwd, lse_positions_fwd / _bwd

tests/test_ray_kernel_cases_cpu.py holds this file against itself (float32 torch meets a quarter of every bound, the inputs reach
the kernels' branches, the helpers reject mutated references); tests/test_gpu_ray_kernels.py holds the kernels against it.

Three kinds of comparison:
  ``assert_exact``     integer tensors, torch.equal;
  ``assert_bitwise``   float32 tensors, equal bit patterns (NaN poison and the sign of zero included);
  ``bounded``          float32 against float64: the project's global views (TOL_FWD forward, TOL_GRAD gradients: max error over the
                       tensor's maximum) AND per block (an embedding row, an output-neuron row of W_in, a ray), every block scaled
                       by its OWN maximum (util.blockwise_nmax_err, TOL_GRAD_BLOCK) -- the global view alone lets a small block be
                       entirely wrong behind a large one.  Returns error / bound per view; < 1 passes.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, Optional

import numpy as np
import torch

from oracle import field as ofield
from tests.util import (FIXED_RAY_LENGTHS, TOL_FWD, TOL_GRAD, TOL_GRAD_BLOCK, blockwise_nmax_err, composite_ref, nmax_err,
                        row_bounds, trained_scene_rays, visibility_ref)

POISON_I64 = -0x5A5A5A5A5A5A5A5
POISON_I32 = -0x5A5A5A5
POISON_F32 = -12345.678      # no input or result of any case equals it
U24 = 2.0 ** -24


# ----------------------------------------------------------------------------------------------------
# comparison helpers
# ----------------------------------------------------------------------------------------------------
def assert_exact(got: torch.Tensor, ref: torch.Tensor, what: str = ""):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert not got.dtype.is_floating_point and got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    if not torch.equal(got, ref):
        bad = (got != ref).reshape(-1).nonzero()[:, 0]
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} integers differ, first at flat index {i}: "
                             f"{int(got.reshape(-1)[i])} != {int(ref.reshape(-1)[i])}")


def assert_bitwise(got: torch.Tensor, ref: torch.Tensor, what: str = ""):
    got, ref = got.detach().cpu().contiguous(), ref.detach().cpu().contiguous()
    assert got.dtype == ref.dtype == torch.float32 and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    a, b = got.view(torch.int32), ref.view(torch.int32)
    if not torch.equal(a, b):
        bad = (a != b).reshape(-1).nonzero()[:, 0]
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()} of {got.numel()} floats differ in their bits, first at flat index {i}: "
                             f"{float(got.reshape(-1)[i])!r} != {float(ref.reshape(-1)[i])!r}")


def bounded(name: str, got: torch.Tensor, ref: torch.Tensor, kind: str, bounds=None) -> Dict[str, float]:
    """error / bound of ``got`` (float32) against ``ref`` (float64): ``kind`` "fwd" -> TOL_FWD, "grad" -> TOL_GRAD over the global
    maximum, and with ``bounds`` (flat block boundaries) TOL_GRAD_BLOCK per block over the block's own maximum."""
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite result"
    tol = {"fwd": TOL_FWD, "grad": TOL_GRAD}[kind]
    res = {name: nmax_err(got, ref, 1e-12) / tol}
    if bounds is not None:
        res[name + "_blk"] = blockwise_nmax_err(got, ref, bounds) / TOL_GRAD_BLOCK
    return res


def worst(res: Dict[str, float]):
    k = max(res, key=lambda n: (res[n] if res[n] == res[n] else math.inf))
    return k, res[k]


def assert_within(res: Dict[str, float], limit: float = 1.0, what: str = ""):
    bad = {k: v for k, v in res.items() if not v < limit}
    assert not bad, (what, bad)


def report(case: str, res: Dict[str, float]) -> str:
    """One line per case, in the style of the hash-geometry report: the worst error over its bound."""
    k, v = worst(res) if res else ("-", 0.0)
    line = f"RAYKERNEL {case}: worst {k} = {v:.3f} of its bound ({len(res)} comparisons)"
    print(line)
    return line


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def pack(cnt: torch.Tensor) -> torch.Tensor:
    cnt = cnt.to(torch.int64)
    return torch.stack([torch.cumsum(cnt, 0) - cnt, cnt], -1).contiguous()


# ----------------------------------------------------------------------------------------------------
# lse_pack_info_from_counts: single-workgroup scan, thread t sums the run [t * per, (t + 1) * per), per = ceil(R / 1024)
# ----------------------------------------------------------------------------------------------------
PACK_R = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 65537)
PACK_PATTERNS = ("zeros", "ones", "random", "big_middle", "last_only")
PACK_BIG = 2 ** 33 + 1


def pack_counts(R: int, pattern: str) -> torch.Tensor:
    if pattern == "zeros":
        return torch.zeros(R, dtype=torch.int64)
    if pattern == "ones":
        return torch.ones(R, dtype=torch.int64)
    c = torch.randint(0, 2001, (R,), generator=_gen(1000 + R), dtype=torch.int64)
    if pattern == "big_middle" and R:
        c[R // 2] = PACK_BIG                         # the sums behind it pass 2^32
    if pattern == "last_only":
        c[:-1] = 0
        if R:
            c[-1] = 1 + R % 7
    return c


def pack_reference(cnts: torch.Tensor):
    """(packed_info [R,2], total [1]) by torch.cumsum on int64."""
    incl = torch.cumsum(cnts, 0)
    return torch.stack([incl - cnts, cnts], -1), (incl[-1:] if cnts.numel() else torch.zeros(1, dtype=torch.int64))


def pack_thread_run(R: int) -> int:
    return (R + 1023) // 1024


def mutation_inclusive_offset(packed: torch.Tensor, index: int) -> torch.Tensor:
    m = packed.clone()
    m[index, 0] += m[index, 1]
    return m


# ----------------------------------------------------------------------------------------------------
# lse_compact_ray_slots
# ----------------------------------------------------------------------------------------------------
SLOT_R = (1, 3, 4, 5, 4099)
SLOT_CAP = (1, 63, 64, 65, 200)


def slot_inputs(R: int, cap: int):
    """Per-ray slots as the single-pass marcher leaves them: ray r's ``cnt[r]`` samples at [r * cap, r * cap + cnt[r]), NaN behind.
    Counts are 0 .. cap; ray 0 holds exactly ``cap`` (a lone ray: cap or 0 by the parity of cap), ray 1 exactly 0, the last ray
    ``cap`` again."""
    g = _gen(7 * R + cap)
    cnt = torch.randint(0, cap + 1, (R,), generator=g, dtype=torch.int64)
    cnt[0] = cap if (R > 1 or cap % 2) else 0
    if R > 1:
        cnt[1] = 0
        cnt[-1] = cap
    live = torch.arange(cap)[None, :] < cnt[:, None]
    ts = torch.rand(R, cap, generator=g)
    te = ts + 0.25 + torch.rand(R, cap, generator=g)
    nan = torch.full((R, cap), math.nan)
    ts_slots, te_slots = torch.where(live, ts, nan).reshape(-1), torch.where(live, te, nan).reshape(-1)
    packed = pack(cnt)
    ref = {"ray_indices": torch.repeat_interleave(torch.arange(R, dtype=torch.int32), cnt), "t_starts": ts[live], "t_ends": te[live]}
    return {"cnt": cnt, "packed": packed, "ts_slots": ts_slots.contiguous(), "te_slots": te_slots.contiguous(), "total": int(cnt.sum()),
            "capacity": R * cap + 3, "ref": ref}


def check_compacted(got: Dict[str, torch.Tensor], inp) -> None:
    """The packed prefix equals the gather; everything at or beyond the total keeps its poison."""
    n = inp["total"]
    assert_exact(got["ray_indices"][:n], inp["ref"]["ray_indices"], "ray_indices")
    assert_exact(got["ray_indices"][n:], torch.full((inp["capacity"] - n,), POISON_I32, dtype=torch.int32), "ray_indices beyond the total")
    for k in ("t_starts", "t_ends"):
        assert_bitwise(got[k][:n], inp["ref"][k], k)
        assert_bitwise(got[k][n:], torch.full((inp["capacity"] - n,), POISON_F32), k + " beyond the total")


# ----------------------------------------------------------------------------------------------------
# lse_ray_planes
# ----------------------------------------------------------------------------------------------------
PLANES_R = (1, 255, 256, 257, 4099)
PLANES_COMBOS = tuple((a, b, c) for a in (False, True) for b in (False, True) for c in (False, True))     # t_min, t_max, jitter present
PLANES_NEAR, PLANES_FAR, PLANES_STEP = 0.05, 6.0, 3.1


def planes_inputs(R: int):
    """t_min on both sides of the near plane, t_max on both sides of the far plane, u with full 24-bit mantissas.  The step (3.1: not
    a power of two, and large against the near plane) makes u * step inexact AND of the magnitude of the sum, so that rounding the
    product first changes the sum's last bit in about a quarter of the rays (with the automatic render step, 0.0035, in under 1 %)."""
    g = _gen(31 + R)
    return {"t_min": torch.rand(R, generator=g) * 0.3, "t_max": 0.5 + torch.rand(R, generator=g) * 8.0, "jitter": torch.rand(R, generator=g)}


def planes_reference(inp, has_min: bool, has_max: bool, has_jit: bool, fused: bool = False):
    """float32 torch: maximum, minimum, near + u * step as two roundings (``fused``: one rounding, what an FMA would give)."""
    R = inp["t_min"].shape[0]
    near = torch.full((R,), PLANES_NEAR, dtype=torch.float32)
    far = torch.full((R,), PLANES_FAR, dtype=torch.float32)
    step = torch.tensor(PLANES_STEP, dtype=torch.float32)
    if has_min:
        near = torch.maximum(near, inp["t_min"])
    if has_max:
        far = torch.minimum(far, inp["t_max"])
    if has_jit:
        if fused:       # the product of two float32 is exact in float64; the sum is rounded to float64, then to float32
            near = (near.double() + inp["jitter"].double() * step.double()).float()
        else:
            near = near + inp["jitter"] * step
    return near, far


# ----------------------------------------------------------------------------------------------------
# lse_fake_sample_if_empty
# ----------------------------------------------------------------------------------------------------
FAKE_SHAPES = ((16, 2), (4, 2), (1, 8))       # (levels, features); level stride = capacity * features > features
FAKE_R, FAKE_CAPACITY = 3, 5


def fake_buffers(levels: int, features: int, n_dev: int):
    C = FAKE_CAPACITY
    return {"packed": torch.full((FAKE_R, 2), POISON_I64, dtype=torch.int64), "n_dev": torch.tensor([n_dev], dtype=torch.int64),
            "ray_indices": torch.full((C,), POISON_I32, dtype=torch.int32), "t_starts": torch.full((C,), POISON_F32),
            "t_ends": torch.full((C,), POISON_F32), "x01": torch.full((C, 3), POISON_F32), "sel": torch.full((C,), 0xA5, dtype=torch.uint8),
            "y": torch.full((levels, C, features), POISON_F32)}


def fake_expected(buf):
    """What the buffers hold afterwards: untouched unless n_dev == 0; then the sample (ray 0, t = 1, 1) and slot 0 of the features
    zeroed, every other element as it was."""
    out = {k: v.clone() for k, v in buf.items()}
    if int(buf["n_dev"]) == 0:
        out["packed"][0, 0], out["packed"][0, 1] = 0, 1
        out["n_dev"][0] = 1
        out["ray_indices"][0] = 0
        out["t_starts"][0] = out["t_ends"][0] = 1.0
        out["x01"][0] = 0.0
        out["sel"][0] = 0
        out["y"][:, 0, :] = 0.0
    return out


def check_fake(got, exp):
    for k, v in exp.items():
        (assert_bitwise if v.dtype == torch.float32 else assert_exact)(got[k], v, k)


# ----------------------------------------------------------------------------------------------------
# visibility routes (ops.visibility_compact_deferred)
# ----------------------------------------------------------------------------------------------------
VIS_SIGMA, VIS_STEP, VIS_EPS, VIS_ALPHA_THRE, VIS_BAND = 1e3, "const", 1e-4, 0.01, 1e-5
VIS_CAP_BELOW, VIS_CAP_ABOVE = 0.001, 0.5         # on either side of alpha_thre; the haze (alpha < 0.0018) straddles the lower one
VIS_MAX_UNDECIDED = 0.002
VIS_PAD = 37                                       # capacity extent: the sample arrays are this much longer than the count


@functools.lru_cache(maxsize=None)
def vis_inputs():
    inp = trained_scene_rays(VIS_SIGMA, seed=1, step=VIS_STEP, lengths=FIXED_RAY_LENGTHS)
    ref = composite_ref(inp["ts"], inp["te"], inp["sigma"], inp["packed_info"])
    inp["alphas_f32"] = 1.0 - torch.exp(-inp["sigma"] * (inp["te"] - inp["ts"]))        # float32 opacities for the from_alpha route
    return inp, ref


def vis_threshold(alpha_thre: float, cap: Optional[float], combine=min) -> float:
    return alpha_thre if cap is None else combine(alpha_thre, cap)


def vis_density_ref(alpha_thre: float, cap: Optional[float] = None, combine=min):
    """(mask, undecided) in float64 for the density routes; ``cap``: the alpha_cap route's min(alpha_thre, cap)."""
    _, ref = vis_inputs()
    return visibility_ref(ref, VIS_EPS, vis_threshold(alpha_thre, cap, combine), VIS_BAND)


def vis_alpha_ref(alpha_thre: float):
    """(mask, undecided) of the from_alpha route: T_k = prod_{i<k} (1 - alpha_i) inside the ray by float64 cumprod, the same band
    rule on T / eps and alpha / alpha_thre."""
    inp, _ = vis_inputs()
    a = inp["alphas_f32"].double()
    T = torch.ones_like(a)
    for s, c in inp["packed_info"].tolist():
        if c > 1:
            T[s + 1:s + c] = torch.cumprod(1.0 - a[s:s + c - 1], 0)
    vis = (T >= VIS_EPS) & (a >= alpha_thre)
    und = ((T / VIS_EPS - 1).abs() < VIS_BAND) | ((a / alpha_thre - 1).abs() < VIS_BAND)
    return vis, und


def check_mask(mask: torch.Tensor, vis: torch.Tensor, und: torch.Tensor) -> int:
    """The band rule of test_visibility_prepass_and_render_agree: outside the band the mask is the float64 one; the band holds at
    most 0.2 % of the samples."""
    assert float(und.float().mean()) <= VIS_MAX_UNDECIDED
    wrong = int((mask.cpu().bool() != vis)[~und].sum())
    assert wrong == 0, f"{wrong} samples outside the band differ from the float64 mask"
    return int(und.sum())


def check_compaction(out, inputs, n: int) -> None:
    """out = (ray_indices, t_starts, t_ends, new_packed, mask, n_dev) of visibility_compact_deferred; ``inputs`` = the (ray_indices
    int32, t_starts, t_ends, packed_info) it was given, ``n`` their sample count (the arrays may be longer)."""
    o_ri, o_ts, o_te, new_packed, mask, n_dev = (t.cpu() for t in out)
    ri, ts, te, packed = (t.cpu() for t in inputs)
    m = mask[:n].bool()
    total = int(m.sum())
    assert_exact(n_dev, torch.tensor([total], dtype=torch.int64), "n_dev")
    cnt = torch.zeros(packed.shape[0], dtype=torch.int64).index_add_(0, ri[:n].long(), m.long())
    assert_exact(new_packed, pack(cnt), "new_packed")
    assert_exact(o_ri[:total], ri[:n][m], "ray_indices")
    assert_bitwise(o_ts[:total], ts[:n][m], "t_starts")
    assert_bitwise(o_te[:total], te[:n][m], "t_ends")


# ----------------------------------------------------------------------------------------------------
# lse_ray_bias_fwd / _bwd, emb_grad_kernel, lse_ray_features_fwd / _bwd
# ----------------------------------------------------------------------------------------------------
# (name, width, emb_dim (None: no embedding), R, embedding rows, index pattern)
#   patterns: one_row (all rays on row 0), own_row (ray r on row r), blocks (contiguous blocks per camera), random, sparse (random
#   among the even rows: the odd ones get no ray)
RAY_BIAS_CASES = (
    ("w64_e32_R4099_rows1000_random", 64, 32, 4099, 1000, "random"),
    ("w64_e32_R4099_rows3_blocks", 64, 32, 4099, 3, "blocks"),
    ("w32_e32_R4099_rows1_one", 32, 32, 4099, 1, "one_row"),
    ("w64_none_R17", 64, None, 17, 0, "none"),
    ("w32_none_R4099", 32, None, 4099, 0, "none"),
    ("w64_e1_R16_rows3_random", 64, 1, 16, 3, "random"),
    ("w32_e16_R15_rows1000_own", 32, 16, 15, 1000, "own_row"),
    ("w64_e17_R17_rows1000_own", 64, 17, 17, 1000, "own_row"),
    ("w32_e33_R1_rows3", 32, 33, 1, 3, "random"),
    ("w64_e97_R4099_rows3_blocks", 64, 97, 4099, 3, "blocks"),
    ("w32_e97_R17_rows1_one", 32, 97, 17, 1, "one_row"),
    ("w64_e16_R1_rows1", 64, 16, 1, 1, "one_row"),
    ("w32_e1_R4099_rows1000_sparse", 32, 1, 4099, 1000, "sparse"),
    ("w64_e33_R15_rows3_sparse", 64, 33, 15, 3, "sparse"),
)
RAY_BIAS_BY_NAME = {c[0]: c for c in RAY_BIAS_CASES}
RAW_LD_CASE = ("raw_w64_e32_R257_rows3_ld80", 64, 32, 257, 3, "random")       # the raw C-ABI case: w_ld = in_pad + 16
RAY_FEATURES_R, RAY_FEATURES_ROWS = (1, 255, 256, 257), (1, 300)
EMB_PARTITIONS = 64          # emb_grad_kernel: 8 ray partitions per workgroup x gridDim.y = 8, combined by atomics


def in_pad_of(emb_dim: Optional[int]) -> int:
    return (31 + (emb_dim or 0) + 15) // 16 * 16


def special_directions(g) -> torch.Tensor:
    u = torch.randn(2, 3, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    eye = torch.eye(3)
    return torch.cat([eye, -eye, 0.25 * u[:1], 3.0 * u[1:], torch.zeros(1, 3)])      # +-axes, lengths 0.25 and 3, the zero vector


def emb_partitions(R: int):
    """[(r0, r1)] of emb_grad_kernel's 64 ray partitions."""
    per = (R + EMB_PARTITIONS - 1) // EMB_PARTITIONS
    return [(min(R, p * per), min(R, min(R, p * per) + per)) for p in range(EMB_PARTITIONS)]


def ray_bias_inputs(case, seed: int = 0):
    name, width, emb_dim, R, rows, pattern = case
    g = _gen(seed * 7919 + sum(map(ord, name)))
    d = torch.randn(R, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    sp = special_directions(g)
    k = min(sp.shape[0], R - 1)
    d[1:1 + k] = sp[:k]                     # ray 0 stays a random unit vector
    in_pad = in_pad_of(emb_dim)
    emb = idx = None
    if emb_dim is not None:
        emb = torch.randn(rows, emb_dim, generator=g)
        if pattern == "one_row":
            idx = torch.zeros(R, dtype=torch.int64)
        elif pattern == "own_row":
            idx = torch.arange(R)
        elif pattern == "blocks":
            idx = (torch.arange(R) * rows) // R
        elif pattern == "random":
            idx = torch.randint(0, rows, (R,), generator=g)
        else:
            assert pattern == "sparse", pattern
            idx = 2 * torch.randint(0, (rows + 1) // 2, (R,), generator=g)
    n_head = width * in_pad + width * width + 16 * width      # W_in first, the rest of the head's parameters behind it
    head = torch.randn(n_head, generator=g) * 0.3
    # upstream gradient: the rays of embedding row e weigh 10^-(e % 4), so that the rows' gradients differ by orders of magnitude
    gout = torch.randn(R, width, generator=g)
    if idx is not None:
        gout = gout * (10.0 ** -(idx % 4).float())[:, None]
    return {"case": case, "dirs": d.contiguous(), "emb": emb, "idx": idx, "head": head, "gout": gout.contiguous(), "width": width,
            "emb_dim": emb_dim, "in_pad": in_pad, "R": R, "rows": rows}


def _features(d, emb, idx, in_pad, dtype, mutation=None):
    R = d.shape[0]
    sh = ofield.sh4_tcnn((d + 1) / 2)
    if mutation == "sh_sign":
        sh = torch.cat([sh[:, :12], -sh[:, 12:13], sh[:, 13:]], -1)           # a degree-3 coefficient with its sign flipped
    parts = [sh, torch.zeros(R, 15, dtype=dtype)]
    if emb is not None:
        parts.append(emb[idx])
    used = 31 + (0 if emb is None else emb.shape[1])
    pad = torch.zeros if mutation == "zero_padding" else torch.ones
    parts.append(pad(R, in_pad - used, dtype=dtype))
    return torch.cat(parts, -1)


def ray_bias_eval(inp, dtype=torch.float64, mutation: Optional[str] = None, g_feat: Optional[torch.Tensor] = None):
    """row_bias = [SH16((d + 1) / 2) | 0 x 15 | emb[idx] | ones] W_in^T and its gradients for the upstream ``gout`` by torch autograd
    in ``dtype`` (float64: the reference; float32: the restatement).  ``g_feat``: upstream gradient on the FEATURES instead (the
    lse_ray_features pair).  ``mutation``: "sh_sign" | "zero_padding" -- deliberately wrong variants for the CPU tier."""
    width, in_pad = inp["width"], inp["in_pad"]
    d = inp["dirs"].to(dtype).clone().requires_grad_(True)
    emb = None if inp["emb"] is None else inp["emb"].to(dtype).clone().requires_grad_(True)
    head = inp["head"].to(dtype).clone().requires_grad_(True)
    feat = _features(d, emb, inp["idx"], in_pad, dtype, mutation)
    rb = feat @ head[: width * in_pad].view(width, in_pad).t()
    if g_feat is not None:
        (feat * g_feat.to(dtype)).sum().backward()
    else:
        (rb * inp["gout"].to(dtype)).sum().backward()
    return {"row_bias": rb.detach(), "feat": feat.detach(), "d_dirs": d.grad, "d_emb": None if emb is None else emb.grad,
            "d_head": head.grad if head.grad is not None else torch.zeros_like(head)}


def compare_ray_bias(got: Dict[str, torch.Tensor], ref: Dict[str, torch.Tensor], inp, preload: Optional[Dict[str, torch.Tensor]] = None,
                     keys=("row_bias", "d_dirs", "d_emb", "d_w_in")) -> Dict[str, float]:
    """error / bound of row_bias [R, width], d_dirs [R, 3], d_emb [rows, emb_dim], d_head (the whole head gradient; its W_in part per
    output row, the rest exactly the preload or 0).  ``preload``: what d_emb / d_head held before the backward (the result is the
    preload plus the reference).  Rows of the embedding that no ray uses: exactly the preload (0 without one)."""
    width, in_pad, R = inp["width"], inp["in_pad"], inp["R"]
    res = {}
    if "row_bias" in keys:
        res.update(bounded("row_bias", got["row_bias"].cpu(), ref["row_bias"], "fwd", row_bounds(R, width)))
    if "d_dirs" in keys:
        res.update(bounded("d_dirs", got["d_dirs"].cpu(), ref["d_dirs"], "grad", row_bounds(R, 3)))
    if "d_emb" in keys and ref["d_emb"] is not None:
        rows, e = ref["d_emb"].shape
        pre = torch.zeros(rows, e) if preload is None else preload["d_emb"]
        g = got["d_emb"].cpu()
        unused = torch.ones(rows, dtype=torch.bool)
        unused[inp["idx"]] = False
        assert_bitwise(g[unused], pre[unused], "d_emb rows that no ray uses")
        res.update(bounded("d_emb", g, pre.double() + ref["d_emb"], "grad", row_bounds(rows, e)))
    if "d_w_in" in keys:
        n_in = width * in_pad
        pre = torch.zeros_like(inp["head"]) if preload is None else preload["d_head"]
        g = got["d_head"].cpu()
        assert_bitwise(g[n_in:], pre[n_in:], "gradient of the head's other layers")
        res.update(bounded("d_w_in", g[:n_in], pre[:n_in].double() + ref["d_head"][:n_in], "grad", row_bounds(width, in_pad)))
    return res


def mutation_scaled_small_row(ref, inp, factor: float = 1.01):
    """The embedding row with the smallest non-zero gradient scaled by ``factor``, every other row exact."""
    m = dict(ref)
    g = ref["d_emb"].clone()
    mx = g.abs().amax(-1)
    row = int(torch.where(mx > 0, mx, torch.full_like(mx, math.inf)).argmin())
    g[row] *= factor
    m["d_emb"] = g
    return m, row


def ray_features_inputs(R: int, rows: int):
    return ray_bias_inputs((f"features_R{R}_rows{rows}", 64, 32, R, rows, "random"))


def feature_upstream(inp) -> torch.Tensor:
    return torch.randn(inp["R"], 64, generator=_gen(5 + inp["R"] + inp["rows"]))


def compare_ray_features(got, ref, inp) -> Dict[str, float]:
    R, rows = inp["R"], inp["rows"]
    res = bounded("d_dirs", got["d_dirs"].cpu(), ref["d_dirs"], "grad", row_bounds(R, 3))
    res.update(bounded("d_emb", got["d_emb"].cpu(), ref["d_emb"], "grad", row_bounds(rows, 32)))
    return res


# ----------------------------------------------------------------------------------------------------
# lse_linear_fwd, lse_linear_bwd_input, lse_gemm_tn_acc
# ----------------------------------------------------------------------------------------------------
ROWMAJOR, LEVELMAJOR = 0, 1
# every (m, k, layout) instance of gemm_tn_dispatch (csrc/mlp.hip)
GEMM_INSTANCES = ((64, 32, LEVELMAJOR), (64, 8, LEVELMAJOR), (32, 8, LEVELMAJOR), (32, 32, LEVELMAJOR), (64, 16, ROWMAJOR),
                  (64, 32, ROWMAJOR), (64, 64, ROWMAJOR), (32, 16, ROWMAJOR), (32, 64, ROWMAJOR), (32, 32, ROWMAJOR), (16, 64, ROWMAJOR),
                  (16, 32, ROWMAJOR))
GEMM_ROWS = (1, 3, 4, 5, 6, 7, 255, 4099)
GEMM_NOT_BUILT = ((48, 64, ROWMAJOR), (64, 24, ROWMAJOR), (16, 16, LEVELMAJOR))
GEMM_LD_EXTRA = 5          # dw_ld = k + 5 > k


def gemm_inputs(m: int, k: int, layout: int, n: int):
    g = _gen(m * 1000 + k * 10 + layout + 17 * n)
    x = torch.randn(n, k, generator=g)
    w = torch.randn(m, k, generator=g) * 0.2
    dy = torch.randn(n, m, generator=g)
    # output neuron o weighs 10^-(o % 3): the rows of dW differ by orders of magnitude
    dy = dy * (10.0 ** -(torch.arange(m) % 3).float())[None, :]
    dw_pre = torch.randn(m, k + GEMM_LD_EXTRA, generator=g) * 0.37
    return {"x": x, "w": w, "dy": dy.contiguous(), "dw_pre": dw_pre, "m": m, "k": k, "layout": layout, "n": n}


def level_major(x: torch.Tensor) -> torch.Tensor:
    """[n, k] -> [k / 2][n][2], the layout lse_hash_fwd writes (the row count is the level stride)."""
    n, k = x.shape
    return x.view(n, k // 2, 2).permute(1, 0, 2).contiguous()


def gemm_eval(inp, dtype=torch.float64):
    x, w, dy = (inp[k].to(dtype) for k in ("x", "w", "dy"))
    return {"y": x @ w.t(), "dx": dy @ w, "dw": inp["dw_pre"][:, : inp["k"]].to(dtype) + dy.t() @ x}


def compare_gemm(got, ref, inp, keys=("y", "dx", "dw")) -> Dict[str, float]:
    m, k, n = inp["m"], inp["k"], inp["n"]
    res = {}
    if "y" in keys:
        res.update(bounded("y", got["y"].cpu(), ref["y"], "fwd", row_bounds(n, m)))
    if "dx" in keys:
        res.update(bounded("dx", got["dx"].cpu(), ref["dx"], "grad", row_bounds(n, k)))
    if "dw" in keys:
        g = got["dw"].cpu()
        assert g.shape == (m, k + GEMM_LD_EXTRA)
        assert_bitwise(g[:, k:].contiguous(), inp["dw_pre"][:, k:].contiguous(), "dW beyond column k")
        res.update(bounded("dw", g[:, :k].contiguous(), ref["dw"], "grad", row_bounds(m, k)))
    return res


# ----------------------------------------------------------------------------------------------------
# lse_segment_sum_rows
# ----------------------------------------------------------------------------------------------------
SEG_WIDTHS = (1, 4, 16, 63, 64)
SEG_LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 200)
SEG_R = (1, 4, 5, 4099)
SEG_BAD_WIDTHS = (0, 65)
SEG_QUANTUM = 2.0 ** -12


def seg_lengths(width: int, R: int):
    """Ray r has length SEG_LENGTHS[(r + offset) % 9]; the offset moves with the width and the ray count, so the lone ray of R = 1
    takes a different length at every width and every length occurs with R = 4099."""
    off = 1 + SEG_WIDTHS.index(width) + 3 * SEG_R.index(R)
    return [SEG_LENGTHS[(r + off) % len(SEG_LENGTHS)] for r in range(R)]


def seg_inputs(width: int, R: int):
    """rows [N, width] and the preloaded ``out`` [R, width] (the kernel adds into it).

    Every value is a multiple of 2^-12 in (-1, 1): a sum of up to 201 of them has at most 21 significant bits, so EVERY order of
    summation is exact in float32.  Values with full mantissas were tried first and do not meet the CPU tier's quarter rule: at a ray
    of 3 rows of one sign the three roundings of a correct float32 sum reach 3 * 2^-24 * sum|rows| against a quarter bound of
    (3 / 16 + 1) * 2^-24 * sum|rows|, and the addition into a preloaded ``out`` rounds in proportion to |out|, which sum|rows| does not
    bound at all (measured: up to 1170 times the bound with N(0, 1) rows and preload).  The inputs were changed, the bound is the one
    stated (``seg_bound``)."""
    cnt = torch.tensor(seg_lengths(width, R), dtype=torch.int64)
    n = int(cnt.sum())
    g = _gen(width * 100 + R)
    q = lambda *shape: torch.randint(-4095, 4096, shape, generator=g).float() * SEG_QUANTUM      # noqa: E731
    return {"rows": q(n, width), "pre": q(R, width), "cnt": cnt, "packed": pack(cnt), "width": width, "R": R}


def seg_eval(inp, dtype=torch.float64, drop_tail: bool = False):
    """pre + per-ray sums.  ``drop_tail``: a sum that leaves out the last cnt % 4 rows of every ray (mutation)."""
    cnt, width, R = inp["cnt"], inp["width"], inp["R"]
    ri = torch.repeat_interleave(torch.arange(R), cnt)
    rows = inp["rows"].to(dtype)
    if drop_tail:
        k = torch.arange(rows.shape[0]) - inp["packed"][:, 0][ri]
        rows = rows * (k < (cnt - cnt % 4)[ri]).to(dtype)[:, None]
    return inp["pre"].to(dtype) + torch.zeros(R, width, dtype=dtype).index_add_(0, ri, rows)


def seg_bound(inp) -> torch.Tensor:
    """Per element [R, width]: (cnt / 4 + 4) * 2^-24 * sum|rows| over the ray and the column -- four accumulators of cnt / 4 terms
    each, their two-level combination and the addition into ``out``."""
    cnt, width, R = inp["cnt"], inp["width"], inp["R"]
    ri = torch.repeat_interleave(torch.arange(R), cnt)
    s = torch.zeros(R, width, dtype=torch.float64).index_add_(0, ri, inp["rows"].double().abs())
    return (cnt.double() / 4 + 4)[:, None] * U24 * s


def compare_seg(got: torch.Tensor, ref: torch.Tensor, inp) -> Dict[str, float]:
    """error / bound, worst element; where the bound is 0 (a ray without rows) the result must be the preload exactly."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    err, bound = (got - ref).abs(), seg_bound(inp)
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return {"segment_sum": float(ratio.max())}


# ----------------------------------------------------------------------------------------------------
# lse_density_fwd / _bwd
# ----------------------------------------------------------------------------------------------------
DENSITY_N = (1, 255, 256, 257)
DENSITY_SELECTORS = ("none", "zeros", "mixed")
DENSITY_SCALE = 0.5           # a power of two: the multiply is exact, the error is the exponential's
F32_MIN_NORMAL = 2.0 ** -126
F32_MAX = float(np.finfo(np.float32).max)


def density_special_h() -> torch.Tensor:
    f = np.float32
    v = []
    for c in (15.0, -15.0):
        v += [np.nextafter(f(c), f(-np.inf)), f(c), np.nextafter(f(c), f(np.inf))]
    v += [f(0.0), f(80.0), f(-80.0), f(89.0), f(-104.0)]
    return torch.from_numpy(np.asarray(v, dtype=np.float32))


def density_inputs(n: int, selector: str):
    """h [n, 16] (column 0 is the density logit, the rest poison that nothing may read into the result), selector, d_sigma = +-2^k
    (exact multiplies again).  n = 1 holds the float32 neighbour above 15, where the backward's clamp and the forward part."""
    g = _gen(3 * n + DENSITY_SELECTORS.index(selector))
    h0 = (torch.rand(n, generator=g) * 40 - 20)
    sp = density_special_h()
    if n == 1:
        h0[0] = sp[2]
    else:
        h0[: sp.numel()] = sp
    h = torch.full((n, 16), POISON_F32)
    h[:, 0] = h0
    sel = {"none": None, "zeros": torch.zeros(n, dtype=torch.uint8), "mixed": (torch.arange(n) % 3 != 1).to(torch.uint8)}[selector]
    d_sigma = torch.sign(torch.randn(n, generator=g)) * 2.0 ** torch.randint(-3, 4, (n,), generator=g).float()
    return {"h": h, "sel": sel, "d_sigma": d_sigma, "n": n}


def density_eval(inp, dtype=torch.float64):
    """sigma = scale * exp(h0) * selector (no clamp); d_h0 = d_sigma * scale * exp(clamp(h0, -15, 15)) * selector: trunc_exp."""
    h0 = inp["h"][:, 0].to(dtype)
    s = torch.ones_like(h0) if inp["sel"] is None else inp["sel"].to(dtype)
    e = torch.exp(h0)
    e = torch.where(e > F32_MAX, torch.full_like(e, math.inf), e)        # float32 trunc_exp overflows to +inf there (h0 = 89), and so must the kernel
    sigma = torch.where(s > 0, DENSITY_SCALE * e, torch.zeros_like(h0))
    d_h0 = torch.where(s > 0, inp["d_sigma"].to(dtype) * DENSITY_SCALE * torch.exp(h0.clamp(-15, 15)), torch.zeros_like(h0))
    return {"sigma": sigma, "d_h0": d_h0}


def _rel_err(got: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """|got - ref| / max(|ref|, smallest normal float32): below the normal range float32 keeps an absolute precision, not a relative
    one (and a flushed denormal is as good as a kept one).  Where the reference is infinite, the same infinity is the exact answer."""
    got, ref = got.detach().cpu().double(), ref.double()
    over = torch.isinf(ref)
    err = (got - ref).abs() / ref.abs().clamp_min(F32_MIN_NORMAL)
    return torch.where(over, torch.where(got == ref, torch.zeros_like(err), torch.full_like(err, math.inf)), err)


@functools.lru_cache(maxsize=None)
def density_exp_error() -> float:
    """Worst relative error of float32 torch.exp against float64 over the logits of every density case (measured, on the CPU)."""
    w = 0.0
    for n in DENSITY_N:
        h0 = density_inputs(n, "none")["h"][:, 0]
        for x in (h0, h0.clamp(-15, 15)):
            e = torch.exp(x.double())
            w = max(w, float(_rel_err(torch.exp(x), torch.where(e > F32_MAX, torch.full_like(e, math.inf), e)).max()))
    return w


def density_bound() -> float:
    return max(4.0 * density_exp_error(), 2.0 ** -22)


def compare_density(got, ref, inp) -> Dict[str, float]:
    res = {}
    unsel = torch.zeros(inp["n"], dtype=torch.bool) if inp["sel"] is None else inp["sel"] == 0
    for k in ("sigma", "d_h0"):
        g = got[k].detach().cpu()
        assert float(g[unsel].abs().max() if bool(unsel.any()) else 0.0) == 0.0, f"{k}: an unselected sample is not exactly 0"
        res[k] = float(_rel_err(g, ref[k]).max()) / density_bound()
    return res


# ----------------------------------------------------------------------------------------------------
# lse_positions_fwd / _bwd
# ----------------------------------------------------------------------------------------------------
POS_AABB = ((-1.0, -2.0, -0.5), (1.0, 2.0, 1.5))          # extents 2, 4, 2: dividing by them is exact
POS_R = (1, 4, 5, 4099)
POS_LENGTHS = (200, 0, 1, 3, 64, 65, 5, 63, 4)
POS_NDEV_N = 300
FACE_BAND = 1e-5             # unit-cube coordinates this close to 0 or 1: float32 and float64 may select differently
TIED_POINTS = ((2.0, 2.0, 1.0), (2.0, -2.0, 2.0), (-3.0, 1.0, 3.0), (1.5, 0.25, -1.5), (-4.0, -4.0, -4.0))


def _step(v: float, up: bool) -> float:
    return float(np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf)))


def crafted_points(contraction: bool) -> torch.Tensor:
    """Points whose float32 arithmetic is exact (a few powers of two summed) or lands one float32 step beside a face."""
    pts = []
    if contraction:
        pts += [(1.0, 0.5, -0.25), (-1.0, 0.25, 0.5), (0.5, 1.0, 0.125), (0.25, -1.0, -0.5), (0.125, 0.5, 1.0), (-0.5, -0.25, -1.0)]     # |p|_inf == 1
        pts += [(1e10, 0.5, -3.0), (-0.25, -1e10, 2.0), (3e38, 1.0, 1.0), (0.0, 2.0, -3e38)]      # the contraction gives exactly 2
        pts += [(2.0, 0.5, -1.0), (-0.75, 4.0, 1.5), (0.5, -0.25, 0.75), (0.0, 0.0, 0.0), (-8.0, 3.0, 0.5)]
        for k in range(3):                                        # one float32 step on either side of |p_k| = 1
            for sgn in (1.0, -1.0):
                for up in (False, True):
                    p = [0.5, -0.25, 0.125]
                    p[k] = sgn * _step(1.0, up)
                    pts.append(tuple(p))
    else:
        lo, hi = POS_AABB
        mid = [0.0, 0.5, 0.75]
        pts += [lo, hi, tuple(mid)]                               # p == lo, p == hi, inside
        for k in range(3):
            for face in (lo[k], hi[k]):
                on = list(mid); on[k] = face; pts.append(tuple(on))           # exactly on the face
                for up in (False, True):                          # one float32 step on either side of it
                    p = list(mid); p[k] = _step(face, up); pts.append(tuple(p))
    return torch.tensor(pts, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _field_oracle(contraction: bool):
    return ofield.FieldOracle("tcnn", contraction=contraction, aabb=torch.tensor(POS_AABB), log2_hashmap_size=10, num_levels=4)


def field_oracle(contraction: bool, dtype=torch.float32):
    fo = _field_oracle(contraction)
    fo.aabb = torch.tensor(POS_AABB, dtype=dtype)
    return fo


def positions_f32_oracle(points: torch.Tensor, contraction: bool):
    """(x01, selector) of oracle.field in float32, no face band left out."""
    x01, sel = field_oracle(contraction).normalize(points.float())
    return x01 + 0.0, sel          # (+ 0.0: the oracle's p * False leaves -0.0 for negative p; the kernel stores +0.0)


def positions_inputs(R: int, contraction: bool, direct: bool):
    """Seeded rays that start inside the unit box and leave it: samples on both sides of |p|_inf = 1 (both contraction branches) and
    of the aabb's faces.  ``direct``: the sample positions themselves are the input (Field.density_fn), one per former sample."""
    g = _gen(11 * R + 2 * int(contraction) + int(direct))
    o = (torch.rand(R, 3, generator=g) - 0.5) * 1.2
    d = torch.randn(R, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    cnt = torch.tensor([POS_LENGTHS[r % len(POS_LENGTHS)] for r in range(R)], dtype=torch.int64)
    packed = pack(cnt)
    n = int(cnt.sum())
    ri = torch.repeat_interleave(torch.arange(R), cnt)
    k = torch.arange(n) - packed[:, 0][ri]
    dt = 3.2 / cnt.clamp_min(1).float()[ri]                        # every ray spans t in [0, 3.2]
    ts = k.float() * dt + 0.3 * dt * torch.rand(n, generator=g)
    te = ts + 0.5 * dt
    w = torch.rand(n, 3, generator=g) + 0.1
    out = {"R": R, "contraction": contraction, "direct": direct, "cnt": cnt, "packed": packed, "ri": ri, "ts": ts, "te": te, "w": w, "n": n}
    if direct:
        out["points"] = ofield.frustum_positions(o[ri], d[ri], ts[:, None], te[:, None]).contiguous()
    else:
        out["o"], out["d"] = o.contiguous(), d.contiguous()
    return out


def positions_eval(inp, dtype=torch.float64, points: Optional[torch.Tensor] = None, upstream: Optional[torch.Tensor] = None):
    """x01, selector and d(position) per sample [n, 3] for the upstream ``w`` on x01 (oracle.field + autograd in ``dtype``)."""
    fo = field_oracle(inp["contraction"], dtype)
    if points is not None or inp["direct"]:
        pos = (inp["points"] if points is None else points).to(dtype).clone().requires_grad_(True)
    else:
        pos = ofield.frustum_positions(inp["o"].to(dtype)[inp["ri"]], inp["d"].to(dtype)[inp["ri"]], inp["ts"].to(dtype)[:, None],
                                       inp["te"].to(dtype)[:, None]).detach().requires_grad_(True)
    x01, sel = fo.normalize(pos)
    w = (inp["w"] if upstream is None else upstream).to(dtype)
    (x01 * w).sum().backward()
    return {"x01": x01.detach(), "sel": sel, "d_pos": pos.grad, "pos": pos.detach()}


def positions_reference(inp):
    """float64 reference + ``edge`` [n]: the samples whose unit-cube coordinates lie within 1e-5 of a face."""
    ref = positions_eval(inp)
    p = ref["pos"]
    raw = (ofield.contract_inf(p) + 2.0) / 4.0 if inp["contraction"] else ofield.normalized_positions(p, torch.tensor(POS_AABB, dtype=torch.float64))
    ref["edge"] = ((raw - 0.5).abs() - 0.5).abs().amin(-1) < FACE_BAND
    return ref


def tied_invariants(points: torch.Tensor, grad: torch.Tensor):
    """What every sub-gradient of the L-inf norm agrees on at a tie: the components of the untied axes, and the sum of
    sign(p_k) * grad_k over the tied (maximal) axes.  Returns (untied [n, 3] with the tied entries zeroed, tied sums [n])."""
    points, grad = points.double().cpu(), grad.double().cpu()
    a = points.abs()
    tied = a == a.amax(-1, keepdim=True)
    return torch.where(tied, torch.zeros_like(grad), grad), (torch.sign(points) * grad * tied).sum(-1)
