"""Shared data and helpers of the loss-epilogue size tests (tests/test_epilogue_cases_cpu.py, tests/test_gpu_epilogue_sizes.py).
Not a test file; imports no GPU code.

The reference is ``oracle/losses.py`` on float64 tensors and nothing else: both losses and every gradient (the three ray tensors,
the two powpow coefficients, the ThreeToOne weights, all eight tensors of each MLP mapper) for the upstream weights (1.3, 0.6), the
colour share and the event share kept apart so that one reference serves the both-bundles, one-bundle and one-loss checks.
Everything here runs on the CPU: the descriptor table, the seeded inputs, the reference (computed once per process and case, shared,
never modified), the comparison both tiers use and the mutated copies of the reference that show the comparison would notice a
subtly wrong kernel.

The float32 constant of the clamp.  ``torch.clamp(x, 1e-5)`` on a float32 tensor compares with float32(1e-5) = 9.99999974e-6, and
so do the kernels; on a float64 tensor it compares with the double 1e-5, which is LARGER, so a float32 input of exactly
float32(1e-5) would pass its gradient in float32 and lose it in float64.  ``as_dtype`` therefore hands the float64 evaluation the
double constant 1e-5 wherever the float32 input holds float32(1e-5): the same side of the same clamp, a value 2.5e-13 away."""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from lsenerf_amd import _lib
from oracle import losses as ol
from tests.util import nmax_err

ID, GT, POWPOW, MLP, RGB_MLP = _lib.LSE_MAP_IDENTITY, _lib.LSE_MAP_GT, _lib.LSE_MAP_POWPOW, _lib.LSE_MAP_MLP, _lib.LSE_MAP_RGB_MLP
NONE, LEARNED, GRAY = _lib.LSE_ONE_DIM_NONE, _lib.LSE_ONE_DIM_LEARNED, _lib.LSE_ONE_DIM_GRAY
LOG, ENERF = _lib.LSE_EVLOSS_LOG, _lib.LSE_EVLOSS_ENERF_NORM

# name -> (LSENeRFModelConfig keywords, the descriptor ops.loss_epilogue takes:
#          (rgb_mapped, rgb_mapper, evs_mapper, ev_one_dim, deblur_group, evs_loss_weight, event_loss_kind))
# The CPU tier holds every tuple against LSENeRFModel(cfg)._epilogue_desc()[0].
CLOSED_FORM: Dict[str, Tuple[dict, tuple]] = {
    "co_map_powpow_learned": (dict(use_mapping=True, mapping_method="powpow", map_mode="co_map", evs_mapping_method="powpow",
                                   ev_one_dim="learned"), (1, POWPOW, POWPOW, LEARNED, 1, 1.0, LOG)),
    "evs_rgb_gt_gray": (dict(use_mapping=True, mapping_method="gt", map_mode="evs_rgb", ev_one_dim="gt"),
                        (1, GT, ID, GRAY, 1, 1.0, LOG)),
    "rgb_evs_powpow": (dict(use_mapping=True, mapping_method="powpow", map_mode="rgb_evs", ev_one_dim=False),
                       (0, ID, POWPOW, NONE, 1, 1.0, LOG)),
    "plain_rgb_key": (dict(use_mapping=False, ev_one_dim=False, evs_loss_weight=0.7), (0, ID, ID, NONE, 1, 0.7, LOG)),
    "deblur_co_map": (dict(use_mapping=True, mapping_method="identity", map_mode="co_map", evs_mapping_method="gt", ev_one_dim="learned",
                           rgb_loss_type="deblur"), (1, ID, GT, LEARNED, 4, 1.0, LOG)),
}
MLP_PAIR: Dict[str, Tuple[dict, tuple]] = {
    "co_map_rgb_mlp_mlp_learned": (dict(use_mapping=True, mapping_method="rgb_mlp", map_mode="co_map", evs_mapping_method="mlp",
                                        ev_one_dim="learned"), (1, RGB_MLP, MLP, LEARNED, 1, 1.0, LOG)),
    "co_map_powpow_rgb_mlp_events": (dict(use_mapping=True, mapping_method="powpow", map_mode="co_map", evs_mapping_method="rgb_mlp",
                                          ev_one_dim=False), (1, POWPOW, RGB_MLP, NONE, 1, 1.0, LOG)),
    "deblur_evs_rgb_rgb_mlp_gray": (dict(use_mapping=True, mapping_method="rgb_mlp", map_mode="evs_rgb", ev_one_dim="gt",
                                         rgb_loss_type="deblur"), (1, RGB_MLP, ID, GRAY, 4, 1.0, LOG)),
    "enerf_co_map_powpow_learned": (dict(use_mapping=True, mapping_method="powpow", map_mode="co_map", evs_mapping_method="powpow",
                                         ev_one_dim="learned", event_loss_type="enerf_norm_loss", evs_loss_weight=3.0),
                                    (1, POWPOW, POWPOW, LEARNED, 1, 3.0, ENERF)),
    "enerf_co_map_rgb_mlp_mlp_learned": (dict(use_mapping=True, mapping_method="rgb_mlp", map_mode="co_map", evs_mapping_method="mlp",
                                              ev_one_dim="learned", event_loss_type="enerf_norm_loss"),
                                         (1, RGB_MLP, MLP, LEARNED, 1, 1.0, ENERF)),
    "enerf_deblur_co_map": (dict(use_mapping=True, mapping_method="identity", map_mode="co_map", evs_mapping_method="gt",
                                 ev_one_dim="learned", rgb_loss_type="deblur", event_loss_type="enerf_norm_loss"),
                            (1, ID, GT, LEARNED, 4, 1.0, ENERF)),
}
DESCRIPTORS: Dict[str, Tuple[dict, tuple]] = {**CLOSED_FORM, **MLP_PAIR}

# ---------------------------------------------------------------------------------------------------- ray counts
# (n_col, n_ev) with the two sides in different classes of the loop they run: below one wave {1, 63}, a partial last wave
# {65, 341, 342, 1023 | 511}, exactly one block {1024 | 512} (64: exactly one wave), one block + 1 {1025 | 513}, several trips
# {2316, 4099 | 1025, 2316}.  The closed-form kernels are 1024 threads wide and their colour loop runs over n_col * 3 (341 -> 1023,
# 342 -> 1026); the MLP backward is 512 threads wide.  (2316, 597) is the training batch.
CLOSED_FORM_SIZES = ((1, 1025), (63, 1024), (64, 2316), (65, 4099), (341, 63), (342, 1), (1023, 64), (1024, 65), (1025, 341),
                     (2316, 597), (4099, 342), (63, 1023))
# with deblur_group 4 the colour bundle holds n_col * 4 rays and the loops run over pixels: 878 pixels, the deblur training batch,
# are several trips of either kernel pair
CLOSED_FORM_DEBLUR_SIZES = ((1, 1025), (129, 1024), (878, 597), (341, 63), (342, 1), (1024, 65), (1025, 2316))
MLP_SIZES = ((1, 513), (63, 512), (65, 2316), (511, 1), (512, 63), (513, 65), (1025, 511), (2316, 597))
MLP_DEBLUR_SIZES = ((1, 513), (129, 512), (878, 597), (511, 1), (512, 63), (513, 2316))
SMALLEST_ENERF_N_EV = 2         # with one event ray delta / ||delta|| is +-1 whatever the rays hold: the loss is constant in them

CLASSES_CLOSED = {"below_wave": (1, 63), "partial_wave": (65, 341, 342, 1023, 597, 129), "one_block": (1024,),
                  "block_plus_1": (1025,), "several_trips": (2316, 4099, 878)}
CLASSES_MLP = {"below_wave": (1, 2, 63), "partial_wave": (65, 511, 129, 597), "one_block": (512,), "block_plus_1": (513,),
               "several_trips": (1025, 2316, 878)}


def sizes_of(name: str):
    """The committed (n_col, n_ev) of descriptor ``name``."""
    fields = DESCRIPTORS[name][1]
    deblur = fields[4] > 1
    if name in CLOSED_FORM:
        sizes = CLOSED_FORM_DEBLUR_SIZES if deblur else CLOSED_FORM_SIZES
    else:
        sizes = MLP_DEBLUR_SIZES if deblur else MLP_SIZES
    if fields[6] == ENERF:
        sizes = tuple((c, max(e, SMALLEST_ENERF_N_EV)) for c, e in sizes)
    return sizes


# (name, n_col, n_ev, seed, variant): everything both tiers run.  ``variant`` "flat": previous == next on every event ray.
# A combination whose float32 CPU evaluation misses a quarter of a bound is moved to the nearest seed that meets it and named here.
MOVED_SEEDS: Dict[Tuple[str, int, int], int] = {
    # one event ray: the loss is ONE squared difference, here 3.9e-5 = (6e-3)^2, and an ulp of the two logarithms is 3e-6 of it
    ("co_map_powpow_rgb_mlp_events", 511, 1): 1,
    # two event rays, nearly parallel to their targets: d_prev at 0.40 of its bound in float32 torch
    ("enerf_co_map_rgb_mlp_mlp_learned", 511, 2): 1,
}


def all_cases() -> List[tuple]:
    out = []
    for name in DESCRIPTORS:
        for n_col, n_ev in sizes_of(name):
            out.append((name, n_col, n_ev, MOVED_SEEDS.get((name, n_col, n_ev), 0), ""))
    out.append(("enerf_co_map_rgb_mlp_mlp_learned", 65, 513, 0, "flat"))
    return out


def case_id(case) -> str:
    name, n_col, n_ev, seed, variant = case
    return f"{name}-{n_col}-{n_ev}-s{seed}" + (f"-{variant}" if variant else "")


# ---------------------------------------------------------------------------------------------------- inputs
CLAMP_F32 = float(np.float32(1e-5))
BELOW_CLAMP_F32 = float(np.nextafter(np.float32(1e-5), np.float32(0)))
UPSTREAM = (1.3, 0.6)


def _mlp_params(in_dim: int, g: torch.Generator) -> List[torch.Tensor]:
    """Weights of one MLP mapper drawn so that, over inputs in [1e-5, 1.2], every hidden layer has ReLUs on both sides and the
    sigmoid stays away from saturation (the CPU tier counts the gates): the first layer's kinks lie inside the input range, and the
    later layers' biases put the pre-activations of a mid-grey input around zero."""
    w0 = torch.rand(16, in_dim, generator=g) * 3.0 - 1.5
    b0 = -(w0.sum(-1)) * (0.1 + 0.8 * torch.rand(16, generator=g))
    out, h = [w0, b0], torch.relu(w0.sum(-1) * 0.5 + b0)
    for _ in range(2):
        w = torch.randn(16, 16, generator=g) * 0.5
        b = -(w @ h) + torch.randn(16, generator=g) * 0.15
        out += [w, b]
        h = torch.relu(w @ h + b)
    out += [torch.randn(in_dim, 16, generator=g) * 0.25, torch.randn(in_dim, generator=g) * 0.2]
    return [t.float().contiguous() for t in out]


EDGE_ROWS = ((0.0, 0.0, 0.0), (CLAMP_F32,) * 3, (BELOW_CLAMP_F32,) * 3, (1.04, 1.18, 1.11), (0.0, CLAMP_F32, 0.5),
             (BELOW_CLAMP_F32, 0.7, CLAMP_F32), (-0.02, -0.02, 0.3))
# under enerf_norm_loss the next-event bundle holds, in the rows where the previous one holds EDGE_ROWS[i], EDGE_ROWS[PARTNER[i]]: the three rows that are
# clamped in every channel face one another, so that those rays' log-intensity change is exactly 0 instead of log(1e5).  (Under
# enerf_norm_loss dL/d delta_r is the difference of two terms that each grow with delta_r; on a ray whose delta is twenty times the
# others' float32 torch itself loses two digits there, the CPU tier showed.)
PARTNER = (1, 2, 0, 3, 5, 6, 4)


def _edge_rows(t: torch.Tensor, g: torch.Generator, keep_last: int = 1, where=None, partner: bool = False):
    """Overwrite seeded rows of ``t`` [n, 3] with the clamp's edges; returns (the mask of the rows left as drawn, the rows chosen).
    The last ``keep_last`` rows are never touched (the comparison's mutations zero the last ray's gradient: it has to be a live
    one), and a tensor of fewer than three free rows keeps all of them as drawn."""
    n = t.shape[0]
    plain = torch.ones(n, dtype=torch.bool)
    free = n - keep_last
    if free < 3:
        return plain, []
    if where is None:
        where = torch.randperm(free, generator=g)[:len(EDGE_ROWS)].tolist()
        if free > 1100 and len(where) >= 4:         # one edge row behind the first 1024 (a second trip of the stride loop)
            where[1] = 1024 + where[1] % (free - 1024)
            where = list(dict.fromkeys(where))
    for i, idx in enumerate(where):
        t[idx] = torch.tensor(EDGE_ROWS[PARTNER[i] if partner else i])
        plain[idx] = False
    return plain, where


@functools.lru_cache(maxsize=None)
def make_inputs(name: str, n_col: int, n_ev: int, seed: int = 0, variant: str = "") -> dict:
    """float32 CPU inputs of one case.  Radiance in [-0.02, 1.18] (below the clamp at 1e-5 up to above 1), rows forced to 0, to
    exactly float32(1e-5), to the float just below it and above 1, rows with the channels on different sides of the clamp, deblur
    groups whose members straddle the clamp (one member above and three below; all four below -- the mappers clamp every member
    before the mean, so the group mean of a mapped descriptor lands ON 1e-5 there, not below it), per-ray ``e_thresh``.
    ``plain_*``: the rows left as drawn."""
    fields = DESCRIPTORS[name][1]
    G = fields[4]
    g = torch.Generator().manual_seed(7919 * seed + 31 * n_col + n_ev + sum(map(ord, name)))
    draw = lambda n: (torch.rand(n, 3, generator=g) * 1.2 - 0.02).float()
    inp = {"col": draw(n_col * G), "prev": draw(n_ev), "next": draw(n_ev)}
    inp["plain_col"], _ = _edge_rows(inp["col"], g, keep_last=G)
    inp["plain_prev"], where = _edge_rows(inp["prev"], g)
    if variant == "flat":
        inp["next"] = inp["prev"].clone()
        inp["plain_next"] = inp["plain_prev"].clone()
    elif fields[6] == ENERF:
        inp["plain_next"], _ = _edge_rows(inp["next"], g, where=where, partner=True)
    else:                                       # log_loss: rows of their own, a clamped ray facing an ordinary one
        inp["plain_next"], _ = _edge_rows(inp["next"], g)
    if G > 1 and n_col >= 4:                      # straddling deblur groups: pixels 0 and 1 (never the last pixel)
        inp["col"][0:G] = torch.tensor([[3e-5, 0.4, 2e-5], [-0.02, 0.0, 5e-6], [BELOW_CLAMP_F32, -0.01, 0.0], [0.0, 1e-6, CLAMP_F32]])[:G]
        inp["col"][G:2 * G] = torch.tensor([[-0.02, 0.0, BELOW_CLAMP_F32]] * G)
        inp["plain_col"][:2 * G] = False
    inp["col_gt"] = torch.rand(n_col, 3, generator=g)
    inp["evs_gt"] = (torch.rand(n_ev, 1, generator=g) - 0.5) * 0.4
    inp["e_thresh"] = 0.15 + 0.1 * torch.rand(n_ev, 1, generator=g)
    inp["pow_rgb"] = torch.tensor([0.6])
    inp["pow_evs"] = torch.tensor([0.8])
    inp["w31"] = torch.tensor([[0.2, 0.5, 0.3]])
    gm = torch.Generator().manual_seed(104729 + seed)
    inp["mlp_rgb"] = _mlp_params(3, gm)
    inp["mlp_evs1"] = _mlp_params(1, gm)
    inp["mlp_evs3"] = _mlp_params(3, gm)
    return inp


def used_params(name: str, inp: dict) -> dict:
    """The parameters descriptor ``name`` reads, by the argument name of ops.loss_epilogue (absent: not passed)."""
    rgb_mapped, rk, ek, od, _, _, _ = DESCRIPTORS[name][1]
    out = {}
    if rgb_mapped and rk == POWPOW:
        out["pow_rgb"] = inp["pow_rgb"]
    if ek == POWPOW:
        out["pow_evs"] = inp["pow_evs"]
    if od == LEARNED:
        out["w31"] = inp["w31"]
    if rgb_mapped and rk == RGB_MLP:
        out["mlp_rgb"] = inp["mlp_rgb"]
    if ek == MLP:
        out["mlp_evs"] = inp["mlp_evs1"]
    elif ek == RGB_MLP:
        out["mlp_evs"] = inp["mlp_evs3"]
    return out


def as_dtype(t: torch.Tensor, dtype) -> torch.Tensor:
    """``t`` in ``dtype``; in float64, float32(1e-5) becomes the double 1e-5 (module docstring)."""
    out = t.to(dtype)
    if dtype == torch.float64:
        out = torch.where(t == CLAMP_F32, torch.full_like(out, 1e-5), out)
    return out.clone()


# ---------------------------------------------------------------------------------------------------- the reference
def _mapper(kind: int, pow_c, mlp):
    if kind == GT:
        return lambda x: x ** (1 / 2.4)
    if kind == POWPOW:
        return lambda x: x ** pow_c
    if kind in (MLP, RGB_MLP):
        return ol.mlp_mapper(mlp)
    return lambda x: x


def _event_out(fields, x, pow_evs, w31, mlp_evs):
    """"ev_out" of one event bundle by oracle.losses.route_outputs.  The fixed gray vector goes in front of the mapper through the
    oracle's own ``to_gray`` (three_to_one_w is a softmax, and softmax(log gray) would divide by the vector's sum, 0.9999)."""
    _, _, ek, od, _, _, _ = fields
    m = _mapper(ek, pow_evs, mlp_evs)
    evs_mapper = (lambda v: m(ol.to_gray(v))) if od == GRAY else m
    return ol.route_outputs(x, training=True, use_mapping=True, map_mode="co_map", ev_out=True, rgb_loss_type="linspace",
                            evs_mapper=evs_mapper, three_to_one_w=w31 if od == LEARNED else None)


def _delta(fields, prev, nxt, pow_evs, w31, mlp_evs):
    """The rays' log-intensity change, [n_ev] (what oracle.losses.log_loss / enerf_norm_loss take the MSE of)."""
    return _log_intensity(fields, nxt, pow_evs, w31, mlp_evs) - _log_intensity(fields, prev, pow_evs, w31, mlp_evs)


def _log_intensity(fields, x, pow_evs, w31, mlp_evs):
    """log(intensity + EPS) of one event bundle, [n_ev]: one of the two terms of ``_delta``."""
    v = _event_out(fields, x, pow_evs, w31, mlp_evs)["ev_out"]
    if v.shape[-1] != 1:
        v = ol.to_gray(v)
    return torch.log(v + ol.EPS).reshape(-1)


GRAD_KEYS = ("d_col", "d_prev", "d_next", "d_pow_rgb", "d_pow_evs", "d_w31")


def evaluate(name: str, inp: dict, dtype=torch.float64, with_scales: bool = False) -> dict:
    """oracle/losses.py on ``dtype`` tensors: {"rgb_loss", "event_loss", d_col, d_prev, d_next, d_pow_rgb, d_pow_evs, d_w31,
    d_mlp_rgb [8], d_mlp_evs [8]} for UPSTREAM; a key is None where the descriptor has no such parameter.  The colour loss reaches
    d_col / d_pow_rgb / d_mlp_rgb only and the event loss the rest, so the dictionary is also the reference of a one-bundle call and
    of a backward of one loss alone.  ``with_scales``: also "scale" = {key: sum_r |dL/d delta_r| |d delta_r / d theta|} for the
    event-side parameters (see ``compare``)."""
    fields = DESCRIPTORS[name][1]
    rgb_mapped, rk, ek, od, G, wgt, kind = fields
    used = used_params(name, inp)
    leaf = lambda t: as_dtype(t, dtype).requires_grad_(True)
    col, prev, nxt = leaf(inp["col"]), leaf(inp["prev"]), leaf(inp["next"])
    P = {k: ([leaf(t) for t in v] if isinstance(v, list) else leaf(v)) for k, v in used.items()}
    col_gt, evs_gt, e_thresh = (as_dtype(inp[k], dtype) for k in ("col_gt", "evs_gt", "e_thresh"))
    col_out = ol.route_outputs(col, training=True, use_mapping=bool(rgb_mapped), map_mode="evs_rgb", ev_out=False,
                               rgb_loss_type="deblur" if G > 1 else "linspace", rgb_mapper=_mapper(rk, P.get("pow_rgb"), P.get("mlp_rgb")))
    ev = lambda x: _event_out(fields, x, P.get("pow_evs"), P.get("w31"), P.get("mlp_evs"))
    losses = ol.loss_dict(col_out, ev(prev), ev(nxt), col_gt, evs_gt, use_mapping=True, evs_loss_weight=wgt,
                          event_loss="log_loss" if kind == LOG else "enerf_norm_loss", e_thresh=e_thresh)
    out = {"rgb_loss": losses["rgb_loss"].detach(), "event_loss": losses["event_loss"].detach()}
    flat = lambda keys: [t for k in keys if k in P for t in (P[k] if isinstance(P[k], list) else [P[k]])]
    rgb_leaves, ev_leaves = [col] + flat(("pow_rgb", "mlp_rgb")), [prev, nxt] + flat(("pow_evs", "w31", "mlp_evs"))
    g_rgb = torch.autograd.grad(losses["rgb_loss"] * UPSTREAM[0], rgb_leaves, allow_unused=True)
    g_ev = torch.autograd.grad(losses["event_loss"] * UPSTREAM[1], ev_leaves, allow_unused=True)
    z = lambda g, t: torch.zeros_like(t) if g is None else g
    g_rgb, g_ev = [z(g, t) for g, t in zip(g_rgb, rgb_leaves)], [z(g, t) for g, t in zip(g_ev, ev_leaves)]
    out.update(d_col=g_rgb.pop(0), d_prev=g_ev.pop(0), d_next=g_ev.pop(0))
    out["d_pow_rgb"] = g_rgb.pop(0) if "pow_rgb" in P else None
    out["d_mlp_rgb"] = [g_rgb.pop(0) for _ in range(8)] if "mlp_rgb" in P else None
    out["d_pow_evs"] = g_ev.pop(0) if "pow_evs" in P else None
    out["d_w31"] = g_ev.pop(0) if "w31" in P else None
    out["d_mlp_evs"] = [g_ev.pop(0) for _ in range(8)] if "mlp_evs" in P else None
    assert not g_rgb and not g_ev
    if with_scales and kind == ENERF:
        out["scale"] = _summand_scales(fields, prev.detach(), nxt.detach(), evs_gt, e_thresh,
                                       {k: P[k] for k in ("pow_evs", "w31", "mlp_evs") if k in P})
    return out


def _summand_scales(fields, prev, nxt, evs_gt, e_thresh, P: dict) -> dict:
    """sum_r |dL/d delta_r| * |d delta_r / d theta| in float64 for every event-side parameter theta: the scale of the terms whose
    sum the parameter's gradient is.  Under enerf_norm_loss the loss does not change when delta is scaled (but for the two EPS), so
    the gradient along every "scale delta" direction -- a powpow exponent, the last bias of a one-channel mapper -- is the residue
    of a cancelling sum, orders of magnitude below its terms; no float32 evaluation resolves the residue itself.
    Where previous == next on every ray, d delta_r / d theta is identically 0 -- the two logarithms' derivatives are the same
    numbers -- and so is that sum, while the terms an implementation adds up are the two logarithms' own: there, and only there,
    the scale is sum_r |dL/d delta_r| (|d log I_next,r / d theta| + |d log I_prev,r / d theta|).  (torch cancels the two exactly,
    one matrix product against its negative; a kernel that adds both bundles into one accumulator keeps a rounding residue,
    measured at 3e-9 of this scale.)"""
    wgt = fields[5]
    keys = list(P)
    tensors = [t.detach() for k in keys for t in (P[k] if isinstance(P[k], list) else [P[k]])]

    def unpack(ts):
        ts, d = list(ts), {}
        for k in keys:
            d[k] = [ts.pop(0) for _ in range(8)] if isinstance(P[k], list) else ts.pop(0)
        return d

    delta = _delta(fields, prev, nxt, P.get("pow_evs"), P.get("w31"), P.get("mlp_evs")).detach().requires_grad_(True)
    with torch.no_grad():
        tgt = (evs_gt / e_thresh).reshape(-1)
        tgt = tgt / (torch.linalg.norm(tgt) + ol.EPS)
    loss = UPSTREAM[1] * wgt * F.mse_loss(delta / (torch.linalg.norm(delta) + ol.EPS), tgt)
    g_delta, = torch.autograd.grad(loss, [delta])

    def one_ray(ts, p_row, n_row):
        d = unpack(ts)
        return _delta(fields, p_row[None], n_row[None], d.get("pow_evs"), d.get("w31"), d.get("mlp_evs"))[0]

    def one_chain(ts, row):
        d = unpack(ts)
        return _log_intensity(fields, row[None], d.get("pow_evs"), d.get("w31"), d.get("mlp_evs"))[0]

    if torch.equal(prev, nxt):
        jac = torch.func.vmap(torch.func.jacrev(one_chain, argnums=0), in_dims=(None, 0))(tuple(tensors), nxt)
        jac = [2.0 * j for j in jac]
    else:
        jac = torch.func.vmap(torch.func.jacrev(one_ray, argnums=0), in_dims=(None, 0, 0))(tuple(tensors), prev, nxt)
    scales = [(g_delta.abs().reshape((-1,) + (1,) * (j.dim() - 1)) * j.abs()).sum(0) for j in jac]
    d = unpack(scales)
    return {"d_" + k: v for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def reference(name: str, n_col: int, n_ev: int, seed: int = 0, variant: str = "") -> dict:
    """The float64 reference of one case: computed once per process, shared, never modified."""
    return evaluate(name, make_inputs(name, n_col, n_ev, seed, variant), torch.float64, with_scales=True)


# ---------------------------------------------------------------------------------------------------- the comparison
TOL_LOSS, TOL_RAY, TOL_PARAM, FLOOR = 1e-5, 1e-5, 1e-4, 1e-6
COLOUR_KEYS = ("rgb_loss", "d_col", "d_pow_rgb", "d_mlp_rgb")
EVENT_KEYS = ("event_loss", "d_prev", "d_next", "d_pow_evs", "d_w31", "d_mlp_evs")


def compare(got: dict, ref: dict, inp: dict, fraction: float = 1.0, keys=COLOUR_KEYS + EVENT_KEYS, do_assert: bool = True) -> Dict[str, float]:
    """``got`` (same keys as ``evaluate``; tensors anywhere, any float type) against the float64 ``ref``.  Bounds, those of
    test_fused_loss_epilogue_matches_torch_routing_and_oracle: losses 1e-5 relative; ray gradients 1e-5 of the tensor's maximum
    (floor 1e-6), on all rows AND on the rows left as drawn by themselves (a row forced to exactly 1e-5 has a gradient 1e4 times
    the others': on its scale alone a wrong gradient of an ordinary ray would pass); parameter gradients 1e-4 of the tensor's
    maximum (floor 1e-6) -- but where ``ref`` carries a summand scale for the tensor (event-side parameters under enerf_norm_loss)
    1e-4 of the maximum of that scale.  ``fraction`` scales every bound (the CPU tier holds float32 torch to a quarter).
    Returns the figures (error / bound per key: all must stay below ``fraction``); asserts unless told not to."""
    res: Dict[str, float] = {}
    for k in ("rgb_loss", "event_loss"):
        if k in keys:
            r = float(ref[k])
            res[k] = abs(float(got[k]) - r) / max(abs(r), 1e-30) / TOL_LOSS
    for k in ("d_col", "d_prev", "d_next"):
        if k in keys:
            assert got[k] is not None and tuple(got[k].shape) == tuple(ref[k].shape), k
            assert bool(torch.isfinite(got[k]).all()), k
            res[k] = nmax_err(got[k], ref[k], FLOOR) / TOL_RAY
            plain = inp["plain_" + k[2:]]
            if bool(plain.any()):
                res[k + "_plain"] = nmax_err(got[k].detach().cpu()[plain], ref[k][plain], FLOOR) / TOL_RAY
    scale = ref.get("scale", {})

    def param(key, g, r, s):
        assert g is not None and tuple(g.shape) == tuple(r.shape), key
        assert bool(torch.isfinite(g).all()), key
        if s is None:
            return nmax_err(g, r, FLOOR) / TOL_PARAM
        err = float((g.detach().double().cpu() - r).abs().max())
        return err / max(FLOOR, float(s.max())) / TOL_PARAM

    for k in ("d_pow_rgb", "d_pow_evs", "d_w31"):
        if k in keys and ref[k] is not None:
            res[k] = param(k, got[k], ref[k], scale.get(k))
    for k in ("d_mlp_rgb", "d_mlp_evs"):
        if k in keys and ref[k] is not None:
            assert got[k] is not None and len(got[k]) == 8, k
            for i in range(8):
                res[f"{k}{i}"] = param(f"{k}{i}", got[k][i], ref[k][i], scale[k][i] if k in scale else None)
    if do_assert:
        bad = {k: v for k, v in res.items() if not v < fraction}
        assert not bad, (bad, res)
    return res


def worst(res: Dict[str, float]) -> Tuple[str, float]:
    k = max(res, key=res.get)
    return k, res[k]


# ---------------------------------------------------------------------------------------------------- mutated copies of the reference
def _copy(ref: dict) -> dict:
    return {k: ([t.clone() for t in v] if isinstance(v, list) else (v.clone() if torch.is_tensor(v) else v)) for k, v in ref.items()
            if k != "scale"}


def mutation_last_ray_zeroed(ref: dict, key: str) -> dict:
    """(a) the last ray never got its gradient (a loop that stops one short)."""
    m = _copy(ref)
    m[key][-1] = 0.0
    return m


def mutation_second_trip_repeats_first(ref: dict, key: str) -> dict:
    """(b) the rows >= 1024 of a ray gradient are those of row - 1024 (a stride loop that forgets to advance its read index)."""
    m = _copy(ref)
    assert m[key].shape[0] > 1024
    m[key][1024:] = ref[key][:m[key].shape[0] - 1024]
    return m


def mutation_mlp_tile_scaled(ref: dict, key: str, layer: int) -> dict:
    """(c) one 16 x 16 weight-gradient tile lost one of a wave's 64 rays per step: scaled by 63 / 64."""
    m = _copy(ref)
    m[key][2 * layer] = m[key][2 * layer] * (63.0 / 64.0)
    return m


def mutation_loss_over_n_minus_1(ref: dict, key: str, n: int) -> dict:
    """(d) the loss divided by n - 1 instead of n."""
    m = _copy(ref)
    m[key] = m[key] * (n / (n - 1.0))
    return m
