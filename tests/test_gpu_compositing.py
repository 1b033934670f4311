"""The per-ray compositing chain (csrc/volrend.hip) at the densities of a TRAINED scene: sigma = scale * exp(h) has no clamp in the
forward, so surfaces carry sigma = 1e3 .. e^15 and beyond next to sigma ~ 0 in the same ray.  Every entry point is held against
the float64 per-ray reference of tests/util.py (composite_ref; gradients from float64 autograd) on seeded rays from
tests/util.trained_scene_rays.  tests/test_compositing_ref_cpu.py shows that a float32 kernel taking its exclusive prefix by lane
shift meets every bound asserted here with a factor 4 to spare.  sigma = inf with dt = 0 is NaN in the reference too (inf * 0) and
is not generated.  Every test prints its figures (`COMPOSITING ...` lines) before it asserts."""
import itertools
import math

import pytest
import torch

from tests.util import (SURFACE_SIGMAS, TOL_FWD, TOL_GRAD, TOL_GRAD_BLOCK, blockwise_nmax_err, composite_ref, emulated_per_ray_grad_error,
                        nmax_err, ray_bounds, rel_l2, select_rays, trained_scene_rays, visibility_ref)

pytestmark = pytest.mark.gpu

STEPS = ("const", "cone")
ONSETS = ("abrupt", "ramp")
STRIDES = (3, 4, 16)
FINITE_GRAD_SIGMAS = tuple(s for s in SURFACE_SIGMAS if s <= 1e10)      # e^15 is the largest the training backward sees; 1e10 beyond it
EPS = 1e-4      # early_stop_eps of the visibility pre-pass


def _ops():
    from lsenerf_amd import ops
    return ops


def _stride(sigma, step, onset):
    return STRIDES[(SURFACE_SIGMAS.index(sigma) + STEPS.index(step) + ONSETS.index(onset)) % 3]


def _cuda(inp):
    return {k: v.cuda() for k, v in inp.items()}


def _args(d, rgb=True):
    return (d["ts"], d["te"], d["sigma"], d["rgb"], d["packed_info"]) if rgb else (d["ts"], d["te"], d["sigma"], d["packed_info"])


def _eval_composite(d, nan_to_num=False, background=None, clamp=False):
    R = d["packed_info"].shape[0]
    o = {"rgb": torch.full((R, 3), math.nan, device="cuda"), "acc": torch.full((R,), math.nan, device="cuda"),
         "depth": torch.full((R,), math.nan, device="cuda"), "ns": torch.full((R,), -1, dtype=torch.int64, device="cuda")}
    _ops().eval_composite(*_args(d), o["rgb"], o["acc"], o["depth"], o["ns"], nan_to_num, background, clamp)
    return o


@torch.no_grad()
def _forward(d):
    """Every forward entry point on the same (GPU) inputs -> {name: tensor}."""
    ops = _ops()
    out = {}
    out["vr.rgb"], out["vr.acc"], out["vr.num"], out["vr.weights"] = ops.volume_render(*_args(d))
    out["vrd.rgb"], out["vrd.acc"], out["vrd.depth"], out["vrd.weights"] = ops.volume_render_depth(*_args(d))
    out["rw.weights"], out["rw.trans"], out["rw.alphas"] = ops.render_weight_from_density(*_args(d, rgb=False))
    ec = _eval_composite(d)
    out["ec.rgb"], out["ec.acc"], out["ec.depth"], out["ec.ns"] = ec["rgb"], ec["acc"], ec["depth"], ec["ns"]
    return out


def _forward_errors(out, ref, packed):
    """{name: (nmax_err, per-ray blockwise error)} of every float output against the float64 reference."""
    R = packed.shape[0]
    per_sample, per_ray1, per_ray3 = ray_bounds(packed), list(range(R + 1)), [3 * r for r in range(R + 1)]
    res = {}
    for name, got in out.items():
        if name == "ec.ns":
            continue
        key = name.split(".")[1]
        bounds = per_sample if key in ("weights", "trans", "alphas") else (per_ray3 if key == "rgb" else per_ray1)
        res[name] = (nmax_err(got, ref[key]), blockwise_nmax_err(got, ref[key], bounds))
    return res


def _worst(errs):
    name = max(errs, key=lambda k: (math.inf if math.isnan(errs[k][0]) else errs[k][0]))
    nameb = max(errs, key=lambda k: (math.inf if math.isnan(errs[k][1]) else errs[k][1]))
    return f"nmax={errs[name][0]:.3e} ({name}) per_ray={errs[nameb][1]:.3e} ({nameb})"


def _isolation_equal(out_all, out_sub, keep, inp, ref_all, ref_sub):
    """Rays marked ``keep`` give the same bits in the full call and in the call without the other rays.  The depth of a ray on
    which the global clip is active depends on the other rays by definition: compared where the clip is inactive in both calls."""
    keep_s = keep[inp["ray_indices"]].cuda()
    keep_r = keep.cuda()
    (lo_a, hi_a), (lo_s, hi_s) = ref_all["range"], ref_sub["range"]
    raw = ref_sub["depth_raw"]
    m = 1e-4
    inner = ((raw > max(lo_a, lo_s) * (1 + m)) & (raw < min(hi_a, hi_s) * (1 - m))).cuda()
    bad = []
    for name, full in out_all.items():
        sel = full[keep_s] if name.split(".")[1] in ("weights", "trans", "alphas") else full[keep_r]
        sub = out_sub[name]
        if name.endswith(".depth"):
            sel, sub = sel[inner], sub[inner]
        if not torch.equal(sel, sub):
            bad.append(name)
    return bad


# ------------------------------------------------------------------------------------------------ 2. forward
@pytest.mark.parametrize("onset", ONSETS)
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("sigma", SURFACE_SIGMAS)
def test_forward_all_entry_points(sigma, step, onset):
    """volume_render, volume_render_depth, render_weight_from_density and eval_composite against the float64 reference:
    nmax_err < TOL_FWD over everything and < 5 TOL_FWD per ray, finite at every sigma (1e10, 3e38 and inf included: nerfacc's
    exclusive sum gives the infinite sample w = T and 0 behind it); at those three, rays without such a sample are bit-identical to
    the call without the offending rays."""
    inp = trained_scene_rays(sigma, seed=1, step=step, onset=onset, rgb_stride=_stride(sigma, step, onset))
    ref = composite_ref(inp["ts"], inp["te"], inp["sigma"], inp["packed_info"], inp["rgb"])
    d = _cuda(inp)
    out = _forward(d)
    errs = _forward_errors(out, ref, inp["packed_info"])
    print(f"COMPOSITING fwd sigma={sigma:.4g} step={step} onset={onset} {_worst(errs)}")
    assert torch.equal(out["ec.ns"].cpu(), inp["packed_info"][:, 1])
    for name, got in out.items():
        assert bool(torch.isfinite(got.float()).all()), f"{name}: {int((~torch.isfinite(got)).sum())} non-finite values"
    for name, (e, eb) in errs.items():
        assert e < TOL_FWD and eb < 5 * TOL_FWD, (name, e, eb)
    if sigma >= 1e10:
        keep = ~inp["has_surface"]
        sub = select_rays(inp, keep)
        ref_sub = composite_ref(sub["ts"], sub["te"], sub["sigma"], sub["packed_info"], sub["rgb"])
        bad = _isolation_equal(out, _forward(_cuda(sub)), keep, inp, ref, ref_sub)
        assert not bad, f"rays without a sigma={sigma:g} sample depend on the rays that have one: {bad}"


# ------------------------------------------------------------------------------------------------ 3. backward
UPSTREAMS = {"rgb": (True, False, False), "acc": (False, True, False), "depth": (False, False, True), "all": (True, True, True)}


def _upstream(R, seed=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(R, 3, generator=g), torch.randn(R, generator=g), torch.randn(R, generator=g)


def _loss(rgb, acc, dep, use, a, b, c):
    terms = [(rgb * a).sum()] * use[0] + [(acc * b).sum()] * use[1] + [(dep * c).sum()] * use[2]
    return sum(terms[1:], terms[0])


def _gpu_grads(entry, d, use, up):
    """(d_sigma, d_rgb) of ops.<entry>; outputs outside ``use`` take no part in the loss, so their upstream gradient is None."""
    sg, cg = d["sigma"].clone().requires_grad_(True), d["rgb"].clone().requires_grad_(True)
    rgb, acc, dep, _ = getattr(_ops(), entry)(d["ts"], d["te"], sg, cg, d["packed_info"])
    _loss(rgb, acc, dep, use, *(t.cuda() for t in up)).backward()
    return sg.grad, (cg.grad if cg.grad is not None else torch.zeros_like(cg))


def _ref_grads(entry, inp, use, up):
    sg, cg = inp["sigma"].double().requires_grad_(True), inp["rgb"].double().requires_grad_(True)
    ref = composite_ref(inp["ts"], inp["te"], sg, inp["packed_info"], cg)
    _loss(ref["rgb"], ref["acc"], ref["depth" if entry == "volume_render_depth" else "num"], use, *(t.double() for t in up)).backward()
    return sg.grad, (cg.grad if cg.grad is not None else torch.zeros_like(cg))


def _grad_errors(got, ref, bounds):
    return nmax_err(got, ref, 1e-12), rel_l2(got, ref), blockwise_nmax_err(got, ref, bounds)


def _per_ray_bound(entry, inp, use, up, ref_d_sigma):
    """Per-ray bound on d_sigma: TOL_GRAD_BLOCK, except where float32 itself cannot hold it.  The backward stores no transmittance;
    it forms T_{k+1} = (1 - sum w) + sum_{i>k} w_i and d_sd_k = dw_k T_{k+1} - sum_{i>k} dw_i w_i.  On an opaque ray the true T_end
    is ~ 0, but 1 - sum w in float32 is 0 or +-2^-24 by the last bits of the forward's expf, and d_sd_k inherits dw_k times that:
    * a gradient on the accumulation gives every sample the same dw = g_acc, the true g_acc T_end vanishes and what is left is the
      rounding noise of two sums of size g_acc;
    * a gradient on the depth gives dw_k = g_d mid_k, up to 190 g_d at the far end of a 2000-sample cone-step ray, where the
      reference's d_sigma is ~ 0: measured 8.2e-3 of the per-ray scale (1e-4 of the call's largest gradient) on its last sample,
      reproduced to three digits by the emulated recurrence fed with the device's weights (sum w = 1 - 2^-24 there, 1 + 2^-24 with
      numpy's exp).
    So the bound is 4 x the worst per-ray error of the float32 emulation of the same recurrence on the same inputs over t_end
    shifts of 0 and +-2^-24 (tests/util.emulated_per_ray_grad_error), never less than TOL_GRAD_BLOCK.
    tests/test_compositing_ref_cpu.py::test_f32_emulation_of_the_backward records that figure per upstream combination.
    nmax_err and rel_l2 keep TOL_GRAD everywhere."""
    emu = emulated_per_ray_grad_error(inp, entry == "volume_render_depth", ref_d_sigma, *(t if u else None for t, u in zip(up, use)))
    return max(TOL_GRAD_BLOCK, 4 * emu)


@pytest.mark.parametrize("onset", ONSETS)
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("sigma", FINITE_GRAD_SIGMAS)
def test_backward_against_float64_autograd(sigma, step, onset):
    """d_sigma and d_rgb of volume_render / volume_render_depth for upstream gradients on rgb, accumulation and depth, each alone
    (the others None) and together: nmax_err and rel_l2 < TOL_GRAD, per ray < TOL_GRAD_BLOCK (d_sigma of the regimes that
    ``_per_ray_bound`` describes: 4 x the float32 emulation's error instead)."""
    stride = _stride(sigma, step, onset)
    inp = trained_scene_rays(sigma, seed=2, step=step, onset=onset, rgb_stride=stride)
    d = _cuda(inp)
    up = _upstream(inp["packed_info"].shape[0])
    bs, bc = ray_bounds(inp["packed_info"]), ray_bounds(inp["packed_info"], 3)
    res = {}
    for entry, (uname, use) in itertools.product(("volume_render", "volume_render_depth"), UPSTREAMS.items()):
        ds, dc = _gpu_grads(entry, d, use, up)
        rs, rc = _ref_grads(entry, inp, use, up)
        assert bool(torch.isfinite(ds).all()) and bool(torch.isfinite(dc).all()), (entry, uname, "non-finite gradient")
        if stride > 3:
            assert float(dc[:, 3:].abs().max()) == 0.0
        res[(entry, uname, "d_sigma")] = _grad_errors(ds, rs, bs) + (_per_ray_bound(entry, inp, use, up, rs),)
        res[(entry, uname, "d_rgb")] = _grad_errors(dc[:, :3], rc[:, :3], bc) + (TOL_GRAD_BLOCK,)
    w = [max(res, key=lambda k: res[k][i]) for i in range(2)] + [max(res, key=lambda k: res[k][2] / res[k][3])]
    strict = max(v[2] for v in res.values() if v[3] == TOL_GRAD_BLOCK)
    print(f"COMPOSITING bwd sigma={sigma:.4g} step={step} onset={onset} nmax={res[w[0]][0]:.3e} {w[0]} l2={res[w[1]][1]:.3e} {w[1]} "
          f"per_ray={strict:.3e} where the bound is TOL_GRAD_BLOCK; closest to its bound: {res[w[2]][2]:.3e} of {res[w[2]][3]:.3e} {w[2]}")
    for k, (e, l2, eb, bound) in res.items():
        assert e < TOL_GRAD and l2 < TOL_GRAD and eb < bound, (k, e, l2, eb, bound)


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("sigma", FINITE_GRAD_SIGMAS)
def test_render_weight_backward(sigma, step):
    """d_sigma of render_weight_from_density for a random per-sample d_weights (lse_render_weight_bwd)."""
    onset = ONSETS[(SURFACE_SIGMAS.index(sigma) + STEPS.index(step)) % 2]
    inp = trained_scene_rays(sigma, seed=6, step=step, onset=onset)
    gw = torch.randn(inp["ts"].shape[0], generator=torch.Generator().manual_seed(8))
    sg = inp["sigma"].cuda().requires_grad_(True)
    w, _, _ = _ops().render_weight_from_density(inp["ts"].cuda(), inp["te"].cuda(), sg, inp["packed_info"].cuda())
    (w * gw.cuda()).sum().backward()
    sr = inp["sigma"].double().requires_grad_(True)
    (composite_ref(inp["ts"], inp["te"], sr, inp["packed_info"])["weights"] * gw.double()).sum().backward()
    e, l2, eb = _grad_errors(sg.grad, sr.grad, ray_bounds(inp["packed_info"]))
    print(f"COMPOSITING rw_bwd sigma={sigma:.4g} step={step} onset={onset} nmax={e:.3e} l2={l2:.3e} per_ray={eb:.3e}")
    assert e < TOL_GRAD and l2 < TOL_GRAD and eb < TOL_GRAD_BLOCK


@pytest.mark.parametrize("step", STEPS)
def test_backward_isolates_an_infinite_ray(step):
    """sigma = inf on some rays: the other rays' gradients equal the float64 reference and, bit for bit, the run without the
    infinite rays; the infinite rays' own gradients are finite wherever the reference's are (everywhere: d alpha / d sd = exp(-inf))."""
    inp = trained_scene_rays(math.inf, seed=2, step=step, onset="abrupt", rgb_stride=4)
    keep = ~inp["has_surface"]
    sub = select_rays(inp, keep)
    up = _upstream(inp["packed_info"].shape[0])
    up_sub = tuple(t[keep] for t in up)
    ks = keep[inp["ray_indices"]]
    use = UPSTREAMS["all"]
    ds, dc = _gpu_grads("volume_render", _cuda(inp), use, up)
    ds_sub, dc_sub = _gpu_grads("volume_render", _cuda(sub), use, up_sub)
    rs, rc = _ref_grads("volume_render", inp, use, up)
    assert bool(torch.isfinite(rs).all()) and bool(torch.isfinite(rc).all())
    n_bad = int((~torch.isfinite(ds)).sum()) + int((~torch.isfinite(dc)).sum())
    es = _grad_errors(ds.cpu()[ks], rs[ks], ray_bounds(sub["packed_info"]))
    ec = _grad_errors(dc.cpu()[ks][:, :3], rc[ks][:, :3], ray_bounds(sub["packed_info"], 3))
    print(f"COMPOSITING bwd sigma=inf step={step} non_finite={n_bad} other_rays d_sigma={es} d_rgb={ec}")
    assert n_bad == 0, f"{n_bad} non-finite gradient values"
    assert torch.equal(ds[ks.cuda()], ds_sub) and torch.equal(dc[ks.cuda()], dc_sub)
    for e, l2, eb in (es, ec):
        assert e < TOL_GRAD and l2 < TOL_GRAD and eb < TOL_GRAD_BLOCK
    # depth epilogue included (its clip range is global, so no bitwise statement): still finite, other rays still right
    ds2, dc2 = _gpu_grads("volume_render_depth", _cuda(inp), use, up)
    rs2, _ = _ref_grads("volume_render_depth", inp, use, up)
    assert bool(torch.isfinite(ds2).all()) and bool(torch.isfinite(dc2).all())
    e, l2, eb = _grad_errors(ds2.cpu()[ks], rs2[ks], ray_bounds(sub["packed_info"]))
    assert e < TOL_GRAD and l2 < TOL_GRAD and eb < TOL_GRAD_BLOCK, (e, l2, eb)


# ------------------------------------------------------------------------------------------------ 4. eval_composite
@pytest.mark.parametrize("sigma,step,onset", [(30.0, "const", "abrupt"), (1e5, "cone", "ramp"), (math.exp(15.0), "const", "ramp"),
                                              (math.inf, "cone", "abrupt")])
def test_eval_composite_equals_render_plus_epilogue_bitwise(sigma, step, onset):
    """lse_eval_composite == volume_render_depth + the epilogue of LSENeRFModel.render_packed (nan_to_num of the colours, background
    blend, clamp), bit for bit, for all 8 flag combinations and background 0, 0.5, 1."""
    ops = _ops()
    for stride in STRIDES:
        d = _cuda(trained_scene_rays(sigma, seed=3, step=step, onset=onset, rgb_stride=stride))
        d["rgb"][::7, 0] = math.nan
        d["rgb"][3::11, 1] = 1.5
        d["rgb"][5::13, 2] = -0.5
        for fix, blend, clamp, bg in itertools.product((False, True), (False, True), (False, True), (0.0, 0.5, 1.0)):
            with torch.no_grad():
                rgb, acc, depth, _ = ops.volume_render_depth(d["ts"], d["te"], d["sigma"], torch.nan_to_num(d["rgb"]) if fix else d["rgb"],
                                                             d["packed_info"])
                if blend:
                    rgb = rgb + bg * (1.0 - acc[:, None])
                if clamp:
                    rgb = torch.clamp(rgb, 0.0, 1.0)
            ec = _eval_composite(d, fix, bg if blend else None, clamp)
            tag = (stride, fix, blend, clamp, bg)
            assert torch.equal(torch.isnan(ec["rgb"]), torch.isnan(rgb)), tag
            assert torch.equal(ec["rgb"].nan_to_num(nan=7.0).view(torch.int32), rgb.nan_to_num(nan=7.0).view(torch.int32)), tag
            assert torch.equal(ec["acc"], acc) and torch.equal(ec["depth"], depth), tag
            assert torch.equal(ec["ns"], d["packed_info"][:, 1]), tag


def test_eval_composite_special_colours():
    """NaN, +inf, -inf, < 0 and > 1 in the colours.  With nan_to_num the render is the float64 reference on torch.nan_to_num(rgb);
    without it a NaN reaches its own ray only; clamp keeps NaN as NaN (torch.clamp) and limits everything else to [0, 1]."""
    inp = trained_scene_rays(1e4, seed=4, step="const", onset="abrupt", rgb_stride=4)
    cnt = inp["packed_info"][:, 1]
    rays = [int(r) for r in torch.nonzero(cnt >= 3).flatten()[:5]]
    r_nan, r_pinf, r_ninf, r_neg, r_big = rays
    start = {r: int(inp["packed_info"][r, 0]) for r in rays}
    for r in (r_nan, r_pinf, r_ninf):
        inp["sigma"][start[r]] = 0.4          # the marked sample has a definite non-zero weight (w * inf, not 0 * inf)
        inp["sigma"][start[r] + 1:start[r] + int(cnt[r])].clamp_(max=0.5)
    inp["rgb"][start[r_nan], 0] = math.nan
    inp["rgb"][start[r_pinf], 1] = math.inf
    inp["rgb"][start[r_ninf], 2] = -math.inf
    inp["rgb"][start[r_neg]:start[r_neg] + int(cnt[r_neg])] = -0.75
    inp["rgb"][start[r_big]:start[r_big] + int(cnt[r_big])] = 2.5
    inp["sigma"][start[r_big]] = 1e4          # opaque: the composite really exceeds 1
    clean = torch.ones(cnt.shape[0], dtype=torch.bool)
    clean[rays] = False
    d = _cuda(inp)
    ref = composite_ref(inp["ts"], inp["te"], inp["sigma"], inp["packed_info"], torch.nan_to_num(inp["rgb"]))
    fixed = _eval_composite(d, nan_to_num=True)
    got, want = fixed["rgb"].cpu().double(), ref["rgb"]
    finite_rays = clean.clone()
    finite_rays[[r_nan, r_neg, r_big]] = True
    e = nmax_err(got[finite_rays], want[finite_rays])
    e_inf = float(((got - want)[[r_pinf, r_ninf]].abs() / want[[r_pinf, r_ninf]].abs().clamp_min(1.0)).max())
    print(f"COMPOSITING special colours nan_to_num: nmax={e:.3e} inf rays rel={e_inf:.3e}")
    assert bool(torch.isfinite(got).all()) and e < TOL_FWD and e_inf < TOL_FWD
    assert float(want[r_pinf, 1]) > 1e35 and float(want[r_ninf, 2]) < -1e35 and float(want[r_neg].max()) < 0 and float(want[r_big].min()) > 1
    assert nmax_err(fixed["acc"], ref["acc"]) < TOL_FWD
    raw = _eval_composite(d, nan_to_num=False)["rgb"].cpu()
    assert math.isnan(float(raw[r_nan, 0])) and float(raw[r_pinf, 1]) == math.inf and float(raw[r_ninf, 2]) == -math.inf
    assert bool(torch.isfinite(raw[r_nan, 1:]).all()) and bool(torch.isfinite(raw[r_pinf, [0, 2]]).all())
    assert torch.equal(raw[clean], fixed["rgb"].cpu()[clean]), "a NaN or an infinity left its own ray"
    assert torch.equal(raw[[r_neg, r_big]], fixed["rgb"].cpu()[[r_neg, r_big]])
    cl = _eval_composite(d, nan_to_num=False, clamp=True)["rgb"].cpu()
    assert math.isnan(float(cl[r_nan, 0])), "clamp must keep NaN (torch.clamp semantics)"
    assert float(cl[r_pinf, 1]) == 1.0 and float(cl[r_ninf, 2]) == 0.0
    assert torch.equal(cl[r_neg], torch.zeros(3)) and torch.equal(cl[r_big], torch.ones(3))
    rest = torch.ones_like(cl, dtype=torch.bool)
    rest[r_nan, 0] = False
    assert torch.equal(cl[rest], torch.clamp(raw, 0.0, 1.0)[rest])
    cf = _eval_composite(d, nan_to_num=True, clamp=True)["rgb"].cpu()
    assert torch.equal(cf, torch.clamp(fixed["rgb"].cpu(), 0.0, 1.0)) and float(cf.min()) == 0.0 and float(cf.max()) == 1.0


def _sized_case(n_rays, owner, seed):
    """``n_rays`` short rays in t = [0.5, 0.7] and one long ray ``owner`` that spans t = [0.02, 2.1]: it alone sets the global
    clip range.  Every third other ray has sigma == 0 throughout: acc == 0, raw depth 0, clipped up to the owner's first mid-point."""
    g = torch.Generator().manual_seed(seed)
    lengths = torch.randint(0, 24, (n_rays,), generator=g)
    t0 = 0.5 + 0.1 * torch.rand(n_rays, generator=g)
    lengths[owner], t0[owner] = 600, 0.02
    inp = trained_scene_rays(1e4, seed=seed, step="const", onset="abrupt", rgb_stride=4, lengths=lengths.tolist(), t0=t0.tolist())
    empty = (torch.arange(n_rays) % 3 == 0) & (torch.arange(n_rays) != owner)
    inp["sigma"][empty[inp["ray_indices"]]] = 0.0
    return inp, empty & (lengths > 0)


@pytest.mark.parametrize("n_rays", [1, 3, 4, 5, 1023, 1024, 1025, 4097])
def test_eval_composite_ray_counts_and_clip_owner(n_rays):
    """4 rays per workgroup in the composite, a 1024-thread strided loop and a 16-wave reduction in depth_finish_kernel: the global
    clip range comes from the first, a middle and the last ray in turn, and rays with acc == 0 show that it was found."""
    for owner in sorted({0, n_rays // 2, n_rays - 1}):
        inp, transparent = _sized_case(n_rays, owner, seed=n_rays + owner)
        ref = composite_ref(inp["ts"], inp["te"], inp["sigma"], inp["packed_info"], inp["rgb"])
        d = _cuda(inp)
        ec = _eval_composite(d)
        vrd = _ops().volume_render_depth(*_args(d))
        lo = (inp["ts"][inp["packed_info"][owner, 0]] + inp["te"][inp["packed_info"][owner, 0]]) * 0.5     # float32, as the kernel forms it
        assert abs(float(lo) - ref["range"][0]) < 1e-7
        R = n_rays
        errs = {k: (nmax_err(ec[k], ref[k]), blockwise_nmax_err(ec[k], ref[k], list(range(0, R * w + 1, w))))
                for k, w in (("rgb", 3), ("acc", 1), ("depth", 1))}
        print(f"COMPOSITING eval n_rays={n_rays} owner={owner} {errs}")
        assert torch.equal(ec["ns"].cpu(), inp["packed_info"][:, 1])
        for k, (e, eb) in errs.items():
            assert e < TOL_FWD and eb < 5 * TOL_FWD, (k, owner, e, eb)
        assert torch.equal(ec["depth"], vrd[2]) and torch.equal(ec["rgb"], vrd[0]) and torch.equal(ec["acc"], vrd[1])
        if bool(transparent.any()):
            assert bool((ec["depth"].cpu()[transparent] == lo).all()), "acc == 0 rays must sit on the global lower clip bound"
            assert float(ec["acc"].cpu()[transparent].abs().max()) == 0.0


def test_eval_composite_no_samples_at_all():
    """No ray has a sample: nerfstudio skips the clip (`steps` is empty), depth = 0 / (0 + 1e-10) = 0, the colour is the background.
    The sample arrays have capacity extent and hold NaN: nothing of them may be read."""
    R = 9
    d = {"ts": torch.full((128,), math.nan, device="cuda"), "te": torch.full((128,), math.nan, device="cuda"),
         "sigma": torch.full((128,), math.nan, device="cuda"), "rgb": torch.full((128, 4), math.nan, device="cuda"),
         "packed_info": torch.zeros(R, 2, dtype=torch.int64, device="cuda")}
    for bg in (None, 0.5):
        ec = _eval_composite(d, nan_to_num=False, background=bg, clamp=True)
        assert torch.equal(ec["rgb"], torch.full((R, 3), bg or 0.0, device="cuda"))
        assert torch.equal(ec["acc"], torch.zeros(R, device="cuda")) and torch.equal(ec["depth"], torch.zeros(R, device="cuda"))
        assert torch.equal(ec["ns"], torch.zeros(R, dtype=torch.int64, device="cuda"))
    with torch.no_grad():
        rgb, acc, depth, _ = _ops().volume_render_depth(*_args(d))
    assert float(rgb.abs().max()) == 0.0 and float(acc.abs().max()) == 0.0 and float(depth.abs().max()) == 0.0


@pytest.mark.parametrize("sigma", [1e3, math.inf])
def test_eval_composite_capacity_extent_and_row_block_views(sigma):
    """Sample arrays longer than the packed extents, NaN beyond: results unchanged.  Outputs that are row blocks of a larger image:
    the rows around them stay untouched."""
    inp = trained_scene_rays(sigma, seed=5, step="cone", onset="ramp", rgb_stride=4)
    d = _cuda(inp)
    want = _eval_composite(d, True, 1.0, True)
    pad = 777
    big = dict(d)
    for k in ("ts", "te", "sigma", "rgb"):
        big[k] = torch.cat([d[k], torch.full((pad,) + tuple(d[k].shape[1:]), math.nan, device="cuda")])
    R, margin = inp["packed_info"].shape[0], 10
    img = {"rgb": torch.full((R + 2 * margin, 3), 7.0, device="cuda"), "acc": torch.full((R + 2 * margin,), 7.0, device="cuda"),
           "depth": torch.full((R + 2 * margin,), 7.0, device="cuda"), "ns": torch.full((R + 2 * margin,), 7, dtype=torch.int64, device="cuda")}
    view = {k: v[margin:margin + R] for k, v in img.items()}
    _ops().eval_composite(*_args(big), view["rgb"], view["acc"], view["depth"], view["ns"], True, 1.0, True)
    for k in img:
        assert torch.equal(view[k], want[k]), k
        assert bool((img[k][:margin] == 7).all()) and bool((img[k][margin + R:] == 7).all()), f"{k}: rows outside the block were written"
    with torch.no_grad():
        a = _ops().volume_render_depth(*_args(d))
        b = _ops().volume_render_depth(*_args(big))
    n = d["ts"].shape[0]
    assert all(torch.equal(x[:n] if x.shape[0] == n + pad else x, y) for x, y in zip(b, a))


# ------------------------------------------------------------------------------------------------ 5. depth clip, pre-pass
def _clip_case():
    """Hand-made rays in front of generator rays: 0 -- one nearly transparent sample at the global minimum (w ~ 2.4e-7, so
    num / (acc + 1e-10) is 4e-4 (relative) below its mid-point: clip active at the lower bound); 1 -- one opaque sample at the global
    maximum (depth == hi: AT the bound, gradient passes as in torch.clip); 2 -- sigma == 0 (acc == 0, raw depth 0, clip active);
    3 -- no samples.  In exact arithmetic num / (acc + 1e-10) cannot exceed a ray's own largest mid-point; the upper clip can act only
    when float32 rounds the quotient one ulp above it, which no input controls, so an ACTIVE upper clip is not asserted."""
    base = trained_scene_rays(1e5, seed=7, step="const", onset="ramp", rgb_stride=3, n_random=20, max_random=100)
    ts = torch.tensor([0.01] + [400.0] + [1.0, 1.1, 1.2, 1.3, 1.4])
    te = torch.tensor([0.02] + [400.5] + [1.1, 1.2, 1.3, 1.4, 1.5])
    sg = torch.tensor([2.4e-5] + [1e6] + [0.0] * 5)
    cnt = torch.cat([torch.tensor([1, 1, 5, 0]), base["packed_info"][:, 1]])
    g = torch.Generator().manual_seed(1)
    inp = {"ts": torch.cat([ts, base["ts"]]), "te": torch.cat([te, base["te"]]), "sigma": torch.cat([sg, base["sigma"]]),
           "rgb": torch.cat([torch.rand(7, 3, generator=g), base["rgb"]]),
           "packed_info": torch.stack([torch.cumsum(cnt, 0) - cnt, cnt], -1).contiguous(),
           "ray_indices": torch.repeat_interleave(torch.arange(cnt.shape[0]), cnt)}
    assert float(base["ts"].min()) > 0.02 and float(base["te"].max()) < 400.0
    return inp


def test_depth_through_the_clip():
    """volume_render_depth forward and backward against the float64 restatement of DepthRenderer("expected"); the gradient is
    exactly zero on rays where the clip is active."""
    inp = _clip_case()
    d = _cuda(inp)
    ref = composite_ref(inp["ts"], inp["te"], inp["sigma"], inp["packed_info"], inp["rgb"])
    lo, hi = (inp["ts"][0] + inp["te"][0]) * 0.5, (inp["ts"][1] + inp["te"][1]) * 0.5
    assert float(ref["depth_raw"][0]) < ref["range"][0] * (1 - 1e-4) and float(ref["depth_raw"][2]) == 0.0
    with torch.no_grad():
        depth = _ops().volume_render_depth(*_args(d))[2].cpu()
    R = depth.shape[0]
    e, eb = nmax_err(depth, ref["depth"]), blockwise_nmax_err(depth, ref["depth"], list(range(R + 1)))
    print(f"COMPOSITING depth clip fwd nmax={e:.3e} per_ray={eb:.3e}")
    assert e < TOL_FWD and eb < 5 * TOL_FWD
    assert float(depth[0]) == float(lo) and float(depth[2]) == float(lo) and float(depth[1]) == float(hi) and float(depth[3]) == float(lo)
    up = _upstream(R)
    bs, bc = ray_bounds(inp["packed_info"]), ray_bounds(inp["packed_info"], 3)
    for uname in ("depth", "all"):
        ds, dc = _gpu_grads("volume_render_depth", d, UPSTREAMS[uname], up)
        rs, rc = _ref_grads("volume_render_depth", inp, UPSTREAMS[uname], up)
        es, ec = _grad_errors(ds, rs, bs), _grad_errors(dc, rc, bc)
        print(f"COMPOSITING depth clip bwd upstream={uname} d_sigma={es} d_rgb={ec}")
        for e, l2, eb in (es, ec):
            assert e < TOL_GRAD and l2 < TOL_GRAD and eb < TOL_GRAD_BLOCK, (uname, e, l2, eb)
        if uname == "depth":
            clipped = (inp["ray_indices"] == 0) | (inp["ray_indices"] == 2)
            assert float(rs[clipped].abs().max()) == 0.0
            assert float(ds.cpu()[clipped].abs().max()) == 0.0, "the gradient must vanish where the clip is active"


@pytest.mark.parametrize("alpha_thre", [0.0, 0.01])
@pytest.mark.parametrize("onset", ONSETS)
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("sigma", SURFACE_SIGMAS)
def test_visibility_prepass_and_render_agree(sigma, step, onset, alpha_thre):
    """visibility_compact against the float64 mask, samples within 1e-5 (relative) of a threshold left out (at most 0.2 % of the
    case, which tests/test_compositing_ref_cpu.py asserts of the reference); and every sample the pre-pass keeps is one the render
    calls visible: the transmittance render_weight_from_density reports for it is >= early_stop_eps (1 - 1e-4)."""
    inp = trained_scene_rays(sigma, seed=1, step=step, onset=onset)
    ref = composite_ref(inp["ts"], inp["te"], inp["sigma"], inp["packed_info"])
    vis, und = visibility_ref(ref, EPS, alpha_thre)
    assert float(und.float().mean()) <= 0.002
    d = _cuda(inp)
    ri32 = d["ray_indices"].int()
    o_ri, o_ts, o_te, new_packed, mask = _ops().visibility_compact(ri32, d["ts"], d["te"], d["sigma"], d["packed_info"], EPS, alpha_thre)
    mask = mask.bool()
    wrong = int((mask.cpu() != vis)[~und].sum())
    with torch.no_grad():
        trans = _ops().render_weight_from_density(*_args(d, rgb=False))[1]
    kept_T = trans[mask]
    print(f"COMPOSITING vis sigma={sigma:.4g} step={step} onset={onset} thre={alpha_thre} kept={int(mask.sum())}/{mask.numel()} "
          f"in_band={int(und.sum())} wrong={wrong} min_kept_T={float(kept_T.min()) if kept_T.numel() else math.nan:.6e} "
          f"nan_T={int(torch.isnan(kept_T).sum())}")
    assert wrong == 0
    assert torch.equal(o_ts, d["ts"][mask]) and torch.equal(o_te, d["te"][mask]) and torch.equal(o_ri, ri32[mask])
    cnt = torch.zeros(d["packed_info"].shape[0], dtype=torch.int64, device="cuda").index_add_(0, d["ray_indices"], mask.long())
    assert torch.equal(new_packed[:, 1], cnt)
    assert bool((kept_T >= EPS * (1 - 1e-4)).all()), "the pre-pass kept a sample the render considers invisible"
