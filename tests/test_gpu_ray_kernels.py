"""GPU tier of the per-ray and sampler bookkeeping kernel tests: every case of tests/ray_kernel_cases.py through ``ops`` (or through
``_lib.call`` where ``ops`` has no wrapper, or allocates an output that the test has to poison first), compared with the helpers
the CPU tier (tests/test_ray_kernel_cases_cpu.py) holds against float32 torch and against mutated references.

  exact integers / bitwise float32:  lse_pack_info_from_counts, lse_compact_ray_slots, lse_ray_planes, lse_fake_sample_if_empty,
                                     lse_visibility_mask, lse_visibility_mask_cap, lse_visibility_mask_alpha, lse_compact_samples
  bounded float32 against float64:   lse_ray_bias_fwd / lse_ray_bias_bwd (+ emb_grad_kernel), lse_ray_features_fwd / _bwd,
                                     lse_linear_fwd, lse_linear_bwd_input, lse_gemm_tn_acc, lse_segment_sum_rows,
                                     lse_density_fwd / lse_density_bwd, lse_positions_fwd / lse_positions_bwd

Every case prints one `RAYKERNEL ...` line with its worst error over its bound before it asserts."""
import ctypes
import math

import pytest
import torch

from tests import ray_kernel_cases as rk
from tests.test_ray_kernel_cases_cpu import ray_bias_preload
from tests.util import TOL_GRAD, per_ray_grad_check, row_bounds

pytestmark = pytest.mark.gpu


def _ops():
    from lsenerf_amd import ops
    return ops


def _lib():
    from lsenerf_amd import _lib
    return _lib


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _call(name, *args):
    _lib().call(name, *args, _ops()._stream())


def _dev(t):
    return None if t is None else t.detach().clone().cuda()


# ------------------------------------------------------------------------------------------------ integer kernels
@pytest.mark.parametrize("R", rk.PACK_R)
def test_pack_info_from_counts(R):
    """lse_pack_info_from_counts against torch.cumsum on int64; ``total`` and ``packed_info`` hold poison before every call (R = 0
    included): ``total`` comes back overwritten, not accumulated."""
    for pattern in rk.PACK_PATTERNS:
        cnts = rk.pack_counts(R, pattern)
        ref_packed, ref_total = rk.pack_reference(cnts)
        c = cnts.cuda()
        packed = torch.full((R, 2), rk.POISON_I64, dtype=torch.int64, device="cuda")
        total = torch.full((1,), rk.POISON_I64, dtype=torch.int64, device="cuda")
        _call("lse_pack_info_from_counts", P(c), R, P(packed), P(total))
        rk.assert_exact(packed, ref_packed, f"packed_info R={R} {pattern}")
        rk.assert_exact(total, ref_total, f"total R={R} {pattern}")
        p2, t2 = _ops().pack_info_from_counts(c)
        rk.assert_exact(p2, ref_packed, "ops.pack_info_from_counts")
        rk.assert_exact(t2, ref_total, "ops.pack_info_from_counts total")
    print(f"RAYKERNEL pack_info R={R}: {len(rk.PACK_PATTERNS)} count patterns, 0 integers differ")


@pytest.mark.parametrize("R", rk.SLOT_R)
def test_compact_ray_slots(R):
    """lse_compact_ray_slots: the packed prefix is the gather of each ray's first cnt slots (NaN behind them is never copied), and
    everything at or beyond the total keeps its poison."""
    for cap in rk.SLOT_CAP:
        inp = rk.slot_inputs(R, cap)
        C = inp["capacity"]
        assert inp["total"] <= R * cap < C and inp["ts_slots"].numel() == R * cap
        ts_s, te_s, packed = inp["ts_slots"].cuda(), inp["te_slots"].cuda(), inp["packed"].cuda()
        out = {"ray_indices": torch.full((C,), rk.POISON_I32, dtype=torch.int32, device="cuda"),
               "t_starts": torch.full((C,), rk.POISON_F32, device="cuda"), "t_ends": torch.full((C,), rk.POISON_F32, device="cuda")}
        _call("lse_compact_ray_slots", P(ts_s), P(te_s), cap, P(packed), R, P(out["ray_indices"]), P(out["t_starts"]), P(out["t_ends"]))
        rk.check_compacted(out, inp)
    print(f"RAYKERNEL compact_ray_slots R={R}: caps {rk.SLOT_CAP}, 0 elements differ")


@pytest.mark.parametrize("R", rk.PLANES_R)
def test_ray_planes(R):
    """lse_ray_planes (ops.ray_planes): bitwise float32 torch maximum / minimum / near + u * step as two roundings, for all 8
    present / absent combinations of t_min, t_max, jitter and inputs shaped [R] and [R, 1]."""
    inp = rk.planes_inputs(R)
    for has_min, has_max, has_jit in rk.PLANES_COMBOS:
        near_ref, far_ref = rk.planes_reference(inp, has_min, has_max, has_jit)
        for shape in ((R,), (R, 1)):
            arg = lambda k, has: inp[k].reshape(shape).cuda() if has else None      # noqa: E731
            near, far = _ops().ray_planes(R, "cuda", rk.PLANES_NEAR, rk.PLANES_FAR, arg("t_min", has_min), arg("t_max", has_max),
                                          arg("jitter", has_jit), rk.PLANES_STEP)
            assert near.shape == (R,) and far.shape == (R,)
            rk.assert_bitwise(near, near_ref, f"near {has_min, has_max, has_jit} {shape}")
            rk.assert_bitwise(far, far_ref, f"far {has_min, has_max, has_jit} {shape}")
    print(f"RAYKERNEL ray_planes R={R}: 8 combinations x 2 shapes, 0 floats differ in their bits")


@pytest.mark.parametrize("levels,features", rk.FAKE_SHAPES)
def test_fake_sample_if_empty(levels, features):
    """lse_fake_sample_if_empty called directly: n_dev = 0 inserts (ray 0, t = 1, 1) and zeroes slot 0 of the feature buffers (level
    stride > feature count), every other element keeps its poison; n_dev = 5 changes nothing at all.  With and without features."""
    for n_dev in (0, 5):
        for with_features in (True, False):
            buf = rk.fake_buffers(levels, features, n_dev)
            exp = rk.fake_expected(buf)
            d = {k: v.cuda() for k, v in buf.items()}
            feats = (d["x01"], d["sel"], d["y"]) if with_features else None
            _ops().fake_sample_if_empty(d["packed"], d["n_dev"], d["ray_indices"], d["t_starts"], d["t_ends"], feats)
            if not with_features:
                exp.update({k: buf[k] for k in ("x01", "sel", "y")})
            rk.check_fake(d, exp)
    print(f"RAYKERNEL fake_sample L={levels} F={features}: 0 elements differ")


def _vis_args(pad=rk.VIS_PAD, alphas=False):
    """The visibility inputs on the device with capacity extent: ``pad`` more elements than samples, NaN / poison in them."""
    inp, _ = rk.vis_inputs()
    n = inp["ts"].shape[0]
    fpad, ipad = torch.full((pad,), math.nan), torch.full((pad,), rk.POISON_I32, dtype=torch.int32)
    ri = torch.cat([inp["ray_indices"].int(), ipad]).cuda()
    ts, te = torch.cat([inp["ts"], fpad]).cuda(), torch.cat([inp["te"], fpad]).cuda()
    val = torch.cat([inp["alphas_f32"] if alphas else inp["sigma"], fpad]).cuda()
    return (ri, ts, te, val, inp["packed_info"].cuda()), n


def test_visibility_routes():
    """ops.visibility_compact_deferred: lse_visibility_mask (plain), lse_visibility_mask_cap (alpha_cap) and lse_visibility_mask_alpha
    (from_alpha), each followed by lse_pack_info_from_counts and lse_compact_samples on arrays of capacity extent."""
    ops = _ops()
    (ri, ts, te, sig, packed), n = _vis_args()
    given = (ri, ts, te, packed)
    plain = ops.visibility_compact_deferred(ri, ts, te, sig, packed, rk.VIS_EPS, rk.VIS_ALPHA_THRE)
    vis, und = rk.vis_density_ref(rk.VIS_ALPHA_THRE)
    band = rk.check_mask(plain[4][:n], vis, und)
    rk.check_compaction(plain, given, n)
    print(f"RAYKERNEL visibility plain: kept {int(plain[5])} of {n}, {band} in the band, 0 wrong")

    def same(a, b, what):
        m = int(a[5])
        rk.assert_exact(a[5], b[5], what + " n_dev")
        rk.assert_exact(a[4][:n], b[4][:n], what + " mask")
        rk.assert_exact(a[3], b[3], what + " new_packed")
        rk.assert_exact(a[0][:m], b[0][:m], what + " ray_indices")
        rk.assert_bitwise(a[1][:m], b[1][:m], what + " t_starts")
        rk.assert_bitwise(a[2][:m], b[2][:m], what + " t_ends")

    for cap_v, thre in ((rk.VIS_CAP_BELOW, rk.VIS_CAP_BELOW), (rk.VIS_CAP_ABOVE, rk.VIS_ALPHA_THRE)):
        cap = torch.tensor([cap_v], dtype=torch.float32, device="cuda")
        capped = ops.visibility_compact_deferred(ri, ts, te, sig, packed, rk.VIS_EPS, rk.VIS_ALPHA_THRE, alpha_cap=cap)
        rk.check_compaction(capped, given, n)
        same(capped, ops.visibility_compact_deferred(ri, ts, te, sig, packed, rk.VIS_EPS, float(cap.item()) if thre == cap_v else thre), f"alpha_cap {cap_v}")
        v, u = rk.vis_density_ref(rk.VIS_ALPHA_THRE, cap_v)
        band = rk.check_mask(capped[4][:n], v, u)
        print(f"RAYKERNEL visibility alpha_cap={cap_v}: kept {int(capped[5])} of {n}, {band} in the band, 0 wrong, bitwise the plain route at {thre}")
    assert int(ops.visibility_compact_deferred(ri, ts, te, sig, packed, rk.VIS_EPS, rk.VIS_CAP_BELOW)[5]) > int(plain[5])

    (ri, ts, te, alphas, packed), n = _vis_args(alphas=True)
    fa = ops.visibility_compact_deferred(ri, ts, te, alphas, packed, rk.VIS_EPS, rk.VIS_ALPHA_THRE, from_alpha=True)
    va, ua = rk.vis_alpha_ref(rk.VIS_ALPHA_THRE)
    band = rk.check_mask(fa[4][:n], va, ua)
    rk.check_compaction(fa, (ri, ts, te, packed), n)
    print(f"RAYKERNEL visibility from_alpha: kept {int(fa[5])} of {n}, {band} in the band, 0 wrong")


# ------------------------------------------------------------------------------------------------ ray bias / ray features
def _run_ray_bias(inp, preload=None):
    ops = _ops()
    d = _dev(inp["dirs"]).requires_grad_(True)
    emb = None if inp["emb"] is None else _dev(inp["emb"]).requires_grad_(True)
    idx = None if inp["idx"] is None else inp["idx"].int().cuda()
    head = _dev(inp["head"]).requires_grad_(True)
    if preload is not None:       # the direct-gradient route: the kernels add into the leaves' existing .grad
        head.grad = _dev(preload["d_head"])
        if emb is not None:
            emb.grad = _dev(preload["d_emb"])
    rb = ops.ray_bias(d, emb, idx, head, inp["width"])
    assert rb.shape == (inp["R"], inp["width"])
    (rb * inp["gout"].cuda()).sum().backward()
    return {"row_bias": rb.detach(), "d_dirs": d.grad, "d_emb": None if emb is None else emb.grad, "d_head": head.grad}


@pytest.mark.parametrize("case", rk.RAY_BIAS_CASES, ids=lambda c: c[0])
def test_ray_bias(case):
    """lse_ray_bias_fwd / lse_ray_bias_bwd / emb_grad_kernel (and lse_gemm_tn_acc for W_in where the padded width has an instance)
    through ops.ray_bias: row_bias, d(directions) per ray, d(embedding) per row (rows without a ray exactly 0), d(W_in) per output
    row, the rest of the head's gradient exactly 0 -- then the same with .grad of the embedding table and of the head preloaded:
    the result is the preload plus the reference."""
    inp = rk.ray_bias_inputs(case)
    ref = rk.ray_bias_eval(inp)
    res = rk.compare_ray_bias(_run_ray_bias(inp), ref, inp)
    pre = ray_bias_preload(inp)
    res_pre = rk.compare_ray_bias(_run_ray_bias(inp, pre), ref, inp, preload=pre, keys=("d_emb", "d_w_in"))
    res.update({k + "_preloaded": v for k, v in res_pre.items()})
    rk.report("ray_bias " + case[0], res)
    rk.assert_within(res, 1.0, case[0])


def test_ray_bias_raw_leading_dimension():
    """The raw C ABI with w_ld = padded width + 16 (NaN in the 16 extra columns of W_in: never read): lse_ray_bias_fwd,
    lse_ray_bias_bwd and lse_gemm_tn_acc with dw_ld = w_ld into a preloaded buffer whose extra columns keep their values."""
    case = rk.RAW_LD_CASE
    inp = rk.ray_bias_inputs(case)
    ref = rk.ray_bias_eval(inp)
    R, width, in_pad, emb_dim, rows = inp["R"], inp["width"], inp["in_pad"], inp["emb_dim"], inp["rows"]
    ld = in_pad + 16
    w = torch.full((width, ld), math.nan)
    w[:, :in_pad] = inp["head"][: width * in_pad].view(width, in_pad)
    w, d, emb, idx, gout = w.cuda(), inp["dirs"].cuda(), inp["emb"].cuda(), inp["idx"].int().cuda(), inp["gout"].cuda()
    feat = torch.full((R, in_pad), rk.POISON_F32, device="cuda")
    rb = torch.full((R, width), rk.POISON_F32, device="cuda")
    _call("lse_ray_bias_fwd", P(d), P(emb), P(idx), R, emb_dim, P(w), ld, width, P(feat), P(rb))
    d_feat = torch.full((R, in_pad), rk.POISON_F32, device="cuda")
    d_dirs = torch.full((R, 3), rk.POISON_F32, device="cuda")
    d_emb = torch.zeros(rows, emb_dim, device="cuda")
    _call("lse_ray_bias_bwd", P(d), P(idx), R, emb_dim, rows, P(w), ld, width, P(gout), P(d_feat), P(d_dirs), P(d_emb))
    pre = torch.randn(width, ld, generator=torch.Generator().manual_seed(4)) * 0.37
    dw = pre.cuda()
    _call("lse_gemm_tn_acc", P(gout), width, P(feat), in_pad, rk.ROWMAJOR, R, P(dw), ld)
    res = rk.compare_ray_bias({"row_bias": rb, "d_dirs": d_dirs, "d_emb": d_emb}, ref, inp, keys=("row_bias", "d_dirs", "d_emb"))
    res.update(rk.bounded("feat", feat.cpu(), ref["feat"], "fwd", row_bounds(R, in_pad)))
    rk.assert_bitwise(dw.cpu()[:, in_pad:].contiguous(), pre[:, in_pad:].contiguous(), "dW beyond the padded width")
    res.update(rk.bounded("d_w_in", dw.cpu()[:, :in_pad].contiguous(), pre[:, :in_pad].double() + ref["d_head"][: width * in_pad].view(width, in_pad),
                          "grad", row_bounds(width, in_pad)))
    rk.report("ray_bias " + case[0], res)
    rk.assert_within(res, 1.0, case[0])


@pytest.mark.parametrize("rows", rk.RAY_FEATURES_ROWS)
@pytest.mark.parametrize("R", rk.RAY_FEATURES_R)
def test_ray_features(R, rows):
    """lse_ray_features_fwd: bit for bit the [R, 64] feature matrix lse_ray_bias_fwd saves on the same inputs;
    lse_ray_features_bwd (+ emb_grad_kernel): d(directions) per ray and d(embedding) per row against float64."""
    inp = rk.ray_features_inputs(R, rows)
    up = rk.feature_upstream(inp)
    ref = rk.ray_bias_eval(inp, g_feat=up)
    d = _dev(inp["dirs"]).requires_grad_(True)
    emb = _dev(inp["emb"]).requires_grad_(True)
    idx = inp["idx"].int().cuda()
    feat = _ops().ray_features(d, emb, idx)
    saved = torch.full((R, 64), rk.POISON_F32, device="cuda")
    rb = torch.empty((R, 64), device="cuda")
    w = inp["head"][: 64 * 64].cuda()
    _call("lse_ray_bias_fwd", P(d), P(emb), P(idx), R, 32, P(w), 64, 64, P(saved), P(rb))
    rk.assert_bitwise(feat.detach(), saved, "features against the matrix lse_ray_bias_fwd saves")
    (feat * up.cuda()).sum().backward()
    res = rk.compare_ray_features({"d_dirs": d.grad, "d_emb": emb.grad}, ref, inp)
    res.update(rk.bounded("feat", feat.detach().cpu(), ref["feat"], "fwd", row_bounds(R, 64)))
    rk.report(f"ray_features R={R} rows={rows}", res)
    rk.assert_within(res)


# ------------------------------------------------------------------------------------------------ dense helpers
@pytest.mark.parametrize("inst", rk.GEMM_INSTANCES, ids=lambda i: f"m{i[0]}_k{i[1]}_{'lm' if i[2] else 'rm'}")
def test_dense_helpers(inst):
    """lse_linear_fwd, lse_linear_bwd_input and lse_gemm_tn_acc at every (m, k, layout) instance gemm_tn_dispatch lists and every row
    count: dW preloaded (the kernel accumulates) with dw_ld > k, the level-major layout strided by the row count."""
    m, k, layout = inst
    res = {}
    for n in rk.GEMM_ROWS:
        inp = rk.gemm_inputs(m, k, layout, n)
        ref = rk.gemm_eval(inp)
        x, w, dy = inp["x"].cuda(), inp["w"].cuda(), inp["dy"].cuda()
        y = torch.full((n, m), rk.POISON_F32, device="cuda")
        dx = torch.full((n, k), rk.POISON_F32, device="cuda")
        dw = inp["dw_pre"].cuda()
        _call("lse_linear_fwd", P(w), P(x), n, m, k, P(y))
        _call("lse_linear_bwd_input", P(w), P(dy), n, m, k, P(dx))
        a = rk.level_major(inp["x"]).cuda() if layout == rk.LEVELMAJOR else x
        _call("lse_gemm_tn_acc", P(dy), m, P(a), k, layout, n, P(dw), k + rk.GEMM_LD_EXTRA)
        r = rk.compare_gemm({"y": y, "dx": dx, "dw": dw}, ref, inp)
        res.update({f"{key}_n{n}": v for key, v in r.items()})
    rk.report(f"dense m={m} k={k} layout={layout}", res)
    rk.assert_within(res)


@pytest.mark.parametrize("m,k,layout", rk.GEMM_NOT_BUILT)
def test_gemm_tn_acc_without_an_instance_is_an_error(m, k, layout):
    """An (m, k, layout) that gemm_tn_dispatch does not list returns the library's error, not a result: dW is untouched."""
    n = 8
    g, a = torch.ones(n, m, device="cuda"), torch.ones(n * k, device="cuda")
    dw = torch.full((m, k), rk.POISON_F32, device="cuda")
    with pytest.raises(_lib().LseHipError, match="no kernel instance"):
        _call("lse_gemm_tn_acc", P(g), m, P(a), k, layout, n, P(dw), k)
    torch.cuda.synchronize()
    rk.assert_bitwise(dw, torch.full((m, k), rk.POISON_F32), "dW after the refused call")


@pytest.mark.parametrize("width", rk.SEG_WIDTHS)
def test_segment_sum_rows(width):
    """lse_segment_sum_rows: out (preloaded: the kernel adds into it) against float64 within (cnt / 4 + 4) * 2^-24 * sum|rows| per
    element -- the four-accumulator order of the sum."""
    res = {}
    for R in rk.SEG_R:
        inp = rk.seg_inputs(width, R)
        assert inp["rows"].shape == (int(inp["cnt"].sum()), width) and inp["rows"].numel() > 0
        rows, packed, out = inp["rows"].cuda(), inp["packed"].cuda(), inp["pre"].cuda()
        _call("lse_segment_sum_rows", P(rows), width, P(packed), R, P(out))
        res[f"R{R}"] = rk.compare_seg(out, rk.seg_eval(inp), inp)["segment_sum"]
    rk.report(f"segment_sum_rows width={width}", res)
    rk.assert_within(res)


@pytest.mark.parametrize("width", rk.SEG_BAD_WIDTHS)
def test_segment_sum_rows_refuses_other_widths(width):
    rows, out = torch.ones(8, 64, device="cuda"), torch.zeros(2, 64, device="cuda")
    packed = rk.pack(torch.tensor([4, 4])).cuda()
    with pytest.raises(_lib().LseHipError, match="width"):
        _call("lse_segment_sum_rows", P(rows), width, P(packed), 2, P(out))
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ density
@pytest.mark.parametrize("n", rk.DENSITY_N)
def test_density(n):
    """lse_density_fwd / lse_density_bwd (ops.density_from_mlp_out, row stride 16) at h = +-15 and their float32 neighbours, 0, +-80,
    89 (the forward overflows to +inf like float32 trunc_exp) and -104: the backward clamps to +-15, the forward does not.  Relative
    bound: 4 x the measured error of float32 torch.exp on these inputs, at least 2^-22.  Unselected outputs exactly 0."""
    res = {}
    for selector in rk.DENSITY_SELECTORS:
        inp = rk.density_inputs(n, selector)
        ref = rk.density_eval(inp)
        h = _dev(inp["h"]).requires_grad_(True)
        sigma = _ops().density_from_mlp_out(h, _dev(inp["sel"]), rk.DENSITY_SCALE)
        sigma.backward(inp["d_sigma"].cuda())
        assert float(h.grad[:, 1:].abs().max()) == 0.0
        r = rk.compare_density({"sigma": sigma.detach(), "d_h0": h.grad[:, 0]}, ref, inp)
        res.update({f"{k}_{selector}": v for k, v in r.items()})
        if n > 1 and selector == "none":
            i89 = int((inp["h"][:, 0] == 89).nonzero()[0])
            assert math.isinf(float(sigma[i89])) and float(sigma[i89]) > 0
    rk.report(f"density n={n} (exp error {rk.density_exp_error():.3e}, bound {rk.density_bound():.3e})", res)
    rk.assert_within(res)


# ------------------------------------------------------------------------------------------------ positions
def _aabb6(contraction):
    return None if contraction else [float(v) for v in rk.POS_AABB[0] + rk.POS_AABB[1]]


def _positions_raw(name, o, d, ri, ts, te, n, n_dev, contraction, a, b):
    """lse_positions_fwd (a = x01, b = selector) / lse_positions_bwd (a = d_x01, b = d_pos) through the C ABI."""
    box = _aabb6(contraction)
    arr = None if box is None else (ctypes.c_float * 6)(*box)
    _call(name, P(o), P(d), P(ri), P(ts), P(te), n, P(n_dev), int(contraction), arr, P(a), P(b))


def _positions_bwd_direct(points, upstream, contraction):
    n = points.shape[0]
    d_pos = torch.full((n, 3), rk.POISON_F32, device="cuda")
    _positions_raw("lse_positions_bwd", points.cuda(), None, None, None, None, n, None, contraction, upstream.cuda().contiguous(), d_pos)
    return d_pos.cpu()


@pytest.mark.parametrize("contraction", [True, False])
def test_positions_crafted_points(contraction):
    """lse_positions_fwd / lse_positions_bwd on points whose float32 arithmetic is exact: |p|_inf == 1 (identity, gradient 0.25 per
    axis), |p|_inf = 1e10 and 3e38 (the contraction gives exactly +-2: unselected, gradient 0), points on the aabb's faces and p == lo,
    one float32 step on either side of every face.  Selector and x01 equal the float32 oracle.field result, no face band left out."""
    pts = rk.crafted_points(contraction)
    n = pts.shape[0]
    x01_ref, sel_ref = rk.positions_f32_oracle(pts, contraction)
    x01, sel = _ops().positions(pts.cuda(), None, None, None, None, None, contraction, _aabb6(contraction))
    assert torch.equal(sel.cpu().bool(), sel_ref), "selector"
    assert torch.equal(x01.cpu(), x01_ref), "x01"
    up = torch.rand(n, 3, generator=torch.Generator().manual_seed(2)) + 0.5
    ref = rk.positions_eval({"contraction": contraction, "direct": True, "w": up}, torch.float32, points=pts)
    d_pos = _positions_bwd_direct(pts, up, contraction)
    assert float(d_pos[~sel_ref].abs().max()) == 0.0
    if contraction:
        on = pts.abs().amax(-1) == 1
        assert torch.equal(d_pos[on], 0.25 * up[on])
        assert not bool(sel_ref[pts.abs().amax(-1) >= 1e10].any())
    else:
        ext = torch.tensor(rk.POS_AABB[1]) - torch.tensor(rk.POS_AABB[0])
        assert torch.equal(d_pos[sel_ref], (up / ext)[sel_ref])
    # torch's autograd is NaN at the origin (the unselected branch of its `where` divides by |p|_inf = 0); the identity branch's
    # gradient there is 0.25 per axis like everywhere inside, which is asserted exactly instead
    fin = torch.isfinite(ref["d_pos"]).all(-1)
    assert bool(fin.all()) or (contraction and bool((pts[~fin] == 0).all()) and int((~fin).sum()) == 1)
    if contraction:
        inside = pts.abs().amax(-1) < 1
        assert bool((~fin <= inside).all()) and torch.equal(d_pos[inside], 0.25 * up[inside])
    res = rk.bounded("d_pos", d_pos[fin], ref["d_pos"][fin].double(), "grad", row_bounds(int(fin.sum()), 3))
    rk.report(f"positions crafted contraction={contraction}: {n} points, selector and x01 equal", res)
    rk.assert_within(res)


@pytest.mark.parametrize("direct", [False, True], ids=["rays", "direct"])
@pytest.mark.parametrize("contraction", [True, False], ids=["contraction", "aabb"])
@pytest.mark.parametrize("R", rk.POS_R)
def test_positions_seeded(R, contraction, direct):
    """lse_positions_fwd (ops.positions) and lse_positions_bwd (C ABI: d(position) per sample) on seeded rays against float64, ray
    mode and direct mode; samples within 1e-5 of a face of the unit cube (by the REFERENCE) carry no upstream gradient."""
    inp = rk.positions_inputs(R, contraction, direct)
    ref = rk.positions_reference(inp)
    keep, n = ~ref["edge"], inp["n"]
    if direct:
        o, d, ri, ts, te, packed = inp["points"].cuda(), None, None, None, None, None
    else:
        o, d, ri, ts, te, packed = inp["o"].cuda(), inp["d"].cuda(), inp["ri"].int().cuda(), inp["ts"].cuda(), inp["te"].cuda(), inp["packed"].cuda()
    x01, sel = _ops().positions(o, d, ri, ts, te, packed, contraction, _aabb6(contraction))
    assert torch.equal(sel.cpu().bool()[keep], ref["sel"][keep])
    res = rk.bounded("x01", x01.cpu()[keep], ref["x01"][keep], "fwd")
    up = (inp["w"] * keep[:, None]).contiguous().cuda()
    d_pos = torch.full((n, 3), rk.POISON_F32, device="cuda")
    _positions_raw("lse_positions_bwd", o, d, ri, ts, te, n, None, contraction, up, d_pos)
    worst, bad = per_ray_grad_check(d_pos.cpu()[keep], ref["d_pos"][keep], max_outliers=0)
    res["d_pos_per_sample"] = worst / TOL_GRAD
    assert float(d_pos.cpu()[~keep].abs().max() if bool((~keep).any()) else 0.0) == 0.0
    rk.report(f"positions R={R} contraction={contraction} direct={direct} n={n}", res)
    rk.assert_within(res)


def test_positions_tied_maxima():
    """At a tie of the largest |p_k| the L-inf norm has a set of sub-gradients.  CONVENTION: lse_positions_bwd gives the whole norm
    gradient to the FIRST maximal axis; torch splits it evenly over the tied axes (for p = (2, 2, 1) and upstream (1, 2, 3) torch's
    contraction gradient is (-0.375, 0.375, 2.25)).  Neither is wrong.  Asserted is what both agree on: the components of the untied
    axes, and the sum of sign(p_k) * grad_k over the tied axes."""
    pts = torch.tensor(rk.TIED_POINTS)
    up = torch.rand(pts.shape, generator=torch.Generator().manual_seed(3)) + 0.5
    ref = rk.positions_eval({"contraction": True, "direct": True, "w": up}, points=pts)
    d_pos = _positions_bwd_direct(pts, up, True)
    u, t = rk.tied_invariants(pts, d_pos)
    u0, t0 = rk.tied_invariants(pts, ref["d_pos"])
    res = rk.bounded("untied", u.float(), u0, "grad", row_bounds(pts.shape[0], 3))
    res.update(rk.bounded("tied_sum", t.float(), t0, "grad", list(range(pts.shape[0] + 1))))
    rk.report("positions tied maxima", res)
    rk.assert_within(res)


@pytest.mark.parametrize("contraction,direct", [(True, False), (False, True)], ids=["contraction_rays", "aabb_direct"])
def test_positions_device_count(contraction, direct):
    """n_dev of lse_positions_fwd and lse_positions_bwd with capacity n and counts {0, 1, n - 37, n, n + 5}: the prefix equals the run
    with that n; x01, selector and d_pos at or beyond the count keep their poison; NaN in t_starts / t_ends (direct mode: in the
    positions) beyond the count changes nothing."""
    inp = rk.positions_inputs(5, contraction, direct)
    n = inp["n"]
    assert n > 37
    up = inp["w"].cuda()
    src = {k: inp[k] for k in (("points",) if direct else ("o", "d", "ts", "te"))}
    ri = None if direct else inp["ri"].int().cuda()

    def run(n_arg, count, poisoned_inputs):
        t = {k: v.clone() for k, v in src.items()}
        if poisoned_inputs:
            for k in (("points",) if direct else ("ts", "te")):
                t[k][min(count, n):] = math.nan
        t = {k: v.cuda() for k, v in t.items()}
        o, d, ts, te = (t["points"], None, None, None) if direct else (t["o"], t["d"], t["ts"], t["te"])
        n_dev = None if count is None else torch.tensor([count], dtype=torch.int64, device="cuda")
        x01 = torch.full((n, 3), rk.POISON_F32, device="cuda")
        sel = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
        d_pos = torch.full((n, 3), rk.POISON_F32, device="cuda")
        _positions_raw("lse_positions_fwd", o, d, ri, ts, te, n_arg, n_dev, contraction, x01, sel)
        _positions_raw("lse_positions_bwd", o, d, ri, ts, te, n_arg, n_dev, contraction, up, d_pos)
        return x01.cpu(), sel.cpu(), d_pos.cpu()

    for count in (0, 1, n - 37, n, n + 5):
        eff = min(count, n)
        base = run(eff, None, False)                      # the plain run with that n (n = 0 launches nothing)
        got = run(n, count, True)
        for b, g, what in zip(base, got, ("x01", "selector", "d_pos")):
            poison = torch.full_like(b[eff:], 0xA5 if b.dtype == torch.uint8 else rk.POISON_F32)
            cmp = rk.assert_exact if b.dtype == torch.uint8 else rk.assert_bitwise
            cmp(g[:eff], b[:eff], f"{what} prefix, count {count}")
            cmp(g[eff:], poison, f"{what} at or beyond the count {count}")
            cmp(b[eff:], poison, f"{what} of the plain run beyond n = {eff}")
    print(f"RAYKERNEL positions n_dev contraction={contraction} direct={direct}: capacity {n}, 5 counts, 0 elements differ")
