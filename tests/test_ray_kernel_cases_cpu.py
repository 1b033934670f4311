"""CPU tier of the per-ray / sampler bookkeeping kernel tests (tests/ray_kernel_cases.py): float32 torch meets a QUARTER of every
bound on every committed case, the inputs reach the branches the kernels have, and the comparison helpers reject subtly wrong
results made from the references.  tests/test_gpu_ray_kernels.py runs the same cases and helpers on the kernels."""
import math

import pytest
import torch

from oracle import field as ofield
from tests import ray_kernel_cases as rk
from tests.util import TOL_GRAD, per_ray_grad_check

QUARTER = 0.25


def _f32(d):
    return {k: (v.float() if torch.is_tensor(v) and v.dtype == torch.float64 else v) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------ float32 restatement
@pytest.mark.parametrize("case", rk.RAY_BIAS_CASES + (rk.RAW_LD_CASE,), ids=lambda c: c[0])
def test_ray_bias_float32_meets_a_quarter_of_every_bound(case):
    inp = rk.ray_bias_inputs(case)
    ref, got = rk.ray_bias_eval(inp), _f32(rk.ray_bias_eval(inp, torch.float32))
    res = rk.compare_ray_bias(got, ref, inp)
    rk.report("cpu ray_bias " + case[0], res)
    rk.assert_within(res, QUARTER, case[0])
    # ... and with the gradient destinations preloaded (the direct-gradient route)
    pre = ray_bias_preload(inp)
    got["d_head"] = pre["d_head"] + got["d_head"]
    if inp["emb"] is not None:
        got["d_emb"] = pre["d_emb"] + got["d_emb"]
    rk.assert_within(rk.compare_ray_bias(got, ref, inp, preload=pre), QUARTER, case[0] + " preloaded")


def ray_bias_preload(inp):
    g = torch.Generator().manual_seed(23)
    pre = {"d_head": torch.randn(inp["head"].shape, generator=g) * 0.37}
    if inp["emb"] is not None:
        pre["d_emb"] = torch.randn(inp["emb"].shape, generator=g) * 0.37
    return pre


@pytest.mark.parametrize("rows", rk.RAY_FEATURES_ROWS)
@pytest.mark.parametrize("R", rk.RAY_FEATURES_R)
def test_ray_features_float32_meets_a_quarter_of_every_bound(R, rows):
    inp = rk.ray_features_inputs(R, rows)
    up = rk.feature_upstream(inp)
    ref, got = rk.ray_bias_eval(inp, g_feat=up), _f32(rk.ray_bias_eval(inp, torch.float32, g_feat=up))
    assert ref["feat"].shape == (R, 64) and bool((ref["feat"][:, 63] == 1).all()) and bool((ref["feat"][:, 16:31] == 0).all())
    rk.assert_within(rk.compare_ray_features(got, ref, inp), QUARTER)


@pytest.mark.parametrize("inst", rk.GEMM_INSTANCES, ids=lambda i: f"m{i[0]}_k{i[1]}_{'lm' if i[2] else 'rm'}")
def test_dense_helpers_float32_meet_a_quarter_of_every_bound(inst):
    for n in rk.GEMM_ROWS:
        inp = rk.gemm_inputs(*inst, n)
        ref, got = rk.gemm_eval(inp), rk.gemm_eval(inp, torch.float32)
        got["dw"] = torch.cat([got["dw"], inp["dw_pre"][:, inp["k"]:]], -1)
        rk.assert_within(rk.compare_gemm(got, ref, inp), QUARTER, (inst, n))
        if inst[2] == rk.LEVELMAJOR:
            lm = rk.level_major(inp["x"])
            assert lm.shape == (inst[1] // 2, n, 2) and torch.equal(lm[1, :, 1], inp["x"][:, 3])


@pytest.mark.parametrize("R", rk.SEG_R)
@pytest.mark.parametrize("width", rk.SEG_WIDTHS)
def test_segment_sum_float32_meets_a_quarter_of_its_bound(width, R):
    inp = rk.seg_inputs(width, R)
    assert int(inp["cnt"].max()) <= 200
    res = rk.compare_seg(rk.seg_eval(inp, torch.float32), rk.seg_eval(inp), inp)
    rk.assert_within(res, QUARTER, (width, R))


def test_segment_sum_cases_hold_every_length():
    assert set(rk.seg_lengths(64, 4099)) == set(rk.SEG_LENGTHS)
    lone = {rk.seg_lengths(w, 1)[0] for w in rk.SEG_WIDTHS}
    assert len(lone) == len(rk.SEG_WIDTHS) and 0 not in lone          # a lone ray: a different non-empty length at every width
    for w in rk.SEG_WIDTHS:
        for R in (4, 5):
            ls = rk.seg_lengths(w, R)
            assert any(l % 4 for l in ls) and any(l >= 4 for l in ls)


@pytest.mark.parametrize("selector", rk.DENSITY_SELECTORS)
@pytest.mark.parametrize("n", rk.DENSITY_N)
def test_density_float32_meets_a_quarter_of_its_bound(n, selector):
    inp = rk.density_inputs(n, selector)
    ref, got = rk.density_eval(inp), rk.density_eval(inp, torch.float32)
    res = rk.compare_density(got, ref, inp)
    print("density exp error", rk.density_exp_error(), "bound", rk.density_bound())
    assert all(v <= QUARTER for v in res.values()), res
    assert 2.0 ** -26 < rk.density_exp_error() < 2.0 ** -22          # a plausible float32 exp: between a sixteenth of an ulp and 2 ulp
    if n > 1:
        h0 = inp["h"][:, 0]
        i89 = int((h0 == 89).nonzero()[0])
        f32 = ofield.trunc_exp(h0)
        assert math.isinf(float(f32[i89])) and (selector == "zeros" or inp["sel"] is not None and not inp["sel"][i89] or math.isinf(float(got["sigma"][i89])))
        # the backward clamps to +-15, the forward does not
        i80 = int((h0 == 80).nonzero()[0])
        assert float(ref["d_h0"][i80].abs()) <= rk.DENSITY_SCALE * 8 * math.exp(15) * (1 + 1e-12)
        for c in (15.0, -15.0):
            assert int((h0 < c).sum()) and int((h0 > c).sum()) and int((h0 == c).sum()) == 1
        assert {15.0, -15.0} < set(h0[:6].tolist()) and len(set(h0[:6].tolist())) == 6


@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("contraction", [True, False])
@pytest.mark.parametrize("R", rk.POS_R)
def test_positions_float32_meets_a_quarter_of_every_bound(R, contraction, direct):
    inp = rk.positions_inputs(R, contraction, direct)
    ref, got = rk.positions_reference(inp), rk.positions_eval(inp, torch.float32)
    keep = ~ref["edge"]
    assert float(ref["edge"].float().mean()) < 0.01
    assert torch.equal(got["sel"][keep], ref["sel"][keep])
    res = rk.bounded("x01", got["x01"][keep].float(), ref["x01"][keep], "fwd")
    rk.assert_within(res, QUARTER)
    per_ray_grad_check(got["d_pos"][keep], ref["d_pos"][keep], tol=TOL_GRAD * QUARTER, max_outliers=0, outlier_tol=1e-2 * QUARTER)
    # branch coverage: both contraction branches with at least 20 samples each; inside and outside the aabb
    mag = ref["pos"].abs().amax(-1)
    if contraction:
        assert int((mag < 1).sum()) >= 20 and int((mag >= 1).sum()) >= 20, (int((mag < 1).sum()), int((mag >= 1).sum()))
    else:
        assert int(ref["sel"].sum()) >= 20 and int((~ref["sel"]).sum()) >= 20


# ------------------------------------------------------------------------------------------------ exact references and inputs
def test_pack_info_cases_cross_a_thread_run_a_wave_and_the_workgroup():
    pers = {R: rk.pack_thread_run(R) for R in rk.PACK_R}
    assert {0, 1, 2, 3, 4, 5, 65} == set(pers.values())
    assert pers[1024] == 1 and pers[1025] == 2 and pers[2048] == 2 and pers[2049] == 3
    for R in rk.PACK_R:
        for pat in rk.PACK_PATTERNS:
            c = rk.pack_counts(R, pat)
            assert c.shape == (R,) and c.dtype == torch.int64
            packed, total = rk.pack_reference(c)
            assert packed.shape == (R, 2) and total.shape == (1,) and int(total) == sum(c.tolist())
        if R >= 2:
            assert int(rk.pack_reference(rk.pack_counts(R, "big_middle"))[1]) > 2 ** 33
            lo = rk.pack_counts(R, "last_only")
            assert int(lo[:-1].sum()) == 0 and int(lo[-1]) > 0


def test_comparison_rejects_an_inclusive_offset_on_a_thread_run_boundary():
    R = 2049
    per = rk.pack_thread_run(R)
    packed, _ = rk.pack_reference(rk.pack_counts(R, "ones"))
    rk.assert_exact(packed, packed.clone(), "packed")
    for index in (per, 64 * per, R - 1):          # first ray of thread 1, of wave 1, the last ray
        with pytest.raises(AssertionError):
            rk.assert_exact(rk.mutation_inclusive_offset(packed, index), packed, "packed")


def test_slot_cases_hold_empty_and_full_rays():
    for R in rk.SLOT_R:
        for cap in rk.SLOT_CAP:
            inp = rk.slot_inputs(R, cap)
            cnt = inp["cnt"]
            assert int(cnt.min()) >= 0 and int(cnt.max()) <= cap and inp["ts_slots"].shape == (R * cap,)
            if R > 1:
                assert bool((cnt == 0).any()) and bool((cnt == cap).any())
            s = inp["ts_slots"].view(R, cap)
            assert int(torch.isnan(s).sum()) == R * cap - inp["total"] and not bool(torch.isnan(inp["ref"]["t_starts"]).any())
            got = {"ray_indices": torch.full((inp["capacity"],), rk.POISON_I32, dtype=torch.int32),
                   "t_starts": torch.full((inp["capacity"],), rk.POISON_F32), "t_ends": torch.full((inp["capacity"],), rk.POISON_F32)}
            for k, v in inp["ref"].items():
                got[k][: inp["total"]] = v
            rk.check_compacted(got, inp)
            if inp["total"]:
                got["t_ends"][inp["total"]] = 0.5              # a write beyond the total
                with pytest.raises(AssertionError):
                    rk.check_compacted(got, inp)
    assert {int(rk.slot_inputs(1, c)["cnt"][0]) for c in rk.SLOT_CAP} >= {0, 1, 63, 65}


def test_ray_planes_inputs_tell_a_fused_multiply_add_apart():
    for R in rk.PLANES_R:
        inp = rk.planes_inputs(R)
        assert bool((inp["t_min"] < rk.PLANES_NEAR).any() or R == 1) and bool((inp["t_min"] > rk.PLANES_NEAR).any() or R == 1)
        two, _ = rk.planes_reference(inp, True, True, True)
        one, _ = rk.planes_reference(inp, True, True, True, fused=True)
        share = float((two != one).float().mean())
        print(f"ray_planes R={R}: a fused multiply-add gives other bits in {share:.1%} of the rays")
        if R > 1:
            assert share >= 0.10, share
            with pytest.raises(AssertionError):
                rk.assert_bitwise(one, two, "near")
    big = rk.planes_inputs(4099)
    assert bool((big["t_max"] < rk.PLANES_FAR).any()) and bool((big["t_max"] > rk.PLANES_FAR).any())
    assert len(rk.PLANES_COMBOS) == 8


def test_fake_sample_expectation():
    for L, F in rk.FAKE_SHAPES:
        assert rk.FAKE_CAPACITY * F > F
        buf = rk.fake_buffers(L, F, 5)
        rk.check_fake(buf, rk.fake_expected(buf))
        buf0 = rk.fake_buffers(L, F, 0)
        exp = rk.fake_expected(buf0)
        assert exp["packed"][0].tolist() == [0, 1] and int(exp["n_dev"]) == 1 and float(exp["t_starts"][0]) == 1.0
        assert int((exp["y"] == 0).sum()) == L * F and int((exp["x01"] == 0).sum()) == 3
        with pytest.raises(AssertionError):
            rk.check_fake(buf0, exp)


def test_visibility_references_and_the_alpha_cap_mutation():
    inp, ref = rk.vis_inputs()
    assert inp["packed_info"][:, 1].tolist() == list(rk.FIXED_RAY_LENGTHS)
    vis, und = rk.vis_density_ref(rk.VIS_ALPHA_THRE)
    assert rk.check_mask(vis, vis, und) == int(und.sum())
    T, a = ref["trans"], ref["alphas"]
    assert bool((T < rk.VIS_EPS).any()) and bool(((a < rk.VIS_ALPHA_THRE) & (T >= rk.VIS_EPS)).any()) and bool(vis.any())
    assert rk.VIS_CAP_BELOW < rk.VIS_ALPHA_THRE < rk.VIS_CAP_ABOVE
    lo, _ = rk.vis_density_ref(rk.VIS_ALPHA_THRE, rk.VIS_CAP_BELOW)
    assert int(lo.sum()) > int(vis.sum())                      # the haze straddles the lower cap: it changes the mask
    hi, und_hi = rk.vis_density_ref(rk.VIS_ALPHA_THRE, rk.VIS_CAP_ABOVE)
    assert torch.equal(hi, vis)
    # `max` in place of `min` in the alpha_cap threshold
    for cap in (rk.VIS_CAP_BELOW, rk.VIS_CAP_ABOVE):
        good, und_c = rk.vis_density_ref(rk.VIS_ALPHA_THRE, cap)
        wrong, _ = rk.vis_density_ref(rk.VIS_ALPHA_THRE, cap, combine=max)
        with pytest.raises(AssertionError):
            rk.check_mask(wrong, good, und_c)
    va, ua = rk.vis_alpha_ref(rk.VIS_ALPHA_THRE)
    assert float(ua.float().mean()) <= rk.VIS_MAX_UNDECIDED and float(((va != vis) & ~ua & ~und).float().mean()) == 0.0
    # the compaction check: a consistent result passes, a shifted offset does not
    n = inp["ts"].shape[0]
    ri = inp["ray_indices"].int()
    cnt = torch.zeros(len(rk.FIXED_RAY_LENGTHS), dtype=torch.int64).index_add_(0, ri.long(), vis.long())
    out = [ri[vis], inp["ts"][vis], inp["te"][vis], rk.pack(cnt), vis.to(torch.uint8), torch.tensor([int(vis.sum())])]
    rk.check_compaction(out, (ri, inp["ts"], inp["te"], inp["packed_info"]), n)
    out[3] = rk.mutation_inclusive_offset(out[3], 3)
    with pytest.raises(AssertionError):
        rk.check_compaction(out, (ri, inp["ts"], inp["te"], inp["packed_info"]), n)


# ------------------------------------------------------------------------------------------------ branch coverage of the ray-bias table
def test_ray_bias_table_covers_what_the_kernels_branch_on():
    C = rk.RAY_BIAS_CASES
    assert 12 <= len(C) <= 16
    assert {c[1] for c in C} == {32, 64}
    assert {c[2] for c in C} == {None, 1, 16, 17, 32, 33, 97}
    assert {rk.in_pad_of(c[2]) for c in C} == {32, 48, 64, 128}
    for width in (32, 64):                                     # both LDS pitches at both widths
        assert {rk.in_pad_of(c[2]) <= 64 for c in C if c[1] == width} == {True, False}
    assert {c[3] for c in C} == {1, 15, 16, 17, 4099}
    assert {c[4] for c in C if c[2] is not None} == {1, 3, 1000}
    assert {c[5] for c in C} == {"one_row", "own_row", "blocks", "random", "sparse", "none"}
    empty_part = odd_part = unused_row = False
    for c in C:
        inp = rk.ray_bias_inputs(c)
        R = inp["R"]
        parts = rk.emb_partitions(R)
        assert parts[0][0] == 0 and max(p[1] for p in parts) == R and all(a[1] == b[0] or b[0] == R for a, b in zip(parts, parts[1:]))
        if inp["idx"] is not None:
            empty_part |= any(hi == lo for lo, hi in parts)
            odd_part |= any((hi - lo) % 4 for lo, hi in parts)
            used = torch.zeros(inp["rows"], dtype=torch.bool)
            used[inp["idx"]] = True
            unused_row |= not bool(used.all())
            assert int(inp["idx"].min()) >= 0 and int(inp["idx"].max()) < inp["rows"]
            if c[5] == "sparse":
                assert not bool(used[1::2].any())
            if c[5] == "blocks":
                assert bool((inp["idx"][1:] >= inp["idx"][:-1]).all()) and bool(used.all())
        if R >= 15:
            d = inp["dirs"]
            n = d.norm(dim=-1)
            assert bool((n == 0).any()) and bool(((n - 0.25).abs() < 1e-6).any()) and bool(((n - 3).abs() < 1e-5).any())
            for k in range(3):
                for s in (1.0, -1.0):
                    assert bool((d == s * torch.eye(3)[k]).all(-1).any())
    assert empty_part and odd_part and unused_row
    assert rk.in_pad_of(rk.RAW_LD_CASE[2]) == 64


# ------------------------------------------------------------------------------------------------ mutations of the float references
def _rejected(res):
    with pytest.raises(AssertionError):
        rk.assert_within(res)
    return rk.worst(res)


def test_comparison_rejects_a_scaled_small_embedding_row():
    case = rk.RAY_BIAS_BY_NAME["w64_e32_R4099_rows3_blocks"]
    inp = rk.ray_bias_inputs(case)
    ref = rk.ray_bias_eval(inp)
    mut, row = rk.mutation_scaled_small_row(ref, inp)
    mx = ref["d_emb"].abs().amax(-1)
    assert float(mx[row]) < 0.05 * float(mx.max())                 # a small row next to a large one that stays exact
    res = rk.compare_ray_bias(_f32(mut), ref, inp)
    assert res["d_emb"] < 1.0                                      # the global view does not see it
    assert _rejected(res)[0] == "d_emb_blk"
    assert rk.worst(rk.compare_ray_bias(_f32(ref), ref, inp))[1] < 0.01


@pytest.mark.parametrize("name", ["w64_e32_R4099_rows3_blocks", "w32_e1_R4099_rows1000_sparse", "w64_e97_R4099_rows3_blocks", "w64_none_R17",
                                  "w32_e16_R15_rows1000_own"])
def test_comparison_rejects_zero_padding_and_a_flipped_sh_sign(name):
    inp = rk.ray_bias_inputs(rk.RAY_BIAS_BY_NAME[name])
    ref = rk.ray_bias_eval(inp)
    zp = rk.compare_ray_bias(_f32(rk.ray_bias_eval(inp, mutation="zero_padding")), ref, inp)
    if inp["in_pad"] > 31 + (inp["emb_dim"] or 0):            # (embedding widths 1, 17, 33, 97 fill the padded width: no ones column)
        with pytest.raises(AssertionError):
            rk.assert_within({k: v for k, v in zp.items() if k.startswith("row_bias")})
        with pytest.raises(AssertionError):
            rk.assert_within({k: v for k, v in zp.items() if k.startswith("d_w_in")})
    else:
        assert name in ("w32_e1_R4099_rows1000_sparse", "w64_e97_R4099_rows3_blocks")
        rk.assert_within(zp, 0.25)
    sh = rk.compare_ray_bias(_f32(rk.ray_bias_eval(inp, mutation="sh_sign")), ref, inp)
    for key in ("row_bias", "d_dirs", "d_w_in"):
        with pytest.raises(AssertionError):
            rk.assert_within({k: v for k, v in sh.items() if k.startswith(key)})


def test_comparison_rejects_a_segment_sum_without_its_tail():
    for width, R in ((64, 4099), (1, 5), (63, 4)):
        inp = rk.seg_inputs(width, R)
        ref = rk.seg_eval(inp)
        assert rk.compare_seg(ref.float(), ref, inp)["segment_sum"] == 0.0
        res = rk.compare_seg(rk.seg_eval(inp, drop_tail=True).float(), ref, inp)
        assert _rejected(res)[1] > 100
        # a ray without rows must come back as the preload, exactly
        empty = (inp["cnt"] == 0).nonzero()
        if empty.numel():
            bad = ref.clone()
            bad[int(empty[0]), 0] += rk.SEG_QUANTUM
            assert math.isinf(rk.compare_seg(bad.float(), ref, inp)["segment_sum"])


def test_contraction_gradient_on_the_wrong_axis_and_the_tie_convention():
    """At a tie of |p_k| the L-inf norm has a set of sub-gradients: the kernel gives the whole norm gradient to the first maximal
    axis, torch splits it evenly.  Both agree on the untied components and on the sum of sign(p_k) * grad_k over the tied axes --
    ``tied_invariants``, what the GPU tier asserts."""
    p = torch.tensor([[2.0, 2.0, 1.0]], dtype=torch.float64, requires_grad=True)
    (ofield.contract_inf(p) * torch.tensor([[1.0, 2.0, 3.0]], dtype=torch.float64)).sum().backward()
    assert torch.equal(p.grad, torch.tensor([[-0.375, 0.375, 2.25]], dtype=torch.float64))
    pts = torch.tensor(rk.TIED_POINTS)
    up = torch.rand(pts.shape, generator=torch.Generator().manual_seed(3)) + 0.5
    inp = {"contraction": True, "direct": True, "w": up}
    ref = rk.positions_eval(inp, points=pts)
    # the kernel's convention, restated: s * g / 4 on every axis, the norm term on the FIRST maximal axis
    a = pts.double().abs()
    m = a.amax(-1, keepdim=True)
    s, ds = 2 / m - 1 / m ** 2, -2 / m ** 2 + 2 / m ** 3
    first = torch.zeros_like(a).scatter_(1, (a == m).double().argmax(-1, keepdim=True), 1.0)
    dot = (up.double() * pts.double()).sum(-1, keepdim=True)
    kern = 0.25 * s * up.double() + first * 0.25 * dot * ds * torch.sign(pts.double())
    assert float((kern - ref["d_pos"]).abs().max()) > 1e-3                       # the two conventions do differ
    for got in (kern, ref["d_pos"]):
        u, t = rk.tied_invariants(pts, got)
        u0, t0 = rk.tied_invariants(pts, ref["d_pos"])
        assert float((u - u0).abs().max()) < 1e-12 and float((t - t0).abs().max()) < 1e-12
    # the norm gradient on a wrong (non-maximal) axis: rejected by the invariants and, on untied points, by the per-ray check
    wrong = 0.25 * s * up.double() + first.roll(1, -1) * 0.25 * dot * ds
    u, t = rk.tied_invariants(pts, wrong)
    assert float((u - u0).abs().max()) > 1e-3 or float((t - t0).abs().max()) > 1e-3
    seeded = rk.positions_inputs(5, True, True)
    sref = rk.positions_reference(seeded)
    q = sref["pos"]
    qa = q.abs()
    qm = qa.amax(-1, keepdim=True)
    out = qm[:, 0] >= 1
    norm_term = sref["d_pos"] - 0.25 * torch.where(out[:, None], 2 / qm - 1 / qm ** 2, torch.ones_like(qm)) * seeded["w"].double()
    moved = sref["d_pos"] - norm_term + norm_term.roll(1, -1)
    with pytest.raises(AssertionError):
        per_ray_grad_check(moved, sref["d_pos"], max_outliers=0)


def test_crafted_points_are_what_they_claim():
    for contraction in (True, False):
        pts = rk.crafted_points(contraction)
        x01, sel = rk.positions_f32_oracle(pts, contraction)
        ref = rk.positions_eval({"contraction": contraction, "direct": True, "w": torch.ones(pts.shape)}, torch.float32, points=pts)
        assert torch.equal(ref["x01"], x01) and torch.equal(ref["sel"], sel)
        assert bool(sel.any()) and bool((~sel).any())
        bad = ~torch.isfinite(ref["d_pos"]).all(-1)        # autograd through the unselected `where` branch: NaN at |p|_inf = 0 only
        assert bool((pts[bad] == 0).all()) and int(bad.sum()) == (1 if contraction else 0)
        if contraction:
            on = pts.abs().amax(-1) == 1
            assert int(on.sum()) == 6 and bool(sel[on].all()) and torch.equal(x01[on], (pts[on] + 2) / 4)
            assert torch.equal(ref["d_pos"][on], torch.full((6, 3), 0.25))                           # identity branch: 0.25 per axis
            far = pts.abs().amax(-1) >= 1e10
            assert int(far.sum()) == 4 and not bool(sel[far].any()) and float(x01[far].abs().max()) == 0.0
            assert float(ref["d_pos"][far].abs().max()) == 0.0
            raw = (ofield.contract_inf(pts[far]) + 2) / 4
            assert bool(((raw.amax(-1) == 1) | (raw.amin(-1) == 0)).all())                       # the contraction gives exactly +-2
        else:
            lo, hi = (torch.tensor(v) for v in rk.POS_AABB)
            on_face = ((pts == lo) | (pts == hi)).any(-1)
            assert int(on_face.sum()) == 8 and not bool(sel[on_face].any())
            # one float32 step outside a face is outside; one step inside is inside where (p - lo) is still exact, and ON the face
            # where the subtraction rounds the step away (p = hi - ulp on an axis with |lo| >= |hi|): float32's answer, the kernel's too
            assert 1 + 3 <= int(sel.sum()) <= 1 + 6 and int((~sel).sum()) >= 8 + 6 and pts.shape[0] == 3 + 6 * 3
