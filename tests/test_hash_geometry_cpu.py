"""CPU tier of the hash-grid geometry tests: the level tables of every geometry in tests/hash_geometry_cases.py against the
oracle's, the replica workspace the library sizes for them, that the shared inputs drive every path of the batched backward at
every geometry (instead of instrumenting the kernel), that the d(x) comparison skips at most 2 % of the samples, and that the
comparison the GPU tier uses rejects four subtly wrong results made on the CPU by mutated copies of the oracle."""
import ctypes

import numpy as np
import pytest
import torch

from tests import hash_geometry_cases as hc

ALL = list(hc.GEOMETRIES)


def _thresholds():
    """(few_runs, stage_max) of the library's defaults and of the constant-step regime (ops.HASH_BWD_DENSE_STEPS)."""
    from lsenerf_amd import _lib, ops
    o = _lib.hash_bwd_default_opts()
    dense = dict(ops.HASH_BWD_DENSE_STEPS)
    return [(int(o.few_runs), int(o.stage_max)), (int(dense["few_runs"]), int(dense["stage_max"]))]


def test_the_table_is_the_one_the_issue_lists():
    assert len(hc.GEOMETRIES) == 16 and set(hc.REP_LV) == set(hc.GEOMETRIES) | {hc.DEFAULT}
    levels = {n: hc.oracle_meta(n).n_levels for n in ALL}
    assert max(levels.values()) == 24 and sum(v > 16 for v in levels.values()) == 2 and min(levels.values()) == 1
    # what the rows are there to isolate
    m = hc.oracle_meta("b64_m4096")
    assert 2 * m.offsets[1] == hc.REPLICA_BUDGET_FLOATS and m.level_size(0) == 64 ** 3 == 1 << 18
    m = hc.oracle_meta("b48_m4096")
    assert hc.dense_levels(m) == [0, 1] and 2 * m.offsets[2] > hc.REPLICA_BUDGET_FLOATS
    m = hc.oracle_meta("b16_m128_L8_T22")
    assert hc.dense_levels(m) == list(range(8)) and m.resolutions[-1] == 128 and m.level_size(7) == 128 ** 3 == 1 << 21
    m = hc.oracle_meta("b2_m2048")
    assert [m.level_size(l) for l in range(4)] == [8, 64, 216, 512]
    m = hc.oracle_meta("b16_m16_L4")
    assert m.per_level_scale == 1.0 and len(set(m.scales)) == 1 and m.resolutions == [16] * 4
    m = hc.oracle_meta("T4_L4")
    assert [m.level_size(l) for l in range(4)] == [16] * 4 and hc.dense_levels(m) == []
    assert hc.dense_levels(hc.oracle_meta("L2_T10")) == [] and len(hc.dense_levels(hc.oracle_meta("L12_T17"))) == 3
    assert len(hc.dense_levels(hc.oracle_meta("b16_m1024"))) == 6


@pytest.mark.parametrize("name", ALL)
def test_level_table_dense_flags_and_replica_workspace(name):
    from lsenerf_amd import _lib, ops
    kw = hc.geometry_kwargs(name)
    meta, meta_o = ops.make_grid_meta(**kw), hc.oracle_meta(name)
    assert list(meta.offsets) == meta_o.offsets and list(meta.resolutions) == meta_o.resolutions
    assert np.array_equal(np.float32(meta.scales), np.float32(meta_o.scales))
    assert meta.n_levels <= _lib.LSE_MAX_GRID_LEVELS and all(o % 8 == 0 for o in meta.offsets)
    for l in range(meta.n_levels):
        assert hc.restated_dense(meta.resolutions[l], meta.offsets[l + 1] - meta.offsets[l]) == meta_o.is_dense(l), l
    o = _lib.hash_bwd_default_opts()
    rep_lv = hc.REP_LV[name]
    assert hc.restated_rep_lv(meta.offsets, meta.n_levels, o.replica_levels, o.replicas) == rep_lv
    desc = meta.desc()
    got = int(_lib.load().lse_hash_bwd_workspace_bytes(ctypes.byref(desc), None))
    assert got == o.replicas * 4 * 2 * meta.offsets[rep_lv]
    assert (got == 0) == (name == "b80_m4096")
    assert got == int(_lib.load().lse_hash_bwd_workspace_bytes(ctypes.byref(desc), ctypes.byref(o)))


def test_points_have_the_segments_the_tests_rely_on():
    x, seg = hc.make_points(0)
    x2, _ = hc.make_points(0)
    assert torch.equal(x, x2) and x.dtype == torch.float32 and not x.is_cuda
    n = x.shape[0]
    assert 4600 <= n <= 4800 and n % 64 != 0 and n % 1024 != 0
    assert seg["A"] == (0, 2048) and seg["B"][1] - seg["B"][0] == 2048 and seg["C"][1] == n
    assert bool(((x >= 0) & (x <= 1)).all())
    blocks = seg["zero_blocks"]
    assert tuple(hi - lo for lo, hi in blocks) == hc.ZERO_BLOCKS and sum(hc.ZERO_BLOCKS) == 640
    zero = (x == 0).all(-1)
    assert int(zero.sum()) == 640                      # exactly the blocks, nothing else
    for lo, hi in blocks:
        assert bool(zero[lo:hi].all()) and lo % 64 != 0
        assert not bool(zero[lo - 1]) and (hi == n or not bool(zero[hi]))
    # runs of zeros across a 16-lane row, a 64-sample wave and a 512-sample workgroup of the generic kernel
    assert any(lo // 16 != (hi - 1) // 16 for lo, hi in blocks) and any(lo // 64 != (hi - 1) // 64 for lo, hi in blocks)
    assert any(lo // 512 != (hi - 1) // 512 for lo, hi in blocks)
    # pos = 0.5 at every level: a sample at the origin is never on a cell face
    assert not bool(hc.on_face(x, [15.0, 2047.0, 4095.0])[zero].any())


@pytest.mark.parametrize("name", ALL)
def test_inputs_take_every_backward_path(name):
    """The batched backward picks a path per (wave = 64-sample chunk, level) by the number of run ends: at most few_runs -> direct
    adds (into the replicas on the levels below rep_lv), more than stage_max -> unstaged cache pass, in between -> queued pass.
    Counted here from the oracle's cell coordinates with the library's own thresholds.  Every geometry reaches all three paths
    with both threshold pairs -- including the ones with fewer than four levels, so no geometry is exempt."""
    x, seg = hc.make_points(0)
    meta_o = hc.oracle_meta(name)
    ne = hc.run_end_counts(x, meta_o)
    assert ne.shape == ((x.shape[0] + 63) // 64, meta_o.n_levels) and int(ne.min()) >= 1 and int(ne.max()) <= 64
    # a chunk inside a block of zeros is one run at every level; uniform points end a run in (nearly) every lane
    lo, hi = seg["zero_blocks"][-1]
    inside = [c for c in range(ne.shape[0]) if lo <= 64 * c and 64 * c + 64 <= hi]
    assert inside and bool((ne[inside] == 1).all())
    rep_lv = hc.REP_LV[name]
    for few_runs, stage_max in _thresholds():
        assert 0 < few_runs < stage_max < 64
        direct = ne <= few_runs
        if rep_lv > 0:
            assert bool(direct[:, :rep_lv].any()), (name, few_runs, "direct adds into the replicas")
            assert bool(direct[:, rep_lv - 1].any()), (name, few_runs, "direct adds into the last replicated level")
        else:
            assert bool(direct.any()), (name, few_runs, "direct adds")
        if rep_lv < meta_o.n_levels:
            assert bool(direct[:, rep_lv:].any()), (name, few_runs, "direct adds into the table gradient itself")
        assert bool(((ne > few_runs) & (ne <= stage_max)).any()), (name, few_runs, stage_max, "queued pass")
        assert bool((ne > stage_max).any()), (name, stage_max, "unstaged pass")


@pytest.mark.parametrize("name", ALL + [hc.DEFAULT])
def test_dx_check_skips_at_most_two_percent(name):
    x, _ = hc.make_points(0)
    meta_o = hc.oracle_meta(name)
    skipped = float(hc.on_face(x, meta_o.scales).float().mean())
    print(f"{name}: d(x) check skips {100 * skipped:.2f} % of {x.shape[0]} samples")
    assert skipped <= hc.MAX_ON_FACE
    if name in ("b16_m128_L8_T22", "L2_T10", hc.DEFAULT):
        xo = hc.make_out_of_range_points()
        assert bool(torch.isfinite(xo).all()) and float(xo.min()) < -3 and float(xo.max()) > 3
        assert float(((xo < 0) | (xo > 1)).any(-1).float().mean()) > 0.5
        assert float(hc.on_face(xo, meta_o.scales).float().mean()) <= hc.MAX_ON_FACE


def test_first_sample_is_off_every_face_where_a_count_of_one_is_tested():
    """tests/test_gpu_hash_geometry.py runs device-side counts of 1 and N - 777: the d(x) comparison of the truncated arrays must
    not consist of skipped samples."""
    x, _ = hc.make_points(0)
    for name in ("L1", "b64_m4096", "T4_L4"):
        face = hc.on_face(x, hc.oracle_meta(name).scales)
        assert not bool(face[0]) and float(face[: x.shape[0] - 777].float().mean()) <= hc.MAX_ON_FACE


# which mutation must be rejected where; the counts keep the parametrisation from becoming vacuous
_APPLIES = {
    "dense_as_hashed": [n for n in ALL if hc.dense_levels(hc.oracle_meta(n))],
    "unpadded_size": [n for n in ALL if hc.folding_levels(hc.oracle_meta(n), hc.make_points(0)[0])],
    "lost_corner": ALL,
    "lost_replica": [n for n in ALL if hc.REP_LV[n] > 0],
}


def test_every_mutation_applies_to_enough_geometries():
    assert {k: len(v) for k, v in _APPLIES.items()} == {"dense_as_hashed": 14, "unpadded_size": 6, "lost_corner": 16, "lost_replica": 15}


@pytest.mark.parametrize("name", ALL)
def test_comparison_passes_the_oracle_and_rejects_every_mutation(name):
    """``check_against_oracle`` is the comparison of the GPU tier.  It accepts the oracle's own results and rejects, at every
    geometry the mutation applies to: (a) a dense level indexed with the hash, (b) a dense level folded back with res^3 instead of
    its padded size (where some sample reaches the fold-back at all: hc.folding_levels), (c) the last sample of every 64-sample chunk reading one corner from the wrong entry at ONE level, (d) one of
    16 replicas of a replicated level lost.  So a kernel with one of these slips fails the GPU tests."""
    ref = hc.reference(name)
    meta_o = ref["meta_o"]
    res = hc.check_against_oracle(ref["y"], ref["dt"], ref["dx"], ref, meta_o)
    assert res["fwd"] == 0.0 and res["dt"] == 0.0 and res["dx"] == 0.0
    # the restated level is the oracle's, bit for bit (results_with_level asserts the forward; here the gradients too)
    same = hc.results_with_level(ref, meta_o.n_levels - 1)
    assert torch.equal(same["y"], ref["y"]) and torch.equal(same["dt"], ref["dt"])
    assert hc.check_against_oracle(same["y"], same["dt"], same["dx"], ref, meta_o)["dx"] < 1e-6
    muts = {"dense_as_hashed": hc.mutation_dense_as_hashed(ref), "unpadded_size": hc.mutation_unpadded_size(ref),
            "lost_corner": hc.mutation_lost_corner(ref), "lost_replica": hc.mutation_lost_replica(ref, hc.REP_LV[name])}
    for kind, bad in muts.items():
        assert (bad is not None) == (name in _APPLIES[kind]), (kind, name)
        if bad is None:
            continue
        with pytest.raises(AssertionError):
            hc.check_against_oracle(bad["y"], bad["dt"], bad["dx"], ref, meta_o)
        # ... and by the part of the comparison that is there for it
        if kind == "lost_replica":
            with pytest.raises(AssertionError):
                hc.check_against_oracle(None, bad["dt"], None, ref, meta_o)
        else:
            with pytest.raises(AssertionError):
                hc.check_against_oracle(bad["y"], None, None, ref, meta_o)
            with pytest.raises(AssertionError):
                hc.check_against_oracle(None, bad["dt"], None, ref, meta_o)


@pytest.mark.parametrize("name", [hc.DEFAULT, "b16_m128_L8_T22"])
def test_out_of_range_points_reach_the_fold_back_of_every_padded_level(name):
    """Outside [0, 1] the wrapped integer coordinates put the raw dense index anywhere in 2^32: every padded dense level takes the
    exact modulo, and a fold-back with the wrong size is rejected by the comparison on these inputs."""
    ref = hc.reference_out_of_range(name)
    meta_o = ref["meta_o"]
    assert hc.folding_levels(meta_o, ref["x"]) == hc.padded_dense_levels(meta_o) != []
    assert bool(torch.isfinite(ref["y"]).all()) and bool(torch.isfinite(ref["dt"]).all()) and bool(torch.isfinite(ref["dx"]).all())
    hc.check_against_oracle(ref["y"], ref["dt"], ref["dx"], ref, meta_o)
    bad = hc.mutation_unpadded_size(ref)
    with pytest.raises(AssertionError):
        hc.check_against_oracle(bad["y"], None, None, ref, meta_o)
    with pytest.raises(AssertionError):
        hc.check_against_oracle(None, bad["dt"], None, ref, meta_o)
