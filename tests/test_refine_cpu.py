"""Host side of the frozen-field refinement step, without a GPU: ``lse_hash_bwd_input`` in the header, the binding and both
libraries (ABI 6, additive), its argument checks, ``LSENeRFModel.freeze_field`` / ``unfreeze_field``, and the routing of the
appearance embedding under ``gbconfig.IS_EVAL`` (R:lse_nerf/lse_embeddings.py:36-38)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grid_desc():
    from lsenerf_amd import _lib
    d = _lib.GridDesc()
    d.n_levels, d.n_features = 1, 2
    d.offsets[0], d.offsets[1], d.scales[0], d.resolutions[0] = 0, 8, 1.0, 2
    return d


def test_hash_bwd_input_is_declared_bound_and_exported():
    from lsenerf_amd import _lib
    from tests.test_host_cpu import _exported
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lse_hip.h")).read(), flags=re.S)
    m = re.search(r"\blse_hash_bwd_input\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m and "const int64_t *n_dev" in m.group(1)
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 8 == len(_lib.SIGNATURES["lse_hash_bwd_input"])
    assert "dtable" not in m.group(1) and "workspace" not in m.group(1) and "opts" not in m.group(1)
    assert re.search(r"#define\s+LSE_ABI_VERSION\s+6\b", src)
    assert _lib.load().lse_abi_version() == 6 == _lib.LSE_ABI_VERSION
    assert "lse_hash_bwd_input" in _exported(_lib.LIB_PATH) and "lse_hash_bwd_input" in _exported(_lib.DEV_LIB_PATH)


def test_hash_bwd_input_argument_checks():
    """Validation runs before any launch: n = 0 is a no-op whatever the pointers are; null pointers with n > 0 and a bad
    descriptor are LSE_E_INVALID (-1)."""
    from lsenerf_amd import _lib
    lib = _lib.load()
    d = _grid_desc()
    one = ctypes.c_void_p(64)          # never dereferenced: every call below returns before a launch
    assert lib.lse_hash_bwd_input(ctypes.byref(d), None, None, None, None, 0, None, None) == 0
    for k in range(4):
        ptrs = [one] * 4
        ptrs[k] = None
        assert lib.lse_hash_bwd_input(ctypes.byref(d), *ptrs, 8, None, None) == -1, k
        assert b"lse_hash_bwd_input" in lib.lse_last_error()
    assert lib.lse_hash_bwd_input(ctypes.byref(d), one, one, one, one, -1, None, None) == -1
    assert lib.lse_hash_bwd_input(None, one, one, one, one, 8, None, None) == -1
    bad = _grid_desc()
    bad.n_features = 4
    assert lib.lse_hash_bwd_input(ctypes.byref(bad), one, one, one, one, 8, None, None) == -1 and b"n_features" in lib.lse_last_error()
    bad = _grid_desc()
    bad.n_levels = 0
    assert lib.lse_hash_bwd_input(ctypes.byref(bad), None, None, None, None, 0, None, None) == -1      # the descriptor comes first
    bad = _grid_desc()
    bad.offsets[1] = 0                 # an empty level
    assert lib.lse_hash_bwd_input(ctypes.byref(bad), one, one, one, one, 8, None, None) == -1
    with pytest.raises(_lib.LseHipError, match="null pointer"):
        _lib.call("lse_hash_bwd_input", ctypes.byref(d), None, None, None, None, 8, None, None)


def _model(embedding_type="evs_emb", eval_mode="param", **kw):
    import lsenerf_amd as la
    cfg = la.LSENeRFModelConfig(grid_levels=1, grid_resolution=8, log2_hashmap_size=8, num_levels=2,
                                embed_config=la.LSEEmbeddingConfig(embedding_type, eval_mode=eval_mode), **kw)
    return la.LSENeRFModel(cfg, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 30)


def test_freeze_field_flips_exactly_the_intended_flags():
    m = _model(use_mapping=True, mapping_method="mlp", map_mode="co_map", evs_mapping_method="powpow")
    m.init_test_params()
    emb = list(m.field.embedding_appearance.parameters())
    assert len(emb) == 2 and any(p is m.field.embedding_appearance.test_emb.weight for p in emb)
    trained = m.get_param_groups()["fields"]
    assert len(trained) > 6 and all(p.requires_grad for p in trained)
    others = [p for p in m.parameters() if not any(p is q for q in trained)]          # scene_aabb: never trainable
    assert others and not any(p.requires_grad for p in others)
    before = {id(p): p.requires_grad for p in m.parameters()}

    left = m.freeze_field()
    assert len(left) == len(emb) and all(any(p is q for q in emb) for p in left)
    for p in trained:
        assert p.requires_grad == any(p is q for q in emb)
    for name in ("mlp_base_grid", "mlp_base_mlp", "mlp_head"):
        assert not getattr(m.field, name).params.requires_grad, name
    assert not any(p.requires_grad for p in list(m.rgb_mapper.parameters()) + list(m.evs_mapper.parameters())
                   + list(m.rgb_to_one.parameters()))
    assert not any(p.requires_grad for p in others)
    with pytest.raises(RuntimeError, match="frozen already"):
        m.freeze_field()
    m.unfreeze_field()
    assert {id(p): p.requires_grad for p in m.parameters()} == before
    m.unfreeze_field()                                           # a second call changes nothing
    assert {id(p): p.requires_grad for p in m.parameters()} == before

    # camera-only refinement: nothing of the field stays trainable; a flag that was off before stays off afterwards
    m.field.mlp_head.params.requires_grad_(False)
    assert m.freeze_field(train_embedding=False) == []
    assert not any(p.requires_grad for p in m.parameters())
    m.unfreeze_field()
    assert not m.field.mlp_head.params.requires_grad and m.field.mlp_base_grid.params.requires_grad
    assert all(p.requires_grad for p in emb)


def test_freeze_field_ignores_the_eval_flag_when_it_lists_the_field():
    """``get_param_groups`` shrinks to the embedding under IS_EVAL; ``freeze_field`` freezes what a TRAINING run lists."""
    from lsenerf_amd import model as M
    m = _model()
    M.gbconfig.IS_EVAL = True
    try:
        left = m.freeze_field()
        assert M.gbconfig.IS_EVAL is True
        assert not m.field.mlp_base_grid.params.requires_grad and not m.field.mlp_head.params.requires_grad
        assert [id(p) for p in left] == [id(p) for p in m.get_param_groups()["fields"]]
    finally:
        M.gbconfig.IS_EVAL = False


def test_is_eval_routes_the_training_path_to_the_test_embedding():
    from lsenerf_amd import model as M
    ids = torch.tensor([3, 7, 7, 29])
    meta = {"appearance_id": ids}
    cams = torch.zeros(4, 1, dtype=torch.long)
    m = _model("evs_emb", "param").train()
    m.init_test_params()
    fld, emb = m.field, m.field.embedding_appearance
    assert M.gbconfig.IS_EVAL is False
    tab, idx = fld._ray_emb(meta, cams, 4, "cpu")
    assert tab is emb.embedding.weight and idx.dtype == torch.int32 and idx.tolist() == ids.tolist()
    g = _model("global_emb", "zero").train()
    z = _model("evs_emb", "zero").train()
    mean = _model("evs_emb", "mean").train()
    M.gbconfig.IS_EVAL = True
    try:
        tab, idx = fld._ray_emb(meta, cams, 4, "cpu")
        assert fld.training and tab is emb.test_emb.weight and tab.shape == (1, 32) and idx.tolist() == [0, 0, 0, 0]
        # the gradient of whatever reads those rows arrives at the test row, not at the training table
        tab[idx.long()].sum().backward()
        assert emb.test_emb.weight.grad is not None and emb.embedding.weight.grad is None
        # a global embedding has one row either way (R:lse_nerf/lse_embeddings.py:84-85); "zero" and "mean" as in evaluation
        tab, idx = g.field._ray_emb(meta, cams, 4, "cpu")
        assert tab is g.field.embedding_appearance.embedding.weight and idx.tolist() == [0, 0, 0, 0]
        assert z.field._ray_emb(meta, cams, 4, "cpu") == (None, None)
        tab, idx = mean.field._ray_emb(meta, cams, 4, "cpu")
        assert tab.shape == (1, 32) and torch.allclose(tab[0], mean.field.embedding_appearance.embedding.weight.mean(0))
    finally:
        M.gbconfig.IS_EVAL = False
    tab, idx = fld._ray_emb(meta, cams, 4, "cpu")
    assert tab is emb.embedding.weight and idx.tolist() == ids.tolist()
    m.eval()
    assert fld._ray_emb(meta, cams, 4, "cpu")[0] is emb.test_emb.weight           # evaluation mode: as before


def test_graphed_step_refuses_what_a_frozen_field_cannot_do():
    """Checked at construction, before anything touches the device."""
    from lsenerf_amd.graph import GraphedTrainStep
    m = _model().train()
    with pytest.raises(ValueError, match="camera_opt"):
        GraphedTrainStep(m, None)
    m.freeze_field()
    with pytest.raises(ValueError, match="frozen hash table"):
        GraphedTrainStep(m, object(), prefetch_march=True)
