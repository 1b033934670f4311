"""Rendered normals of the eval render (``LSENeRFModelConfig.eval_normals``) on a 24 x 16 camera over a small field with a
half-occupied grid: the count-free route against the ``forward`` loop bit for bit, colour untouched by the option, the image against
the float64 twin's compositing of ``LSEField.normals_packed`` on the same samples, the field API, and ``evaluate_set``'s picture."""
import functools

import pytest
import torch

from tests import normals_ref as nr
from tests.util import TOL_FWD, nmax_err, random_binaries, random_rays

pytestmark = pytest.mark.gpu

H, W = 16, 24             # 384 rays
CHUNK = 100               # four chunks, the last one 84 rays
AWAY = slice(140, 150)    # rays inside the second chunk that point away from every grid: no samples


@functools.lru_cache(maxsize=None)
def _model(eval_normals="off", contraction=True):
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig
    torch.manual_seed(5)
    cfg = LSENeRFModelConfig(grid_levels=2, grid_resolution=32, eval_num_rays_per_chunk=CHUNK, log2_hashmap_size=14,
                             eval_normals=eval_normals, disable_scene_contraction=not contraction)
    m = LSENeRFModel(cfg, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 8).cuda()
    with torch.no_grad():     # a table large enough for the logit to vary over a cell: gradients of ordinary size
        m.field.mlp_base_grid.params.uniform_(-0.5, 0.5, generator=torch.Generator(device="cuda").manual_seed(9))
    b = random_binaries(2, 32, 0.5, 5)
    m.occupancy_grid.binaries.copy_(b.cuda())
    m.occupancy_grid.occs.copy_(b.float().flatten().cuda() * 0.5)
    m.occupancy_grid._invalidate_occ_mean()
    return m.eval()


@functools.lru_cache(maxsize=None)
def _bundle():
    from lsenerf_amd import RayBundle
    o, d = random_rays(H * W, seed=1)
    o[AWAY], d[AWAY] = torch.tensor([3.0, 3.0, 3.0]), torch.tensor([1.0, 1.0, 1.0]) / 3.0 ** 0.5      # rays that meet no grid
    return RayBundle(origins=o.cuda().reshape(H, W, 3), directions=d.cuda().reshape(H, W, 3),
                     pixel_area=torch.full((H, W, 1), 1e-6, device="cuda"),
                     camera_indices=torch.zeros(H, W, 1, dtype=torch.long, device="cuda"),
                     metadata={"appearance_id": torch.arange(H * W, device="cuda").remainder(8).reshape(H, W, 1)})


@functools.lru_cache(maxsize=None)
def _render(eval_normals, contraction=True):
    return _model(eval_normals, contraction).get_outputs_for_camera_ray_bundle(_bundle())


def _loop(model):
    from lsenerf_amd.evaluation import _flatten_bundle, _slice
    flat = _flatten_bundle(_bundle())
    with torch.no_grad():
        outs = [model(_slice(flat, lo, min(len(flat), lo + CHUNK))) for lo in range(0, len(flat), CHUNK)]
    return {k: torch.cat([o[k] for o in outs]) for k in outs[0] if torch.is_tensor(outs[0][k])}


@pytest.mark.parametrize("mode", ["field", "world"])
def test_routes_agree_bit_for_bit_and_colour_is_unchanged(mode):
    from lsenerf_amd.evaluation import uses_count_free_route
    model = _model(mode)
    assert uses_count_free_route(model, H * W)
    out, loop, off = _render(mode), _loop(model), _render("off")
    assert "normals" not in off and set(out) == set(off) | {"normals"} and set(loop) == set(out)
    assert tuple(out["normals"].shape) == (H, W, 3)
    assert torch.equal(out["normals"].reshape(-1, 3), loop["normals"])
    for k in ("rgb", "accumulation", "depth", "num_samples_per_ray"):
        assert torch.equal(out[k], off[k]), k
        assert torch.equal(loop[k].reshape(out[k].shape), off[k]), k
    n = out["normals"].reshape(-1, 3)
    hit = out["num_samples_per_ray"].reshape(-1) > 0
    assert int(hit.sum()) > 50 and not bool(hit[AWAY].any())              # rays with and without samples
    assert bool((n[~hit] == 0.0).all())
    assert float((n[hit].norm(dim=-1) - 1.0).abs().max()) < 1e-4         # unit vectors
    assert not model.training


@pytest.mark.parametrize("mode,contraction", [("field", True), ("world", True), ("world", False)])
def test_image_against_the_twin_on_the_same_samples(mode, contraction):
    """Chunk by chunk as the count-free route marches them: d_x01 from ``normals_packed``, the rendered sigma, the twin's compositing."""
    from lsenerf_amd.evaluation import _flatten_bundle, _slice
    model = _model(mode, contraction)
    cfg, fld = model.config, model.field
    image = _render(mode, contraction)["normals"].reshape(-1, 3).cpu()
    flat = _flatten_bundle(_bundle())
    worst = 0.0
    with torch.no_grad():
        for lo in range(0, H * W, CHUNK):
            part = _slice(flat, lo, min(H * W, lo + CHUNK))
            ri, ts, te, packed, n_dev = model.sampler.sample_packed(
                part, near_plane=cfg.near_plane, far_plane=cfg.far_plane, render_step_size=cfg.render_step_size,
                alpha_thre=cfg.alpha_thre, cone_angle=cfg.cone_angle)
            rays_o, rays_d = part.origins.contiguous(), part.directions.contiguous()
            table, eidx = fld._eval_emb(len(part), rays_o.device)
            feats = {}
            sigma, _, _, _ = fld.density_rgb_packed(rays_o, rays_d, ri, ts, te, packed, eidx, table, n_dev, features_out=feats)
            d_x01 = fld.normals_packed(feats["x01"], feats["y"], n_dev)
            assert not d_x01.requires_grad
            ref = nr.composite_normals(ts, te, sigma, d_x01, packed, world=mode == "world", rays_o=rays_o, rays_d=rays_d,
                                       contraction=contraction, aabb6=None if contraction else fld._aabb_list())
            worst = max(worst, nmax_err(image[lo:lo + len(part)], torch.from_numpy(ref)))
    print("EVAL_NORMALS", mode, "contraction" if contraction else "aabb", "image vs twin:", worst)
    assert worst < 5 * TOL_FWD, worst


def test_d_x01_against_the_float64_field():
    """``normals_packed`` itself: the kernels' d_x01 against autograd through the float64 twin of grid and base network on points
    away from cell faces and ReLU gates."""
    from tests import hash_geometry_cases as hg
    from oracle import hashgrid as ohg
    from tests.util import TOL_GRAD
    model = _model("field")
    fld = model.field
    meta = fld.mlp_base_grid.meta
    meta_o = ohg.tcnn_grid_meta(n_levels=meta.n_levels, log2_hashmap_size=meta.log2_hashmap_size,
                                base_resolution=meta.base_resolution, per_level_scale=meta.per_level_scale)
    assert tuple(meta_o.offsets) == tuple(meta.offsets)
    g = torch.Generator().manual_seed(3)
    pos = (torch.rand(500, 3, generator=g) - 0.5) * 1.6
    with torch.no_grad():
        x01, sel, y = fld._encode_packed(pos.cuda(), None, None, None, None, None)
        d_x01 = fld.normals_packed(x01, y).cpu()
    ref, _, pre0 = nr.field_logit_grad64(x01.cpu().double(), fld.mlp_base_grid.params.detach().cpu(), meta_o,
                                         fld.mlp_base_mlp.params.detach().cpu())
    keep = ~(hg.on_face(x01.cpu(), meta_o.scales) | nr.gate_band(pre0))
    assert float(keep.float().mean()) > 0.8 and bool(sel.bool().all())
    err = nmax_err(d_x01[keep], ref[keep], 1e-12)
    print("EVAL_NORMALS d_x01 vs float64:", err, "kept", int(keep.sum()), "max |g|", float(ref.abs().max()))
    assert err < TOL_GRAD, err


def test_field_api_on_stock_ray_samples():
    from lsenerf_amd import _lib
    from lsenerf_amd.field import FieldHeadNames
    from lsenerf_amd.rays import Frustums, RaySamples
    fld = _model("off").field
    g = torch.Generator().manual_seed(4)
    o = ((torch.rand(6, 5, 3, generator=g) - 0.5) * 0.8).cuda()
    d = torch.nn.functional.normalize(torch.randn(6, 5, 3, generator=g), dim=-1).cuda()
    starts = torch.rand(6, 5, 1, generator=g).cuda() * 0.3
    fr = Frustums(origins=o, directions=d, starts=starts, ends=starts + 0.01, pixel_area=torch.full((6, 5, 1), 1e-6, device="cuda"))
    rs = RaySamples(frustums=fr, camera_indices=torch.zeros(6, 5, 1, dtype=torch.long, device="cuda"))
    with torch.no_grad():
        plain = fld(rs)
        out = fld(rs, compute_normals=True)
        sigma, normals = fld.density_normals(fr.get_positions())
    assert FieldHeadNames.NORMALS not in plain and set(out) == set(plain) | {FieldHeadNames.NORMALS}
    assert tuple(out[FieldHeadNames.NORMALS].shape) == (6, 5, 3) and tuple(normals.shape) == (6, 5, 3)
    assert torch.equal(out[FieldHeadNames.NORMALS], normals)
    assert torch.equal(out[FieldHeadNames.DENSITY], sigma) and torch.equal(out[FieldHeadNames.RGB], plain[FieldHeadNames.RGB])
    assert float((normals.norm(dim=-1) - 1.0).abs().max()) < 1e-5 and not normals.requires_grad
    # with gradients recorded for the rest of the field, the normals still carry no history
    out = fld(rs, compute_normals=True)
    assert out[FieldHeadNames.DENSITY].requires_grad and not out[FieldHeadNames.NORMALS].requires_grad
    assert torch.equal(out[FieldHeadNames.NORMALS], normals)


def test_field_api_on_packed_ray_samples():
    """The sampler's packed ``RaySamples``: NORMALS per sample, equal to ``normals_packed`` on the same packed samples."""
    from lsenerf_amd.evaluation import _flatten_bundle, _slice
    from lsenerf_amd.field import FieldHeadNames
    model = _model("off")
    cfg, fld = model.config, model.field
    part = _slice(_flatten_bundle(_bundle()), 0, CHUNK)
    with torch.no_grad():
        rs, _ = model.sampler(ray_bundle=part, near_plane=cfg.near_plane, far_plane=cfg.far_plane,
                              render_step_size=cfg.render_step_size, alpha_thre=cfg.alpha_thre, cone_angle=cfg.cone_angle)
        out = fld(rs, compute_normals=True)
        x01, _, y = fld._encode_packed(part.origins.contiguous(), part.directions.contiguous(), rs.ray_indices,
                                       rs.frustums.starts.reshape(-1), rs.frustums.ends.reshape(-1), rs.packed_info)
        want = -torch.nn.functional.normalize(fld.normals_packed(x01, y), dim=-1)
    n = rs.frustums.starts.reshape(-1).shape[0]
    assert n > 100 and out[FieldHeadNames.NORMALS].reshape(-1, 3).shape[0] == n
    assert torch.equal(out[FieldHeadNames.NORMALS].reshape(-1, 3), want)
    assert out[FieldHeadNames.DENSITY].reshape(-1).shape[0] == n


def test_small_grid_base_mlp_is_refused():
    from lsenerf_amd import _lib
    from lsenerf_amd.field import LSEField
    fld = LSEField(torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 4, num_levels=4, log2_hashmap_size=10).cuda().eval()
    assert fld.mlp_base_mlp.in_pad != fld.mlp_base_mlp.in_dim
    with pytest.raises(_lib.LseHipError, match="small-grid base MLP"):
        fld.density_normals(torch.zeros(4, 3, device="cuda"))


def test_evaluate_set_adds_the_picture_only_when_asked():
    from lsenerf_amd import EvalSet
    from lsenerf_amd.cameras import EdCameras
    from lsenerf_amd.evaluation import normals_colormap
    c2w = torch.tensor([[[1.0, 0, 0, 0.2], [0, 1, 0, 0.1], [0, 0, 1, 2.5]]])
    cams = EdCameras(c2w, fx=20.0, fy=20.0, cx=W / 2, cy=H / 2, width=W, height=H, times=torch.tensor([0.0]))
    images = torch.randint(0, 256, (1, H, W, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    es = EvalSet("cuda", images, cams, appearance_ids=[1])
    seen = {}
    for mode in ("off", "field"):
        _model(mode).evaluate_set(es, on_image=lambda i, outputs, imgs, mode=mode: seen.setdefault(mode, (outputs, imgs)))
    assert "normals" not in seen["off"][0] and "normals" not in seen["off"][1]
    outputs, imgs = seen["field"]
    assert tuple(imgs["normals"].shape) == (H, W, 3) and set(imgs) == set(seen["off"][1]) | {"normals"}
    assert torch.equal(imgs["normals"], normals_colormap(outputs["normals"], outputs["accumulation"]))
    assert float(imgs["normals"].min()) >= 0.0 and float(imgs["normals"].max()) <= 1.0 + 1e-6
