"""Whole-image evaluation on the GPU: LSENeRFModel.get_outputs_for_camera_ray_bundle (count-free route + lse_eval_composite)
against the eager eval forward it replaces (bit for bit) and the CPU oracle, the host-sync count of both routes, output shapes,
the lse_image_metrics kernel against a float64 numpy restatement, and get_image_metrics_and_images."""
import math

import numpy as np
import pytest
import torch

from tests.test_eval_cpu import ssim_numpy
from tests.util import TOL_FWD, nmax_err, random_binaries, random_rays

pytestmark = pytest.mark.gpu

H, W = 24, 40             # 960 rays
CHUNK = 256               # four chunks, the last one 192 rays
KEYS = ("rgb", "accumulation", "depth", "num_samples_per_ray")


def _model(seed=5, num_train_data=8, **kw):
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig
    torch.manual_seed(seed)
    cfg = LSENeRFModelConfig(grid_levels=2, grid_resolution=32, eval_num_rays_per_chunk=CHUNK, **kw)
    m = LSENeRFModel(cfg, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), num_train_data).cuda()
    b = random_binaries(2, 32, 0.5, seed)
    m.occupancy_grid.binaries.copy_(b.cuda())
    m.occupancy_grid.occs.copy_(b.float().flatten().cuda() * 0.5)
    m.occupancy_grid._invalidate_occ_mean()
    return m.eval()


def _bundle(seed=1, empty_chunk=None):
    """An [H, W] bundle of rays aimed into the scene box; ``empty_chunk``: the rays of that chunk point away from every grid."""
    from lsenerf_amd import RayBundle
    o, d = random_rays(H * W, seed=seed)
    if empty_chunk is not None:
        sl = slice(empty_chunk * CHUNK, (empty_chunk + 1) * CHUNK)
        o[sl] = torch.tensor([3.0, 3.0, 3.0])
        d[sl] = torch.tensor([1.0, 1.0, 1.0]) / math.sqrt(3.0)
    n = H * W
    return RayBundle(origins=o.cuda().reshape(H, W, 3), directions=d.cuda().reshape(H, W, 3),
                     pixel_area=torch.full((H, W, 1), 1e-6, device="cuda"),
                     camera_indices=torch.zeros(H, W, 1, dtype=torch.long, device="cuda"),
                     metadata={"appearance_id": torch.arange(n, device="cuda").remainder(8).reshape(H, W, 1)})


def _eager(model, bundle):
    """What a user writes today: model(chunk) in eval mode over the same chunks."""
    from lsenerf_amd.evaluation import _flatten_bundle, _slice
    flat = _flatten_bundle(bundle)
    outs = [model(_slice(flat, lo, min(len(flat), lo + CHUNK))) for lo in range(0, len(flat), CHUNK)]
    return {k: torch.cat([o[k] for o in outs]) for k in outs[0] if torch.is_tensor(outs[0][k])}


def _check_equal(model, bundle, mapper_keys=(), exact=KEYS):
    """``exact`` keys bit for bit; ``mapper_keys`` (mapper / nn.Linear outputs: library GEMMs round by batch size) within 1e-6."""
    from lsenerf_amd.evaluation import uses_count_free_route
    assert uses_count_free_route(model, H * W)
    with torch.no_grad():
        ref = _eager(model, bundle)
    out = model.get_outputs_for_camera_ray_bundle(bundle)
    for k in exact:
        got = out[k].reshape(H * W, -1)
        want = ref[k].reshape(H * W, -1)
        assert got.dtype == want.dtype and torch.equal(got, want), (k, (got.float() - want.float()).abs().max().item())
    for k in mapper_keys:
        assert k in out and k in ref, k
        assert (out[k].reshape(H * W, -1) - ref[k].reshape(H * W, -1)).abs().max().item() <= 1e-6, k
    assert set(out) == set(ref)
    return out, ref


def test_eval_render_bit_equal_default_config():
    _check_equal(_model(), _bundle())


def test_eval_render_bit_equal_cone0_linear_co_map_mlp_mappers(monkeypatch):
    from lsenerf_amd import model as M
    monkeypatch.setattr(M.MLP_Mapper, "init_steps", 60)
    monkeypatch.setattr(M.RGB_MLP_Mapper, "init_steps", 60)
    m = _model(cone_angle=0.0, use_mapping=True, mapping_method="rgb_mlp", map_mode="co_map", evs_mapping_method="mlp",
               ev_one_dim="learned")
    from lsenerf_amd.renderer import LinearRenderer
    assert isinstance(m.renderer_rgb, LinearRenderer)
    # co_map: "rgb" is the colour mapper's output; the render itself is "linear" (= max(radiance, 1e-5), elementwise)
    _check_equal(m, _bundle(seed=2), mapper_keys=("rgb", "ev_out", "ev_linear"),
                 exact=("linear", "accumulation", "depth", "num_samples_per_ray"))


@pytest.mark.parametrize("mode", ["zero", "mean", "param"])
def test_eval_render_bit_equal_embedding_modes(mode):
    from lsenerf_amd import LSEEmbeddingConfig
    m = _model(num_train_data=32, embed_config=LSEEmbeddingConfig(embedding_type="evs_emb", eval_mode=mode))
    with torch.no_grad():
        m.field.embedding_appearance.embedding.weight.normal_(0.0, 0.5)     # rows that differ: the modes differ
    if mode == "param":
        m.init_test_params()
    _check_equal(m, _bundle(seed=3))


def test_eval_render_bit_equal_white_background():
    _check_equal(_model(background_color="white"), _bundle(seed=4))


def test_eval_render_empty_middle_chunk_and_short_last_chunk():
    """Chunk 1 marches no sample at all: nerfstudio's fake sample lands on its first ray (one sample, depth clipped to t = 1); the
    last chunk has 192 rays."""
    out, _ = _check_equal(_model(), _bundle(seed=5, empty_chunk=1))
    ns = out["num_samples_per_ray"].reshape(-1)
    assert ns[CHUNK].item() == 1 and int(ns[CHUNK + 1:2 * CHUNK].sum().item()) == 0
    assert out["depth"].reshape(-1)[CHUNK].item() == 1.0
    assert int(ns[3 * CHUNK:].gt(0).sum().item()) > 0 and (H * W) % CHUNK != 0


def test_eval_render_matches_oracle_model():
    """The count-free eval render against the CPU oracle (tests/util.make_model_pair) chunk by chunk, within the bar the project holds
    whole model renders to (tests/util.compare_model_outputs: 5 x TOL_FWD, normalised max error)."""
    from lsenerf_amd import RayBundle
    from tests.util import make_model_pair
    # per-image embeddings in eval mode "zero" on both sides (the oracle's eval embedding is the zero / mean vector)
    hip, orc = make_model_pair(grid_levels=2, grid_resolution=32, seed=96, occupied_frac=0.5, emb_type="evs_emb")
    hip.config.eval_num_rays_per_chunk = CHUNK
    hip.eval()
    orc.training = False
    n = 600
    o, d = random_rays(n, seed=11)
    rb = RayBundle(origins=o.cuda(), directions=d.cuda(), camera_indices=torch.zeros(n, 1, dtype=torch.long, device="cuda"))
    out = hip.get_outputs_for_camera_ray_bundle(rb)
    refs = [orc.exec_get_outputs(o[lo:lo + CHUNK], d[lo:lo + CHUNK]) for lo in range(0, n, CHUNK)]
    ref = {k: torch.cat([r[k] for r in refs]) for k in ("rgb", "accumulation", "depth", "num_samples_per_ray")}
    assert torch.equal(out["num_samples_per_ray"].reshape(-1).cpu(), ref["num_samples_per_ray"].reshape(-1))
    for k in ("rgb", "accumulation", "depth"):
        err = nmax_err(out[k].reshape(n, -1).cpu(), ref[k].reshape(n, -1).detach(), 1e-3)
        assert err < 5 * TOL_FWD, (k, err)


def test_eval_render_makes_no_host_sync_per_chunk():
    """SYNC_STATS counts the sampler's count read-backs: the count-free route enqueues a four-chunk image without one; the eager
    eval loop makes at least one per chunk."""
    from lsenerf_amd import ops
    m, b = _model(), _bundle(seed=6)
    m.get_outputs_for_camera_ray_bundle(b)          # warm
    torch.cuda.synchronize()
    c0 = ops.SYNC_STATS["count"]
    m.get_outputs_for_camera_ray_bundle(b)
    assert ops.SYNC_STATS["count"] == c0
    with torch.no_grad():
        _eager(m, b)
    torch.cuda.synchronize()
    assert ops.SYNC_STATS["count"] - c0 >= (H * W + CHUNK - 1) // CHUNK


def test_eval_output_shapes_bundle_and_render_camera():
    from lsenerf_amd.cameras import EdCameras
    m = _model()
    out = m.get_outputs_for_camera_ray_bundle(_bundle(seed=7))
    for k, c in (("rgb", 3), ("accumulation", 1), ("depth", 1), ("num_samples_per_ray", 1)):
        assert tuple(out[k].shape) == (H, W, c), (k, out[k].shape)
    c2w = torch.tensor([[[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 2.5]]])
    cams = EdCameras(c2w, fx=30.0, fy=30.0, cx=W / 2, cy=H / 2, width=W, height=H)
    out = m.render_camera(cams, 0)
    for k, c in (("rgb", 3), ("accumulation", 1), ("depth", 1), ("num_samples_per_ray", 1)):
        assert tuple(out[k].shape) == (H, W, c), (k, out[k].shape)
    assert out["num_samples_per_ray"].sum().item() > 0 and out["accumulation"].max().item() > 0
    # the same rays through the bundle route; the bundle is built on the host and moved to the model's device by the call
    coords = cams.get_image_coords().reshape(-1, 2)
    rb = cams.generate_rays(torch.zeros(H * W, dtype=torch.long), coords)
    out2 = m.get_outputs_for_camera_ray_bundle(rb)
    for k in KEYS:
        assert torch.equal(out2[k].reshape(H, W, -1).to(out[k].device), out[k]), k


def _images(B, C, h, w, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        p = torch.rand(B, C, h, w, generator=g)
        t = (p + 0.2 * torch.randn(B, C, h, w, generator=g)).clamp(0, 1)
    else:   # structured: smooth gradients + a bright square, target slightly shifted and blurred, range 0.3 at an offset of 2
        yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
        base = 0.5 * xx + 0.3 * torch.sin(6 * yy)
        base[h // 4:h // 2, w // 4:w // 2] += 0.8
        p = base.expand(B, C, h, w).clone() + 0.02 * torch.rand(B, C, h, w, generator=g)
        t = torch.roll(p, shifts=(1, 2), dims=(2, 3)) * 0.9
        p, t = 2.0 + 0.3 * p, 2.0 + 0.3 * t
    return p.float().contiguous(), t.float().contiguous()


@pytest.mark.parametrize("B,C", [(1, 1), (1, 3), (2, 1), (2, 3)])
@pytest.mark.parametrize("hw", [(11, 11), (37, 53), (480, 640)])
@pytest.mark.parametrize("kind", ["random", "structured"])
def test_image_metrics_kernel_vs_numpy(B, C, hw, kind):
    from lsenerf_amd import ops
    h, w = hw
    p, t = _images(B, C, h, w, kind, seed=B * 7 + C * 3 + h)
    ssim, mse = ops.image_metrics(p.cuda(), t.cuda())
    assert ssim.dim() == 0 and mse.dim() == 0 and ssim.is_cuda and mse.is_cuda
    ref_ssim = ssim_numpy(p.numpy(), t.numpy(), ops.ssim_window().numpy())
    ref_mse = float(np.mean((p.numpy().astype(np.float64) - t.numpy().astype(np.float64)) ** 2))
    assert abs(ssim.item() - ref_ssim) <= 1e-5, (ssim.item(), ref_ssim)
    assert abs(mse.item() - ref_mse) <= 1e-6 * ref_mse, (mse.item(), ref_mse)
    ssim2, mse2 = ops.image_metrics(p.cuda(), t.cuda())
    assert torch.equal(ssim, ssim2) and torch.equal(mse, mse2)


def test_image_metrics_refuses_small_images():
    from lsenerf_amd import _lib, ops
    for shape in [(1, 3, 10, 64), (1, 3, 64, 10)]:
        x = torch.rand(*shape, device="cuda")
        with pytest.raises(_lib.LseHipError, match="H and W must be >= 11"):
            ops.image_metrics(x, x)


@pytest.mark.parametrize("masked", [False, True])
def test_get_image_metrics_and_images(masked):
    from lsenerf_amd import ops
    m = _model()
    out = m.get_outputs_for_camera_ray_bundle(_bundle(seed=8))
    g = torch.Generator().manual_seed(9)
    batch = {"image": torch.rand(H, W, 3, generator=g)}
    if masked:
        batch["msk"] = (torch.rand(H, W, generator=g) > 0.3).float()
    metrics, images = m.get_image_metrics_and_images(out, batch)
    gt = batch["image"].cuda()
    pred = out["rgb"]
    if masked:
        msk = batch["msk"].cuda()[..., None]
        gt, pred = gt * msk, pred * msk
    ssim, mse = ops.image_metrics(gt.permute(2, 0, 1)[None].contiguous(), pred.permute(2, 0, 1)[None].contiguous())
    assert metrics["ssim"] == ssim.item()
    assert metrics["psnr"] == pytest.approx(10 * math.log10(1 / mse.item()), rel=1e-6)
    assert ("lpips" in metrics) == bool(getattr(m.lpips, "available", True))
    assert set(images) == {"img", "accumulation", "depth", "err_map"}
    assert tuple(images["img"].shape) == (H, 2 * W, 3)
    assert torch.equal(images["img"][:, W:], out["rgb"])                  # the unmasked prediction
    for k in ("accumulation", "depth", "err_map"):
        assert tuple(images[k].shape) == (H, W, 3), k
        assert images[k].min().item() >= -1e-6 and images[k].max().item() <= 1 + 1e-6 or k == "err_map"
