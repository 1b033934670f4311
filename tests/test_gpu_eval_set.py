"""A whole eval set on the GPU (lsenerf_amd.eval_set): lse_camera_rays against EdCameras.generate_rays and, bit for bit, against the
batch composer; lse_eval_image_prep against the torch expressions of image_metrics_and_images; lse_log_scale_correct against the
float64 twin of tests/test_eval_set_cpu.py; evaluate_set against the per-image route, and its host waits."""
import math

import numpy as np
import pytest
import torch

from tests.test_eval_set_cpu import scale_fit_f64, seeded_pair
from tests.test_gpu_eval import CHUNK, H, W, _model
from tests.util import TOL_FWD, nmax_err

pytestmark = pytest.mark.gpu

N_IMG = 3
DIST = (0.1, -0.05, 0.01, 0.0, 1e-3, -2e-3)
RANGES = [(0, 960), (0, 1), (959, 1), (37, 63), (40, 65), (255, 257)]
SENTINEL = -7.5


def _look_at(pos):
    """[3, 4] pose of a camera at ``pos`` looking at the origin (OpenGL frame: -z forward, y up)."""
    pos = torch.tensor(pos, dtype=torch.float64)
    back = pos / pos.norm()
    up = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64) if abs(float(back[1])) < 0.9 else torch.tensor([0.0, 0.0, 1.0],
                                                                                                           dtype=torch.float64)
    right = torch.linalg.cross(up, back)
    right = right / right.norm()
    up = torch.linalg.cross(back, right)
    return torch.stack([right, up, back, pos], dim=1).float()


def _cameras(dist=None):
    from lsenerf_amd.cameras import EdCameras
    c2w = torch.stack([_look_at(p) for p in ((0.3, 0.2, 2.5), (2.4, -0.4, 0.7), (-0.5, 2.3, -0.9))])
    return EdCameras(c2w, fx=30.0, fy=31.0, cx=W / 2 - 0.25, cy=H / 2 + 0.5, width=W, height=H,
                     times=torch.tensor([0.0, 0.5, 1.0]), distortion_params=None if dist is None else torch.tensor(dist))


def _images(seed=0, masked=None):
    g = torch.Generator().manual_seed(seed)
    images = torch.randint(0, 256, (N_IMG, H, W, 3), generator=g, dtype=torch.uint8)
    msk = None
    if masked == "u8":
        msk = (torch.rand(N_IMG, H, W, generator=g) > 0.3).to(torch.uint8)
    elif masked == "f32":
        msk = (torch.rand(N_IMG, H, W, generator=g) > 0.3).float()
    return images, msk


def _eval_set(masked=None, dist=None, seed=0):
    from lsenerf_amd import EvalSet
    images, msk = _images(seed, masked)
    return EvalSet("cuda", images, _cameras(dist), msk=msk, appearance_ids=[1, 2, 3]), images, msk


# ---------------------------------------------------------------------------------------------------- rays
@pytest.fixture(scope="module", params=[False, True], ids=["pinhole", "distorted"])
def ray_refs(request):
    """Per lens: the eval set, the host rays of every pixel of camera 1 (EdCameras.generate_rays) and the composer's rays of the
    same pixels from the same pose table -- computed once, read by every range."""
    from lsenerf_amd.data import BatchComposer, DeviceScene
    dist = DIST if request.param else None
    s, images, _ = _eval_set(dist=dist)
    cams = s.cameras
    cam = 1
    coords = cams.get_image_coords().reshape(-1, 2)
    host = cams.generate_rays(torch.full((H * W,), cam, dtype=torch.long), coords)
    scene = DeviceScene.from_arrays("cuda", col_images=images, col_cameras=cams, col_appearance_ids=[1, 2, 3])
    comp = BatchComposer(scene, H * W, 0, seed=0, num_embd=8)
    comp.set_poses(col=s.poses)
    idx = torch.cat([torch.full((H * W, 1), cam, dtype=torch.long), coords.long()], dim=1)
    (col, _, _), _ = comp.compose(indices=(idx, None))
    composed = {"origins": col.origins.clone(), "directions": col.directions.clone(), "pixel_area": col.pixel_area.clone(),
                "directions_norm": col.metadata["directions_norm"].clone()}
    assert s.cam_desc.distort == int(request.param)
    return s, cam, host, composed


@pytest.mark.parametrize("first,n", RANGES)
def test_camera_rays_equal_host_rays_and_the_composer_bit_for_bit(ray_refs, first, n):
    from lsenerf_amd import ops
    s, cam, host, composed = ray_refs
    pad = 70                                             # rows behind [0, n): must keep the sentinel
    out = tuple(torch.full((n + pad, w), SENTINEL, device="cuda") for w in (3, 3, 1, 1))
    got = ops.camera_rays(s.cam_desc, s.poses[cam], first, n, out=out)
    assert all(g is o for g, o in zip(got, out))
    want_host = (host.origins, host.directions, host.pixel_area, host.metadata["directions_norm"])
    for name, g, hst in zip(("origins", "directions", "pixel_area", "directions_norm"), got, want_host):
        err = nmax_err(g[:n], hst[first:first + n])
        print(name, first, n, err)
        assert err < TOL_FWD, (name, err)
        assert torch.equal(g[:n].reshape(n, -1), composed[name][first:first + n].reshape(n, -1)), name
        assert bool((g[n:] == SENTINEL).all()), f"{name}: a row outside [0, {n}) was written"
    # allocated outputs: the same values
    fresh = ops.camera_rays(s.cam_desc, s.poses[cam], first, n)
    for g, f in zip(got, fresh):
        assert f.shape[0] == n and torch.equal(g[:n], f)


def test_camera_bundle_is_the_host_bundle(ray_refs):
    from lsenerf_amd.eval_set import camera_bundle
    s, cam, host, _ = ray_refs
    rb = camera_bundle(s, cam)                           # image i of this set is camera i
    assert tuple(rb.origins.shape) == (H, W, 3) and tuple(rb.camera_indices.shape) == (H, W, 1)
    assert nmax_err(rb.directions, host.directions) < TOL_FWD and nmax_err(rb.pixel_area, host.pixel_area) < TOL_FWD
    assert torch.equal(rb.camera_indices.reshape(-1, 1).cpu(), host.camera_indices)
    assert torch.equal(rb.times.reshape(-1, 1).cpu(), host.times)
    assert nmax_err(rb.metadata["directions_norm"], host.metadata["directions_norm"]) < TOL_FWD
    assert rb.metadata["appearance_id"].unique().tolist() == [cam + 1]
    # an optimised rig: new poses in the table move the rays
    before = rb.origins.clone()
    s.set_poses(s.poses + torch.tensor([0.0, 0.0, 0.0, 0.125], device="cuda"))
    assert torch.equal(camera_bundle(s, cam).origins, before + 0.125)
    s.set_poses(s.cameras.camera_to_worlds)


# ---------------------------------------------------------------------------------------------------- prep
@pytest.mark.parametrize("masked", [None, "u8", "f32"])
def test_prep_planes_equal_the_torch_expressions(masked):
    from lsenerf_amd import ops
    images, msk = _images(3, masked)
    g = torch.Generator().manual_seed(5)
    rgb = torch.rand(H * W, 3, generator=g).cuda()
    m = _model()
    for i in range(N_IMG):
        gt_u8 = images[i].cuda()
        mk = None if msk is None else msk[i].cuda()
        gt_pl, pr_pl, stats = ops.eval_image_prep(gt_u8, rgb, mk)
        assert stats is None
        image = (images[i].float() / 255.0).cuda()      # divided on the host, as a dataset hands it over (a true division)
        pred = rgb.reshape(H, W, 3)
        if mk is not None:
            image, pred = image * mk[..., None], pred * mk[..., None]
        assert torch.equal(gt_pl, torch.moveaxis(image, -1, 0)[None]) and torch.equal(pr_pl, torch.moveaxis(pred, -1, 0)[None])
        # a float32 ground truth is taken as it is
        gt_f, _, _ = ops.eval_image_prep((images[i].float() / 255.0).cuda(), rgb, mk)
        assert torch.equal(gt_f, gt_pl)
        # hence the metrics are today's, bit for bit
        ssim, mse = ops.image_metrics(gt_pl, pr_pl)
        batch = {"image": images[i].float() / 255.0}
        if msk is not None:
            batch["msk"] = msk[i]
        outputs = {"rgb": rgb.reshape(H, W, 3), "accumulation": torch.ones(H, W, 1, device="cuda"),
                   "depth": torch.ones(H, W, 1, device="cuda")}
        metrics, _ = m.get_image_metrics_and_images(outputs, batch)
        assert metrics["ssim"] == ssim.item() and metrics["psnr"] == (10.0 * torch.log10(1.0 / mse)).item()
    if masked is not None:
        assert 0 < int((gt_pl == 0).sum()) < gt_pl.numel()


# ---------------------------------------------------------------------------------------------------- scale correction
def _correct(gt, pred, msk):
    from lsenerf_amd import ops
    h, w = gt.shape[:2]
    rgb = torch.from_numpy(pred).cuda().reshape(h * w, 3)
    gt_pl, _, stats = ops.eval_image_prep(torch.from_numpy(gt).cuda(), rgb, None if msk is None else torch.from_numpy(msk).cuda(),
                                          event_stats=True)
    coef, corrected, gray = ops.log_scale_correct(gt_pl, rgb, stats)
    return coef, corrected, gray, gt_pl


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("hw", [(11, 11), (37, 53), (480, 640)])
def test_log_scale_correct_vs_float64_twin(hw, masked):
    h, w = hw
    gt, pred, msk = seeded_pair(h, w, seed=h + 2 * int(masked), masked=masked)
    coef, corrected, gray, gt_pl = _correct(gt, pred, msk)
    gt_m = gt if msk is None else gt * msk[..., None]                  # float32 product: the image the twin is fed
    assert np.array_equal(gt_pl[0].permute(1, 2, 0).cpu().numpy(), gt_m)
    a64, b64, corr64, gray64 = scale_fit_f64(gt_m, pred)
    a, b = (float(v) for v in coef.tolist())
    rel = float(np.max(np.abs(corrected.cpu().numpy().reshape(h, w).astype(np.float64) - corr64) / corr64))
    print(hw, masked, "a", a, a64, abs(a - a64), "b", b, b64, abs(b - b64), "corrected rel", rel)
    assert tuple(corrected.shape) == tuple(gray.shape) == (1, 1, h, w)
    assert abs(a - a64) <= 1e-6 and abs(b - b64) <= 1e-6
    assert rel <= 4e-6
    # the grey plane: three float32 products (weights rounded to float32) summed left to right, one rounding each; for channels
    # <= 1 that is at most 0.15 + 0.3 + 0.04 (products) + 0.3 + 0.3 (sums) + 0.3 (weights) = 1.4e-7
    assert float(np.max(np.abs(gray.cpu().numpy().reshape(h, w) - gray64))) <= 2.5e-7
    coef2, corrected2, gray2, _ = _correct(gt, pred, msk)
    assert torch.equal(coef, coef2) and torch.equal(corrected, corrected2) and torch.equal(gray, gray2)


def test_log_scale_correct_constant_prediction_takes_the_nan_rule():
    gt, pred, _ = seeded_pair(37, 53, seed=9, masked=False)
    pred[:] = 0.3
    coef, corrected, _, _ = _correct(gt, pred, None)
    want = float(np.float32(5 / 255))
    assert coef.tolist() == [want, want]
    assert bool(torch.isfinite(corrected).all())


# ---------------------------------------------------------------------------------------------------- the whole set
@pytest.mark.parametrize("eps", [0.0, 1e-4])
def test_evaluate_set_equals_the_per_image_route(eps):
    from lsenerf_amd import ops
    from lsenerf_amd.eval_set import camera_bundle
    from lsenerf_amd.evaluation import uses_count_free_route
    m = _model(eval_early_stop_eps=eps, eval_segment_samples=64)
    assert uses_count_free_route(m, H * W)
    s, images, msk = _eval_set(masked="f32", seed=11)
    seen = []
    average, per_image = m.evaluate_set(s, on_image=lambda i, out, imgs: seen.append((i, set(imgs), tuple(imgs["img"].shape))))
    assert seen == [(i, {"img", "accumulation", "depth", "err_map"}, (H, 2 * W, 3)) for i in range(N_IMG)]
    has_lpips = bool(getattr(m.lpips, "available", True))
    keys = {"psnr", "ssim"} | ({"lpips"} if has_lpips else set())
    assert len(per_image) == N_IMG and all(set(r) == keys for r in per_image)
    assert set(average) == keys | {"num_rays_per_sec", "fps"} and average["fps"] > 0
    rgbs = []
    for i in range(N_IMG):
        out = m.get_outputs_for_camera_ray_bundle(camera_bundle(s, i))
        assert tuple(out["rgb"].shape) == (H, W, 3) and int(out["num_samples_per_ray"].sum()) > 0
        metrics, _ = m.get_image_metrics_and_images(out, {"image": images[i].float() / 255.0, "msk": msk[i]})
        assert per_image[i]["psnr"] == metrics["psnr"] and per_image[i]["ssim"] == metrics["ssim"], (i, per_image[i], metrics)
        rgbs.append(out["rgb"].reshape(H * W, 3).contiguous())
    assert len({r["ssim"] for r in per_image}) == N_IMG                        # three different images
    for k in ("psnr", "ssim"):
        mean = float(np.mean(np.array([r[k] for r in per_image], dtype=np.float32)))
        assert average[k] == pytest.approx(mean, rel=1e-6)
    # the event-only metric: the rows are image_metrics on the correction kernel's planes
    ev_average, ev_rows = m.evaluate_set(s, events_only=True)
    assert all(set(r) == keys for r in ev_rows)
    for i in range(N_IMG):
        gt_pl, _, stats = ops.eval_image_prep(s.data.images[i], rgbs[i], s.data.msk[i], event_stats=True)
        _, corrected, gray = ops.log_scale_correct(gt_pl, rgbs[i], stats)
        ssim, mse = ops.image_metrics(gray, corrected)
        assert ev_rows[i]["ssim"] == ssim.item() and ev_rows[i]["psnr"] == (10.0 * torch.log10(1.0 / mse)).item()
        assert ev_rows[i]["ssim"] != per_image[i]["ssim"] and ev_rows[i]["psnr"] != per_image[i]["psnr"]
    for k in ("psnr", "ssim"):
        mean = float(np.mean(np.array([r[k] for r in ev_rows], dtype=np.float32)))
        assert ev_average[k] == pytest.approx(mean, rel=1e-6)


def test_evaluate_set_waits_once_and_still_reports_an_overflow(monkeypatch):
    """Nothing waits for the device from the first image up to the one overflow read behind the last (torch's sync debug mode is
    at "error" until then), no sampler read-back (ops.SYNC_STATS), and a truncated ray of any image still raises."""
    from lsenerf_amd import eval_set as es, ops
    m = _model()
    s, _, _ = _eval_set(masked="u8", seed=12)
    for events_only in (False, True):
        m.evaluate_set(s, events_only=events_only)      # warm
    torch.cuda.synchronize()
    grid = m.occupancy_grid
    orig, reached = grid.check_deferred_overflow, []

    def overflow_read():
        reached.append(torch.cuda.get_sync_debug_mode())
        torch.cuda.set_sync_debug_mode("default")
        orig()
    monkeypatch.setattr(grid, "check_deferred_overflow", overflow_read)
    for events_only in (False, True):
        del reached[:]
        c0 = ops.SYNC_STATS["count"]
        torch.cuda.set_sync_debug_mode("error")
        try:
            _, rows = m.evaluate_set(s, events_only=events_only)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert reached == [2]                            # reached once for the three images, the mode still at "error"
        assert ops.SYNC_STATS["count"] == c0
        assert len(rows) == N_IMG and all(math.isfinite(r["psnr"]) for r in rows)
    # a short direction in the middle image: the capacity bound assumes unit length, the ray is truncated and flagged.  (Constant
    # steps through a fully occupied grid, as in tests/test_gpu_deferred.py: a quarter-length direction then needs four times the
    # samples of the bound.)
    m = _model(cone_angle=0.0, alpha_thre=0.0)
    m.occupancy_grid.binaries.fill_(True)
    grid = m.occupancy_grid
    orig = grid.check_deferred_overflow
    monkeypatch.setattr(grid, "check_deferred_overflow", overflow_read)
    bundle = es.camera_bundle

    def short_bundle(eval_set, i):
        rb = bundle(eval_set, i)
        if i == 1:
            rb.directions = rb.directions * 0.25
        return rb
    monkeypatch.setattr(es, "camera_bundle", short_bundle)
    del reached[:]
    with pytest.raises(RuntimeError, match="shorter than 1"):
        m.evaluate_set(s)
    assert len(reached) == 1
    monkeypatch.setattr(es, "camera_bundle", bundle)
    m.evaluate_set(s)                                    # reported once, then clear
