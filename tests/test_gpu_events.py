"""``lsenerf_amd.events`` at model level, on the small model of tests/test_gpu_pointcloud.py seen from 7 poses of a short arc at
24 x 40 pixels in chunks of 256 rays: the planes against the torch expression on whole-camera renders, the stream and the
frames against the numpy twin (tests/events_ref.py) fed with the GPU's own planes -- all bit for bit.  The threshold comes from the
planes themselves (the median non-zero plane-to-plane change), so roughly half of the (pixel, interval) items fire."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import events_ref as er
from tests.util import random_binaries

pytestmark = pytest.mark.gpu

H, W = 24, 40
P = H * W
CHUNK = 256
N_POSES = 7
TIMES = 10.0 + 0.004 * np.arange(N_POSES, dtype=np.float64) ** 1.25
CAP_STEP = 127
KINDS = ("default", "co_map")


@functools.lru_cache(maxsize=None)
def _model(kind):
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig
    from lsenerf_amd import model as M
    torch.manual_seed(5)
    kw = {}
    if kind == "co_map":
        kw = dict(cone_angle=0.0, use_mapping=True, mapping_method="rgb_mlp", map_mode="co_map", evs_mapping_method="mlp",
                  ev_one_dim="learned")
    saved = M.MLP_Mapper.init_steps, M.RGB_MLP_Mapper.init_steps
    M.MLP_Mapper.init_steps = M.RGB_MLP_Mapper.init_steps = 60          # (the mappers' identity fit at construction: kept short)
    try:
        cfg = LSENeRFModelConfig(grid_levels=2, grid_resolution=32, eval_num_rays_per_chunk=CHUNK, log2_hashmap_size=14, **kw)
        m = LSENeRFModel(cfg, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 8).cuda()
    finally:
        M.MLP_Mapper.init_steps, M.RGB_MLP_Mapper.init_steps = saved
    with torch.no_grad():     # a table large enough for density and colour to vary from pixel to pixel and from pose to pose
        m.field.mlp_base_grid.params.uniform_(-0.5, 0.5, generator=torch.Generator(device="cuda").manual_seed(9))
    b = random_binaries(2, 32, 0.5, 5)
    m.occupancy_grid.binaries.copy_(b.cuda())
    m.occupancy_grid.occs.copy_(b.float().flatten().cuda() * 0.5)
    m.occupancy_grid._invalidate_occ_mean()
    return m.eval()


@functools.lru_cache(maxsize=None)
def _cameras():
    """7 cameras 2.5 from the centre on an arc of 0.3 rad about the y axis, looking at it (OpenGL frame: -z forward)."""
    from lsenerf_amd.cameras import EdCameras
    c2w = []
    for a in np.linspace(0.0, 0.3, N_POSES):
        c, s = math.cos(a), math.sin(a)
        c2w.append([[c, 0.0, s, 2.5 * s], [0.0, 1.0, 0.0, 0.1], [-s, 0.0, c, 2.5 * c]])
    return EdCameras(torch.tensor(c2w, dtype=torch.float32), fx=30.0, fy=30.0, cx=W / 2, cy=H / 2, width=W, height=H,
                     times=torch.zeros(N_POSES))


def _poses():
    return _cameras().camera_to_worlds.cuda().contiguous()


@functools.lru_cache(maxsize=None)
def _planes(kind):
    """The GPU's planes of the 7 poses (host copy, read-only), the threshold taken from them and the twin's run over them."""
    from lsenerf_amd.events import log_intensity_planes
    L = log_intensity_planes(_model(kind), _cameras(), _poses()).cpu().numpy()
    assert L.shape == (N_POSES, P) and L.dtype == np.float32 and np.isfinite(L).all()
    step = np.abs(np.diff(L.astype(np.float64), axis=0))
    thr = float(np.median(step[step > 0]))
    counts, ev, ref = er.append(L, TIMES, W, L[0], thr, thr, CAP_STEP)
    fired = float((counts != 0).mean())
    print(f"{kind}: threshold {thr:.6g}, {len(ev[2])} events, {fired:.3f} of the items fire, largest |count| {int(np.abs(counts).max())}")
    assert 0.05 < fired < 0.95, fired
    L.setflags(write=False)
    return L, thr, counts, ev, ref


def _same(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _same_stream(stream, ev, n=None):
    n = len(ev[2]) if n is None else n
    return len(stream) == n and (stream.H, stream.W) == (H, W) and all(
        _same(getattr(stream, k), w[:n]) for k, w in zip("xytp", ev))


@functools.lru_cache(maxsize=None)
def _eval_set():
    from lsenerf_amd import EvalSet
    return EvalSet("cuda", torch.zeros((N_POSES, H, W, 3), dtype=torch.uint8), _cameras())


@pytest.mark.parametrize("kind", KINDS)
def test_planes_are_the_loss_operand_of_whole_camera_renders(kind):
    """Bit for bit against the torch expression on the render of the same camera through the package's existing device route
    (``camera_bundle`` of an ``EvalSet`` + ``get_outputs_for_camera_ray_bundle``).  ``render_camera`` builds its rays on the host,
    which agree with the device's only within a tolerance (tests/test_gpu_eval_set.py): its planes are printed beside, not asserted."""
    from lsenerf_amd.eval_set import camera_bundle
    from lsenerf_amd.model import EPS, to_gray
    model = _model(kind)
    L = _planes(kind)[0]
    key = model._plan()["ev_key"]
    assert key == ("ev_out" if kind == "co_map" else "rgb")

    def operand(out):
        v = out[key].reshape(P, -1)
        assert v.shape[-1] == (1 if kind == "co_map" else 3)
        return torch.log((to_gray(v) if v.shape[-1] != 1 else v) + EPS).reshape(-1)
    for i in range(N_POSES):
        assert _same(operand(model.get_outputs_for_camera_ray_bundle(camera_bundle(_eval_set(), i))), L[i]), i
    host = operand(model.render_camera(_cameras(), 3)).cpu().numpy()
    print(f"{kind}: planes from host-built rays differ from the device's by at most {float(np.abs(host - L[3]).max()):.3g}")


@pytest.mark.parametrize("kind", KINDS)
def test_simulated_stream_is_the_twin_whatever_the_window(kind):
    model = _model(kind)
    L, thr, counts, ev, ref = _planes(kind)
    n = len(ev[2])
    for window in (2, 6):
        stream, ref_out, total = model.simulate_events(_cameras(), _poses(), TIMES, thr, window=window, cap_step=CAP_STEP, sort=False)
        assert total == n and _same_stream(stream, ev) and _same(ref_out, ref), window
    # a capacity below the count: dropped in order, the true total comes back
    cut, ref_cut, total = model.simulate_events(_cameras(), _poses(), TIMES, thr, window=2, cap_step=CAP_STEP, sort=False,
                                                max_events=n // 3)
    assert total == n and _same_stream(cut, ev, n // 3) and _same(ref_cut, ref)
    roomy, _, total = model.simulate_events(_cameras(), _poses(), TIMES, thr, window=4, cap_step=CAP_STEP, sort=False, max_events=n + 9)
    assert total == n and _same_stream(roomy, ev)
    # sorted: non-decreasing times, the same events, ties in stream order
    ordered, _, _ = model.simulate_events(_cameras(), _poses(), TIMES, thr, window=6, cap_step=CAP_STEP)
    order = np.argsort(ev[2], kind="stable")
    assert bool((ordered.t[1:] >= ordered.t[:-1]).all()) and _same_stream(ordered, [a[order] for a in ev])
    # a level given on entry, two thresholds
    ref0 = (L[0] + np.float32(2.5) * np.float32(thr)).astype(np.float32)
    c2, ev2, r2 = er.append(L, TIMES, W, ref0, thr, 1.5 * thr, 3)
    s2, ro2, t2 = model.simulate_events(_cameras(), _poses(), TIMES, thr, threshold_neg=1.5 * thr, window=3, cap_step=3, sort=False,
                                        ref=torch.from_numpy(ref0))
    assert t2 == len(ev2[2]) and _same_stream(s2, ev2) and _same(ro2, r2)


@pytest.mark.parametrize("kind", KINDS)
def test_predicted_frames_are_the_counts_between_their_poses(kind):
    from lsenerf_amd.events import accumulate_events, event_frame_metrics
    model = _model(kind)
    L, thr, _, _, _ = _planes(kind)
    poses = _poses()
    # S = 1: exactly the two poses of a frame, the level starting at the first
    pairs = torch.stack([poses[:-1], poses[1:]], dim=1)
    frames = model.predict_event_frames(_cameras(), pairs, thr, cap_step=CAP_STEP)
    assert frames.shape == (N_POSES - 1, H, W) and frames.dtype == torch.int32
    for k in range(N_POSES - 1):
        assert _same(frames[k].reshape(P), er.count(L[k:k + 2], L[k], thr, thr, CAP_STEP)[0][0]), k
    # S = 3: the summed counts, and the accumulated stream of the same poses wherever no event sits on the frame's end
    triples = torch.stack([poses[0:4], poses[3:7]])
    frames3 = model.predict_event_frames(_cameras(), triples, thr, cap_step=CAP_STEP)
    compared = 0
    for f, k0 in enumerate((0, 3)):
        counts, ev, _ = er.append(L[k0:k0 + 4], TIMES[k0:k0 + 4], W, L[k0], thr, thr, CAP_STEP)
        assert _same(frames3[f].reshape(P), counts.sum(0).astype(np.int32)), f
        stream, _, total = model.simulate_events(_cameras(), poses[k0:k0 + 4], TIMES[k0:k0 + 4], thr, cap_step=CAP_STEP)
        assert total == len(ev[2])
        acc = accumulate_events(stream, TIMES[[k0, k0 + 3]], dtype=torch.int32)
        assert acc.shape == (1, H, W) and acc.dtype == torch.int32
        on_end = ev[2] == TIMES[k0 + 3]
        clear = np.ones(P, bool)
        clear[ev[1][on_end].astype(np.int64) * W + ev[0][on_end]] = False
        compared += int(clear.sum())
        assert _same(acc.reshape(P).cpu().numpy()[clear], frames3[f].reshape(P).cpu().numpy()[clear]), f
        assert _same(accumulate_events(stream, TIMES[[k0, k0 + 3]]), acc.clamp(-128, 127).to(torch.int8))
    assert compared > P                                                    # most pixels have no event on a frame's end
    m = event_frame_metrics(frames3, frames3)
    assert m == {"mean_abs_diff": 0.0, "sign_agreement": 1.0}


def test_modes_and_settings_are_restored_and_nothing_is_trained():
    from lsenerf_amd import evaluation
    model = _model("default")
    cfg = model.config
    L, thr, counts, ev, ref = _planes("default")
    saved = cfg.eval_normals, cfg.eval_early_stop_eps
    seen = []
    render_flat = evaluation.render_flat

    def spy(m, rb, check_overflow=True):
        seen.append((m.config.eval_normals, m.training, check_overflow))
        return render_flat(m, rb, check_overflow=check_overflow)
    try:
        evaluation.render_flat = spy
        model.train()
        model.field.mlp_head.eval()                                        # a mixed state: every module gets its own mode back
        cfg.eval_normals = "world"
        modes = [m.training for m in model.modules()]
        with torch.enable_grad():
            stream, ref_out, total = model.simulate_events(_cameras(), _poses(), TIMES, thr, window=4, cap_step=CAP_STEP, sort=False)
            frames = model.predict_event_frames(_cameras(), _poses()[None, :3], thr)
        assert seen == [("off", False, False)] * (N_POSES + 3)            # every plane once, no normals pass, no read per pose
        assert (cfg.eval_normals, cfg.eval_early_stop_eps) == ("world", saved[1])
        assert [m.training for m in model.modules()] == modes and model.training
        assert _same_stream(stream, ev) and total == len(ev[2]) and _same(ref_out, ref)
        assert not stream.t.requires_grad and all(p.grad is None for p in model.parameters())
        assert _same(frames.reshape(P), er.count(L[:3], L[0], thr, thr, CAP_STEP)[0].sum(0).astype(np.int32))
        # the early-stop route renders the planes too (the normals setting alone would refuse it)
        cfg.eval_early_stop_eps = 1e-4
        early, _, _ = model.simulate_events(_cameras(), _poses()[:3], TIMES[:3], thr, cap_step=CAP_STEP)
        assert len(early) > 0 and (cfg.eval_normals, cfg.eval_early_stop_eps) == ("world", 1e-4)
        # a failure inside still restores everything
        def broken(m, rb, check_overflow=True):
            raise RuntimeError("no more poses")
        evaluation.render_flat = broken
        with pytest.raises(RuntimeError, match="no more poses"):
            model.simulate_events(_cameras(), _poses(), TIMES, thr)
        assert (cfg.eval_normals, cfg.eval_early_stop_eps) == ("world", 1e-4) and [m.training for m in model.modules()] == modes
    finally:
        evaluation.render_flat = render_flat
        cfg.eval_normals, cfg.eval_early_stop_eps = saved
        model.eval()
    model.occupancy_grid.check_deferred_overflow()


def test_spline_event_poses_are_the_splines_event_cameras():
    from lsenerf_amd.cameras import CameraOptimizerConfig, EdCameras, SplineCameraOptimizer
    from lsenerf_amd.events import spline_event_poses
    cams = _cameras()
    timed = EdCameras(cams.camera_to_worlds, fx=30.0, fy=30.0, cx=W / 2, cy=H / 2, width=W, height=H,
                      times=torch.from_numpy(TIMES).float())
    dM = torch.eye(4)
    dM[0, 3] = 0.05
    spline = SplineCameraOptimizer(CameraOptimizerConfig(mode="off", optim_type="spline"), N_POSES, "cpu", timed, dM=dM)
    at = torch.tensor([float(TIMES[0]), float(TIMES[2]) + 1e-3, float(TIMES[-1])])
    poses = spline_event_poses(spline, at)
    assert poses.shape == (3, 3, 4) and poses.dtype == torch.float32 and poses.is_contiguous() and not poses.requires_grad
    assert torch.equal(poses, spline.get_evs_cameras(at).detach().float())
    assert float((poses[0] - (torch.cat([cams.camera_to_worlds[0], torch.tensor([[0.0, 0, 0, 1]])]) @ dM)[:3]).abs().max()) < 1e-4
