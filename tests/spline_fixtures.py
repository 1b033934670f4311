"""Shared by tests/test_spline_dev_cpu.py and tests/test_gpu_spline_dev.py: the spline fixtures, their conditions, and the float64
restatement of the spline pose path of cameras.py that the kernels of csrc/spline.hip are held against (it never sees a kernel)."""
import copy

import torch

from tests.test_compose_cpu import COL_HW, COL_TIMES, EVS_TIMES, N_COL, _cams

SCALE = 1.3


# ---------------------------------------------------------------------------------------------------- fixtures
def rel_pose():
    """A non-trivial rgb -> event camera pose dM (4x4): a rotation of ~15 degrees and a baseline."""
    from lsenerf_amd import cameras as cam
    return cam.hom_exp_map_SO3xR3(torch.tensor([[0.05, -0.02, 0.03, 0.1, 0.2, -0.15]]))[0]


def make_spline(cams, factor=1, exp_t=0.3, scale=SCALE, scheme="active", mode="SO3xR3"):
    from lsenerf_amd import cameras as cam
    cfg = cam.CameraOptimizerConfig(mode=mode, optim_type="spline", exp_t=exp_t, control_pnt_factor=factor, scheme=scheme)
    spl = cfg.setup(num_cameras=len(cams), device="cpu", cameras=cams, dM=rel_pose())
    with torch.no_grad():
        spl.scale.fill_(scale)
    return spl


def _synthetic_spline(tangents):
    """A spline with GIVEN control tangents [K, 6] at control times 0, 1, ..., K - 1 (built over K throw-away cameras)."""
    K = len(tangents)
    spl = make_spline(_cams(K, COL_HW, 11, [float(i) for i in range(K)], 31.0))
    assert spl.ctrl_tangents.shape == (K, 6)
    with torch.no_grad():
        spl.ctrl_tangents.copy_(torch.as_tensor(tangents, dtype=torch.float32))
    return spl


def _k5():
    """K = 5, 300 queries (a control point's list is longer than one wave): a flipped pair (rotation vectors (0, 0, 3) and
    (0, 0, -3): dot = cos 3 < 0), a rotation vector that is exactly zero, a pair 2.1 degrees apart (lerp) and pairs far apart."""
    spl = _synthetic_spline([[0.3, -0.2, 0.1, 0.0, 0.0, 3.0], [0.5, 0.1, -0.3, 0.0, 0.0, -3.0], [-0.4, 0.6, 0.2, 0.0, 0.0, 0.0],
                             [0.1, 0.9, -0.7, 0.03, 0.01, -0.02], [2.5, -3.5, 1.0, 0.5, -0.4, 0.3]])
    g = torch.Generator().manual_seed(3)
    rnd = lambda n: torch.rand(n, generator=g) * 5.0 - 0.5               # beyond both ends
    col = rnd(50)
    col[:5] = torch.tensor([0.0, 1.0, 2.0, 3.0, 4.0])                    # exactly at the control times, the last one too
    prev, nxt = rnd(60), rnd(40)
    prev[:2] = torch.tensor([4.0, 0.0])
    return spl, [("deblur", col), ("evs", prev), ("evs", nxt)], [(50, 4, 3, 4), (60, 3, 4), (40, 3, 4)]


def _k70():
    """K = 70, 130 queries (more control points than a wave or a block has lanes / waves): rotation vectors that walk in steps of
    ~0.02 rad (lerp) and ~0.3 rad (slerp); no query falls into [21, 40], so control points 22 .. 39 are on no list."""
    g = torch.Generator().manual_seed(5)
    step = torch.randn(70, 3, generator=g)
    step = step / step.norm(dim=1, keepdim=True) * torch.where(torch.arange(70) % 3 == 0, 0.3, 0.02)[:, None]
    rot = 0.4 * torch.randn(1, 3, generator=g) + torch.cumsum(step, 0) * torch.tensor([1.0, -1.0, 1.0])
    spl = _synthetic_spline(torch.cat([torch.rand(70, 3, generator=g) * 8.0 - 4.0, rot], 1))

    def rnd(n):
        t = torch.rand(n, generator=g) * 50.0 - 0.5
        return torch.where(t > 21.0, t + 19.0, t)                         # [-0.5, 21] and [40, 68.5]
    col, prev = rnd(70), rnd(60)
    col[:3] = torch.tensor([69.0, 0.0, 45.0])
    prev[:2] = torch.tensor([69.0, 75.0])
    return spl, [("rgb", col), ("evs", prev), None], [(70, 1, 3, 4), (60, 3, 4), None]


def _scene_like(factor, deblur, prevnext):
    """The spline of make_scene's six colour cameras, queried like a composer over that scene queries it."""
    spl = make_spline(_cams(N_COL, COL_HW, 2, COL_TIMES, 31.0), factor=factor)
    col, evs = torch.tensor(COL_TIMES), torch.tensor(EVS_TIMES)
    G = 4 if deblur else 1
    if prevnext:
        return spl, [("deblur" if deblur else "rgb", col), ("evs", evs[:9]), ("evs", evs[1:10])], [(N_COL, G, 3, 4), (9, 3, 4), (9, 3, 4)]
    return spl, [("deblur" if deblur else "rgb", col), ("evs", evs), None], [(N_COL, G, 3, 4), (10, 3, 4), None]


FIXTURES = {"scene_f1_deblur_consec": lambda: _scene_like(1, True, False), "scene_f3_rgb_prevnext": lambda: _scene_like(3, False, True),
            "k5_q300": _k5, "k70_q130": _k70}


def pair_dots(spl):
    """float64 dot of the normalised quaternions of every adjacent control pair."""
    from lsenerf_amd import cameras as cam
    q = cam.exp_map_to_quat(spl.ctrl_tangents.detach().double()[:, 3:])
    q = q / q.norm(dim=1, keepdim=True)
    return (q[:-1] * q[1:]).sum(1)


def check_fixture(spl):
    """The fixture conditions: float32 and float64 take the same branches, translations lie within [-4, 4].  Returns the dots."""
    dots = pair_dots(spl)
    assert float(dots.abs().min()) >= 1e-3, float(dots.abs().min())
    assert float((dots.abs() - 0.9995).abs().min()) >= 1e-4, float((dots.abs() - 0.9995).abs().min())
    assert float(spl.ctrl_tangents.detach()[:, :3].abs().max()) <= 4.0
    return dots


# ---------------------------------------------------------------------------------------------------- float64 restatement
def tables_f64(spl64, segments, scale=None, ctrl=None):
    """The pose tables of ``segments`` in float64: ``get_rgb_cameras`` / ``get_evs_cameras`` / ``get_deblur_cameras`` restated with the
    pose maths of cameras.py (dtype-generic) on float64 parameters.  The one difference from calling them on a float64 copy:
    ``vectorized_generalized_interpolation`` casts its control poses to float32, which a float64 reference must not.  Times, index and
    fraction are float32 as cameras.py computes them (they are inputs of the kernels), then exact in float64."""
    from lsenerf_amd import cameras as cam
    ctrl = spl64.ctrl_tangents if ctrl is None else ctrl
    scale = spl64.scale if scale is None else scale
    ctrl_ts = spl64.ctrl_ts.float()
    out = []
    for seg in segments:
        if seg is None:
            out.append(None)
            continue
        kind, times = seg
        times = times.float()
        if kind == "deblur":
            delta = spl64.exp_t / (spl64.n_deblur_rays - 1)
            times = (times.reshape(-1, 1) - spl64.exp_t / 2 + (delta * torch.arange(spl64.n_deblur_rays))[None]).reshape(-1)
        ts = torch.clip(times, ctrl_ts[0], ctrl_ts[-1]).reshape(-1)
        idx = torch.clamp(torch.searchsorted(ctrl_ts, ts, right=True), 1, len(ctrl_ts) - 1) - 1
        t = ((ts - ctrl_ts[idx]) / (ctrl_ts[idx + 1] - ctrl_ts[idx])).double().unsqueeze(-1)
        poses = cam.exp_map_to_quat_map(ctrl)
        p0, p1 = poses[idx], poses[idx + 1]
        vec = torch.cat([(1 - t) * p0[:, :3] + t * p1[:, :3], cam.slerp(p0[:, 3:], p1[:, 3:], t)], dim=1)
        c2w = cam.quat_map_to_mtx(vec)[:, :3, :4]
        if kind == "evs":
            dM = spl64.dM.double()
            c2w = c2w @ torch.cat((dM[:, :3], torch.cat((dM[:3, 3:4] * scale, dM[3:, 3:4]), dim=0)), dim=1)
        out.append(c2w.reshape(-1, 4, 3, 4) if kind == "deblur" else c2w)
    return out


def tables_f32(spl, segments):
    """cameras.py itself (float32, differentiable): what ``spline_tables`` returns for cameras at the segments' times."""
    out = []
    for seg in segments:
        if seg is None:
            out.append(None)
            continue
        kind, times = seg
        if kind == "deblur":
            out.append(spl.get_deblur_cameras(times.reshape(-1, 1)).reshape(-1, 4, 3, 4))
        else:
            out.append({"rgb": spl.get_rgb_cameras, "evs": spl.get_evs_cameras}[kind](times.reshape(-1)))
    return out


def double_copy(spl):
    s = copy.deepcopy(spl).cpu()
    s.ctrl_tangents.data = s.ctrl_tangents.data.double()
    s.scale.data = s.scale.data.double()
    return s


def autograd_f64(spl, segments, d_tables):
    """``(d ctrl_tangents, d scale)`` in float64 from table gradients ``d_tables`` (one per segment, None where absent)."""
    s = double_copy(spl)
    tabs = tables_f64(s, segments)
    loss = sum((t.reshape(g.shape) * g.detach().cpu().double()).sum() for t, g in zip(tabs, d_tables) if t is not None)
    gc, gs = torch.autograd.grad(loss, [s.ctrl_tangents, s.scale], allow_unused=True)
    return gc, torch.zeros(1, dtype=torch.float64) if gs is None else gs


def autograd_f32(spl, segments, d_tables):
    """The same through cameras.py's own float32 expressions on the CPU: the baseline of the backward's bar."""
    s = copy.deepcopy(spl).cpu()
    tabs = tables_f32(s, segments)
    loss = sum((t.reshape(g.shape) * g.detach().cpu().float()).sum() for t, g in zip(tabs, d_tables) if t is not None)
    gc, gs = torch.autograd.grad(loss, [s.ctrl_tangents, s.scale], allow_unused=True)
    return gc, torch.zeros(1) if gs is None else gs


def random_table_grads(shapes, seed):
    """Random d tables with zero rows for some cameras (every fifth row)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for shape in shapes:
        if shape is None:
            out.append(None)
            continue
        d = torch.randn(shape, generator=g)
        d.reshape(-1, 12)[::5] = 0.0
        out.append(d)
    return out
