"""Fixtures of the device pose deltas (csrc/pose_delta.hip, lsenerf_amd.pose_delta_dev): parameter rows that visit every branch of the
two exponentials of cameras.py, and a float64 RESTATEMENT of ``data.camera_tables`` over them (Rodrigues written out entry by entry,
both branch points, the mask) that never sees a kernel.  tests/test_pose_delta_cpu.py holds the restatement to cameras.py in float64;
tests/test_gpu_pose_delta.py holds the kernels to the restatement."""
import torch

MODES = ("SO3xR3", "SE3")
COUNTS = (1, 65, 300)                     # one row; one past a wave; more than one block
# |w| of row c is MAGS[c % 8]; None: the whole row is exact zeros (the state training starts from).  Row 0 is 0.0101, the worst case
# of float32 cameras.py, so that the one-camera fixture is not trivial and the masked cameras {0, 7, C - 1} hide no magnitude
MAGS = (0.0101, None, 0.005, 0.011, 0.02, 0.3, 1.0, 3.1)
FIXTURES = [(mode, C) for mode in MODES for C in COUNTS]


def masked_cameras(C):
    return None if C == 1 else torch.tensor([0, 7, C - 1])


def make_params(C, seed=0):
    """float32 [C, 6] = (v, w): |w| by MAGS on random axes, translations uniform in +-3 (one row per eight at exactly +-3)."""
    g = torch.Generator().manual_seed(1000 + seed + C)
    axis = torch.randn(C, 3, generator=g, dtype=torch.float64)
    axis = axis / axis.norm(dim=1, keepdim=True)
    v = (torch.rand(C, 3, generator=g, dtype=torch.float64) * 2 - 1) * 3
    p = torch.zeros(C, 6, dtype=torch.float64)
    for c in range(C):
        m = MAGS[c % 8]
        if m is None:
            continue
        p[c, :3] = v[c]
        p[c, 3:] = axis[c] * m
        if c % 8 == 5:
            p[c, :3] = torch.tensor([3.0, -3.0, 3.0], dtype=torch.float64)
    return p.float()


def make_base(C, seed=0):
    """float32 [C, 3, 4]: random unit-quaternion rotations, translations uniform in +-4."""
    g = torch.Generator().manual_seed(2000 + seed + C)
    q = torch.randn(C, 4, generator=g, dtype=torch.float64)
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(C, 3, 3)
    t = (torch.rand(C, 3, 1, generator=g, dtype=torch.float64) * 2 - 1) * 4
    return torch.cat([R, t], 2).float()


def rot_norms(p):
    return p[:, 3:].double().norm(dim=1)


def check_fixture(p):
    """The rows meet the conditions they were chosen for (float32 values): on which side of both branch points they lie."""
    t2 = (p[:, 3:] * p[:, 3:]).sum(1)
    for c in range(p.shape[0]):
        m = MAGS[c % 8]
        if m is None:
            assert float(p[c].abs().max()) == 0.0
        else:
            assert (float(t2[c]) < 1e-4) == (m < 0.01), (c, m, float(t2[c]))
            assert abs(float(t2[c]) ** 0.5 - m) < 1e-6 * max(1.0, m)
    assert float(p[:, :3].abs().max()) <= 3.0


# ---------------------------------------------------------------------------------------------------- the restatement
def _rodrigues(a, b, w):
    """I + a hat(w) + b hat(w)^2, entry by entry: [N, 3, 3]."""
    x, y, z = w.unbind(1)
    rows = [1 - b * (y * y + z * z), b * x * y - a * z, b * x * z + a * y,
            b * x * y + a * z, 1 - b * (x * x + z * z), b * y * z - a * x,
            b * x * z - a * y, b * y * z + a * x, 1 - b * (x * x + y * y)]
    return torch.stack(rows, 1).reshape(-1, 3, 3)


def exp_map(p, mode):
    """``(R [N, 3, 3], t [N, 3])`` of tangent rows p = (v, w), in p's dtype, with the branches of cameras.py."""
    v, w = p[:, :3], p[:, 3:]
    t2 = (w * w).sum(1)
    if mode == "SO3xR3":
        th = t2.clamp(min=1e-4).sqrt()
        return _rodrigues(torch.sin(th) / th, (1 - torch.cos(th)) / th ** 2, w), v
    assert mode == "SE3", mode
    small = t2 < 1e-4
    th = torch.where(small, torch.ones_like(t2), t2).sqrt()
    a = torch.where(small, 1 - t2 / 6, torch.sin(th) / th)
    b = torch.where(small, 0.5 - t2 / 24, (1 - torch.cos(th)) / th ** 2)
    c = torch.where(small, 1.0 / 6 - t2 / 120, (th - torch.sin(th)) / th ** 3)
    V = _rodrigues(b, c, w)
    return _rodrigues(a, b, w), (V @ v[:, :, None])[:, :, 0]


def tables(p, base, mode, masked=None):
    """[C, 3, 4] = [R_corr R0 | t0 + t_corr]; a masked camera keeps (R0 | t0).  dtype of p; base is converted."""
    base = base.to(p.dtype)
    R, t = exp_map(p, mode)
    out = torch.cat([R @ base[:, :, :3], base[:, :, 3:] + t[:, :, None]], 2)
    if masked is not None:
        keep = torch.zeros(p.shape[0], dtype=torch.bool)
        keep[masked] = True
        out = torch.where(keep[:, None, None], base, out)
    return out


def tables_f64(p, base, mode, masked=None):
    return tables(p.detach().double(), base.double(), mode, masked)


def autograd_f64(p, base, mode, masked, d_table):
    """d p [C, 6] float64: autograd of the restatement at the (float32) values of p."""
    leaf = p.detach().double().requires_grad_(True)
    tables(leaf, base.double(), mode, masked).backward(d_table.double())
    return leaf.grad


# ---------------------------------------------------------------------------------------------------- cameras.py itself
def make_optimizer(p, mode, masked=None, dtype=torch.float32, device="cpu"):
    from lsenerf_amd import cameras as cam
    opt = cam.CameraOptimizer(cam.CameraOptimizerConfig(mode=mode), p.shape[0], device=device, non_trainable_camera_indices=masked)
    opt.pose_adjustment = torch.nn.Parameter(p.detach().to(dtype).to(device).clone())
    return opt


def make_cameras(base):
    from lsenerf_amd import cameras as cam
    return cam.EdCameras(base, 30.0, 30.0, 8.0, 6.0, 16, 12, times=torch.arange(base.shape[0], dtype=torch.float32))


def cameras_py(p, base, mode, masked, d_table, dtype):
    """``(tables, d p)`` of ``data.camera_tables`` over a ``CameraOptimizer`` in ``dtype`` on the CPU (``masked`` goes through
    ``non_trainable_camera_indices``)."""
    from lsenerf_amd.data import camera_tables
    opt = make_optimizer(p, mode, masked, dtype)
    cams = make_cameras(base)
    cams.camera_to_worlds = base.to(dtype)
    out = camera_tables(cams, opt)
    out.backward(d_table.to(dtype))
    return out.detach(), opt.pose_adjustment.grad.detach()


def random_table_grad(C, seed=7):
    return torch.randn(C, 3, 4, generator=torch.Generator().manual_seed(seed + C))


def baseline_rows(p, mode):
    """The rows float32 cameras.py is a fair baseline on: all for SO3xR3; for SE3 those with |w| outside (0.01, 0.1), where its
    (1 - cos t) / t^2 and (t - sin t) / t^3 do not cancel."""
    n = rot_norms(p)
    return torch.ones_like(n, dtype=torch.bool) if mode == "SO3xR3" else ~((n > 0.01) & (n < 0.1))
