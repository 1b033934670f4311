"""The kernels of csrc/tsdf.hip and the masked surface nets of csrc/mesh.hip against the numpy twin (tests/tsdf_ref.py), bit for bit
(int32 views compared): integration over lattices whose point counts are no multiple of 64 with cameras that leave points behind
them, outside the image, on see-through pixels and on pixels without a usable depth; batches against single views; the masked nets
on fused volumes and on a field with scattered NaN; the fused vertex colours."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import mesh_ref as mr
from tests import tsdf_ref as tr

pytestmark = pytest.mark.gpu

LO, HI = (-1.0, -0.8, -0.9), (0.9, 1.0, 1.1)
H, W = 32, 24
CAMS = {
    "pinhole": tr.Camera(fx=30.0, fy=28.0, cx=9.3, cy=17.8, H=H, W=W),                                    # an offset principal point
    "distorted": tr.Camera(fx=30.0, fy=28.0, cx=11.5, cy=15.5, H=H, W=W, dist=(0.12, -0.03, 0.0, 0.0, 0.004, -0.006)),
    "narrow": tr.Camera(fx=160.0, fy=160.0, cx=11.5, cy=15.5, H=H, W=W),                                  # most points miss the image
}
EYES = [(2.2, 0.1, 0.0), (0.75, 0.3, 0.2), (-1.4, 1.5, 0.8), (0.2, -0.4, -2.2), (-0.9, -1.6, 1.1)]      # the second is inside the box


def _i32(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32)


@functools.lru_cache(maxsize=None)
def _views(cam_name):
    """(poses, depth, acc, rgb) of the five views, as read-only numpy arrays: the sphere's renders with see-through pixels (the
    misses, and hits with a low accumulation) and pixels whose depth is 0, negative, NaN or +inf."""
    cam = CAMS[cam_name]
    poses = np.stack([tr.look_at(e, tr.CENTRE) for e in EYES])
    depth, acc, rgb = tr.render_views(cam, poses)
    rng = np.random.default_rng(4)
    r = rng.random(depth.shape)
    acc[(r < 0.10) & (acc > 0)] = 0.3
    acc[(r >= 0.10) & (r < 0.14)] = np.nan
    for k, bad in enumerate((0.0, -0.7, np.nan, np.inf)):
        depth[(r >= 0.2 + 0.04 * k) & (r < 0.24 + 0.04 * k)] = bad
    for a in (poses, depth, acc, rgb):
        a.setflags(write=False)
    return poses, depth, acc, rgb


def _cam_desc(cam):
    from lsenerf_amd import ops
    return ops.camera_desc(cam.fx, cam.fy, cam.cx, cam.cy, cam.H, cam.W, cam.dist if cam.distort else None)


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()             # (the cached inputs are read-only)


@pytest.mark.parametrize("carve", [True, False])
@pytest.mark.parametrize("res", [(13, 9, 17), (1, 1, 1)])
@pytest.mark.parametrize("cam_name", ["pinhole", "distorted", "narrow"])
def test_integrate_is_the_twin_however_the_views_are_batched(cam_name, res, carve):
    from lsenerf_amd import ops, tsdf
    cam = CAMS[cam_name]
    poses, depth, acc, rgb = _views(cam_name)
    desc = _cam_desc(cam)
    r2 = tr.border_r2_max(cam)
    got_r2 = tsdf.border_r2_max(desc)
    assert got_r2 == r2 == float("inf") if not cam.distort else abs(got_r2 - r2) < 1e-4 * r2
    r2 = float(np.float32(got_r2))
    trunc = 0.3
    kw = dict(truncation=trunc, min_acc=0.5, carve=carve, r2_max=r2)
    want_tw, want_cw = tr.integrate(*tr.new_state(res), res, LO, HI, cam, poses, depth, acc, rgb, **kw)
    n = want_tw.shape[0]
    d_poses, d_depth, d_acc, d_rgb = _dev(poses), _dev(depth), _dev(acc), _dev(rgb)
    results = []
    for batches in (((0, 5),), ((0, 2), (2, 4), (4, 5)), tuple((j, j + 1) for j in range(5))):
        tw = torch.zeros((n, 2), device="cuda")
        cw = torch.zeros((n, 4), device="cuda")
        for a, b in batches:
            ops.tsdf_integrate(tw, cw, res, LO, HI, desc, d_poses[a:b], d_depth[a:b], d_acc[a:b], d_rgb[a:b], **kw)
        results.append((tw, cw))
        assert np.array_equal(_i32(tw), _i32(want_tw)), (batches, int((_i32(tw) != _i32(want_tw)).sum()))
        assert np.array_equal(_i32(cw), _i32(want_cw)), (batches, int((_i32(cw) != _i32(want_cw)).sum()))
    for tw, cw in results[1:]:
        assert torch.equal(tw, results[0][0]) and torch.equal(cw, results[0][1])
    if res != (1, 1, 1):
        w = want_tw[:, 1]
        assert 0 < (w == 0).sum() < n and (want_cw[:, 3] > 0).any() and (want_tw[:, 0] < 1).any()      # the inputs reach every branch
        assert cam_name == "narrow" or w.max() >= 3
    # without a colour state, and without colours to fuse, the distances are the same and cw stays as it is
    tw = torch.zeros((n, 2), device="cuda")
    ops.tsdf_integrate(tw, None, res, LO, HI, desc, d_poses, d_depth, d_acc, d_rgb, **kw)
    assert np.array_equal(_i32(tw), _i32(want_tw))
    tw.zero_()
    cw = torch.full((n, 4), 0.25, device="cuda")
    ops.tsdf_integrate(tw, cw, res, LO, HI, desc, d_poses, d_depth, d_acc, None, **kw)
    assert np.array_equal(_i32(tw), _i32(want_tw)) and bool((cw == 0.25).all())
    # no views: the state is untouched
    before = results[0][0].clone()
    ops.tsdf_integrate(results[0][0], results[0][1], res, LO, HI, desc, d_poses[:0], d_depth[:0], d_acc[:0], d_rgb[:0], **kw)
    assert torch.equal(results[0][0], before)


# ---------------------------------------------------------------------------------------------------- masked surface nets
@functools.lru_cache(maxsize=None)
def _field(kind, res):
    """float32 [points], read-only: a twin-fused sphere volume's field (all five pinhole views, or the first alone) or the sphere
    with scattered non-finite values."""
    if kind == "nonfinite":
        s = mr.seeded_nonfinite(res)
    else:
        poses, depth, acc, rgb = _views("pinhole")
        m = 5 if kind == "fused5" else 1
        tw, _ = tr.integrate(tr.new_state(res)[0], None, res, LO, HI, CAMS["pinhole"], poses[:m], depth[:m], acc[:m], None, 0.3)
        s = tr.field(tw)
    s.setflags(write=False)
    return s


def _box(kind):
    return (mr.UNIT_LO, mr.UNIT_HI) if kind == "nonfinite" else (LO, HI)


@pytest.mark.parametrize("res", [(13, 9, 17), (20, 20, 20)])
@pytest.mark.parametrize("kind", ["fused5", "fused1", "nonfinite"])
def test_masked_surface_nets_are_the_twin(kind, res):
    from lsenerf_amd import ops
    s = _field(kind, res)
    lo, hi = _box(kind)
    want_v, want_t = tr.surface_nets(s, res, lo, hi, 0.0)
    assert want_v.shape[0] > 20 and want_t.shape[0] >= 12 and np.isnan(s).any()
    d_s = _dev(s)
    v, t, totals = ops.surface_nets(d_s, res, lo, hi, 0.0, skip_nan=True)
    assert totals.tolist() == [want_v.shape[0], want_t.shape[0] // 2]
    assert np.array_equal(_i32(v), _i32(want_v)) and np.array_equal(t.cpu().numpy(), want_t)
    # fixed capacities: rows beyond the totals stay unwritten, the totals are true
    cap_v, cap_q = want_v.shape[0] + 7, want_t.shape[0] // 2 + 5
    ws = torch.empty(ops.surface_nets_workspace_bytes(res), dtype=torch.uint8, device="cuda")
    tot = torch.empty(2, dtype=torch.int64, device="cuda")
    vb = torch.full((cap_v, 3), -7.0, device="cuda")
    tb = torch.full((2 * cap_q, 3), -7, dtype=torch.int32, device="cuda")
    ops.surface_nets_count(d_s, res, 0.0, ws, tot, skip_nan=True)
    ops.surface_nets_emit(d_s, res, lo, hi, 0.0, ws, vb, tb, skip_nan=True)
    assert tot.tolist() == [want_v.shape[0], want_t.shape[0] // 2]
    assert np.array_equal(_i32(vb[:want_v.shape[0]]), _i32(want_v)) and bool((vb[want_v.shape[0]:] == -7.0).all())
    assert np.array_equal(tb[:want_t.shape[0]].cpu().numpy(), want_t) and bool((tb[want_t.shape[0]:] == -7).all())
    # a capacity below the totals drops the rows beyond it and nothing else
    vs = torch.full((5, 3), -7.0, device="cuda")
    ts = torch.full((2 * 3, 3), -7, dtype=torch.int32, device="cuda")
    ops.surface_nets_emit(d_s, res, lo, hi, 0.0, ws, vs, ts, skip_nan=True)
    assert np.array_equal(_i32(vs), _i32(want_v[:5])) and np.array_equal(ts.cpu().numpy(), want_t[:6])


@pytest.mark.parametrize("kind,res", [("fused5", (13, 9, 17)), ("nonfinite", (20, 20, 20))])
def test_flags_zero_through_the_ex_entry_points_is_the_existing_pair(kind, res):
    from lsenerf_amd import _lib, ops
    s = _dev(_field(kind, res))
    lo, hi = _box(kind)
    v, t, totals = ops.surface_nets(s, res, lo, hi, 0.0)
    rv, rt = mr.surface_nets(_field(kind, res), res, lo, hi, 0.0)
    assert np.array_equal(_i32(v), _i32(rv)) and np.array_equal(t.cpu().numpy(), rt)
    ws = torch.zeros(ops.surface_nets_workspace_bytes(res), dtype=torch.uint8, device="cuda")
    tot = torch.zeros(2, dtype=torch.int64, device="cuda")
    v2, t2 = torch.empty_like(v), torch.empty_like(t)
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())
    c_lo, c_hi = ops._box3(lo, hi)
    st = ops._stream()
    _lib.call("lse_surface_nets_count_ex", ptr(s), *res, 0.0, 0, ptr(ws), ws.numel(), ptr(tot), st)
    _lib.call("lse_surface_nets_emit_ex", ptr(s), *res, c_lo, c_hi, 0.0, 0, ptr(ws), ws.numel(), v.shape[0], t.shape[0] // 2, ptr(v2),
              ptr(t2), st)
    assert torch.equal(tot, totals) and torch.equal(v2, v) and torch.equal(t2, t)
    assert v.shape[0] > tr.surface_nets(_field(kind, res), res, lo, hi, 0.0)[0].shape[0]          # and the mask does drop something


# ---------------------------------------------------------------------------------------------------- vertex colours
@pytest.mark.parametrize("res", [(13, 9, 17), (20, 20, 20), (1, 1, 1)])
def test_vertex_colours_are_the_twin(res):
    from lsenerf_amd import ops
    poses, depth, acc, rgb = _views("pinhole")
    tw, cw = tr.integrate(*tr.new_state(res), res, LO, HI, CAMS["pinhole"], poses, depth, acc, rgb, 0.3)
    v, _ = tr.surface_nets(tr.field(tw), res, LO, HI, 0.0)
    rng = np.random.default_rng(1)
    extra = np.float32([HI, LO, (HI[0], 0.1, 0.2), (0.3, HI[1], HI[2]), (2.0, -3.0, 0.0), (np.nan, 0.0, 0.0)])      # on and outside the box
    inside = (np.float32(LO) + rng.random((64, 3)).astype(np.float32) * (np.float32(HI) - np.float32(LO))).astype(np.float32)
    vtx = np.concatenate([v, extra, inside]).astype(np.float32)
    want = tr.vertex_colors(cw, res, LO, HI, vtx)
    assert res == (1, 1, 1) or ((want != 0).any() and (want == 0).all(axis=1).any())          # coloured and colourless vertices
    d_cw, d_v = _dev(cw), _dev(vtx)
    got = ops.tsdf_vertex_colors(d_cw, res, LO, HI, d_v)
    assert np.array_equal(_i32(got), _i32(want)), int((_i32(got) != _i32(want)).sum())
    # rows beyond n_dev are untouched
    m = vtx.shape[0] // 2
    out = torch.full((vtx.shape[0], 3), -7.0, device="cuda")
    ops.tsdf_vertex_colors(d_cw, res, LO, HI, d_v, out=out, n_dev=torch.tensor([m], dtype=torch.int64, device="cuda"))
    assert np.array_equal(_i32(out[:m]), _i32(want[:m])) and bool((out[m:] == -7.0).all())
    assert ops.tsdf_vertex_colors(d_cw, res, LO, HI, d_v[:0]).shape == (0, 3)
