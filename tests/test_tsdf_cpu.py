"""TSDF mesh export without a GPU: the new entry points are declared, bound and exported by both libraries and refuse bad arguments
before any launch; the numpy twin (tests/tsdf_ref.py) fuses analytic depth renders of a sphere into a mesh that stays within one
voxel edge of the sphere for 6, 1 and 3 views -- which the unmasked surface nets do not --, is closed for 6 views and open for
one; the twin is batch-invariant; and the masked nets and the colour blend keep their stated edge cases."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import mesh_ref as mr
from tests import tsdf_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lse_tsdf_integrate", "lse_surface_nets_count_ex", "lse_surface_nets_emit_ex", "lse_tsdf_vertex_colors")
LO, HI = mr.UNIT_LO, mr.UNIT_HI
RES = 24
H_EDGE = 2.0 / RES                  # the voxel edge h = 1 / 12
TRUNC = 3 * H_EDGE
CAM = tr.Camera(fx=40.0, fy=40.0, cx=23.5, cy=23.5, H=48, W=48)
DIST = 2.2
AXIS6 = [(DIST, 0, 0), (-DIST, 0, 0), (0, DIST, 0), (0, -DIST, 0), (0, 0, DIST), (0, 0, -DIST)]
OBLIQUE3 = [tuple(DIST * np.asarray(d) / np.linalg.norm(d)) for d in ((1.0, 1.0, 1.0), (-1.0, 0.6, 0.5), (0.3, -1.0, 0.8))]
SCENES = {"six": AXIS6, "one": AXIS6[:1], "oblique": OBLIQUE3}


def _libs():
    from lsenerf_amd import _lib
    return [_lib.load(), _lib._load_dev()]


# ---------------------------------------------------------------------------------------------------- ABI and refusals
def test_symbols_are_declared_bound_and_exported_by_both_libraries():
    from lsenerf_amd import _lib, ops
    hdr_full = open(os.path.join(ROOT, "include", "lse_hip.h")).read()
    assert "TSDF fusion" in hdr_full
    hdr = re.sub(r"/\*.*?\*/", "", hdr_full, flags=re.S)
    for lib in _libs():
        assert lib.lse_abi_version() == _lib.LSE_ABI_VERSION == 6
        for name in NEW:
            assert re.search(r"\bint " + name + r"\s*\(", hdr), name
            assert name in _lib.SIGNATURES and hasattr(lib, name), name
            n_args = len(re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S).group(1).split(","))
            assert n_args == len(_lib.SIGNATURES[name]), name
    assert re.search(r"#define LSE_NETS_SKIP_NAN\s+1\b", hdr) and _lib.LSE_NETS_SKIP_NAN == 1
    for fn in ("tsdf_integrate", "tsdf_vertex_colors", "surface_nets"):
        assert callable(getattr(ops, fn))
    from lsenerf_amd import LSENeRFModel, tsdf
    assert callable(tsdf.export_tsdf_mesh) and callable(tsdf.TSDFVolume) and callable(LSENeRFModel.export_tsdf_mesh)


def _cam_desc(**kw):
    from lsenerf_amd import _lib
    f = dict(fx=40.0, fy=40.0, cx=11.5, cy=15.5, dist=(ctypes.c_float * 6)(), distort=0, H=32, W=24)
    f.update(kw)
    return _lib.CameraDesc(**f)


def test_bad_arguments_are_refused_before_any_launch():
    """Every call below fails a host-side check (LSE_E_INVALID = -1): none reaches a launch, so the dummy addresses are never read."""
    F3 = ctypes.c_float * 3
    lo, hi = F3(-1, -1, -1), F3(1, 1, 1)
    ptr, odd8, odd16 = ctypes.c_void_p(4096), ctypes.c_void_p(4100), ctypes.c_void_p(4104)
    big = 1 << 40
    cam = ctypes.byref(_cam_desc())
    inf, nan = float("inf"), float("nan")
    for lib in _libs():
        def integ(tw=ptr, cw=ptr, res=(4, 4, 4), lo_=lo, hi_=hi, cam_=cam, poses=ptr, n=2, depth=ptr, acc=ptr, rgb=ptr, trunc=0.25):
            return lib.lse_tsdf_integrate(tw, cw, *res, lo_, hi_, cam_, poses, n, depth, acc, rgb, trunc, 0.5, 1, inf, None)
        bad = []
        for res in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (2000, 2000, 2000), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)):
            bad += [integ(res=res), lib.lse_tsdf_vertex_colors(ptr, *res, lo, hi, ptr, 8, None, ptr, None),
                    lib.lse_surface_nets_count_ex(ptr, *res, 0.0, 1, ptr, big, ptr, None),
                    lib.lse_surface_nets_emit_ex(ptr, *res, lo, hi, 0.0, 1, ptr, big, 1, 1, ptr, ptr, None)]
        bad += [integ(n=-1), integ(trunc=0.0), integ(trunc=-1.0), integ(trunc=inf), integ(trunc=nan),
                integ(cam_=ctypes.byref(_cam_desc(fx=0.0))), integ(cam_=ctypes.byref(_cam_desc(fy=0.0))),
                integ(cam_=ctypes.byref(_cam_desc(H=0))), integ(cam_=ctypes.byref(_cam_desc(W=0))),
                integ(cam_=ctypes.byref(_cam_desc(W=-3))),
                integ(tw=None), integ(cam_=None), integ(lo_=None), integ(hi_=None), integ(poses=None), integ(depth=None),
                integ(acc=None), integ(tw=odd8), integ(cw=odd16), integ(cw=odd8),
                # the masked nets: what the plain pair refuses, and unknown flags
                lib.lse_surface_nets_count_ex(ptr, 4, 4, 4, 0.0, 2, ptr, big, ptr, None),
                lib.lse_surface_nets_count_ex(None, 4, 4, 4, 0.0, 1, ptr, big, ptr, None),
                lib.lse_surface_nets_count_ex(ptr, 4, 4, 4, 0.0, 1, ptr, 4 * 64 + 8 * 2 - 1, ptr, None),
                lib.lse_surface_nets_count_ex(ptr, 4, 4, 4, 0.0, 1, odd8, big, ptr, None),
                lib.lse_surface_nets_emit_ex(ptr, 4, 4, 4, lo, hi, 0.0, -1, ptr, big, 1, 1, ptr, ptr, None),
                lib.lse_surface_nets_emit_ex(ptr, 4, 4, 4, lo, hi, 0.0, 1, None, big, 1, 1, ptr, ptr, None),
                lib.lse_surface_nets_emit_ex(ptr, 4, 4, 4, lo, hi, 0.0, 1, ptr, big, -1, 1, ptr, ptr, None),
                lib.lse_surface_nets_emit_ex(ptr, 4, 4, 4, lo, hi, 0.0, 1, ptr, big, 1, 1, None, ptr, None),
                # vertex colours: a negative count, null or misaligned pointers
                lib.lse_tsdf_vertex_colors(ptr, 4, 4, 4, lo, hi, ptr, -1, None, ptr, None),
                lib.lse_tsdf_vertex_colors(None, 4, 4, 4, lo, hi, ptr, 8, None, ptr, None),
                lib.lse_tsdf_vertex_colors(odd8, 4, 4, 4, lo, hi, ptr, 8, None, ptr, None),
                lib.lse_tsdf_vertex_colors(ptr, 4, 4, 4, None, hi, ptr, 8, None, ptr, None),
                lib.lse_tsdf_vertex_colors(ptr, 4, 4, 4, lo, None, ptr, 8, None, ptr, None),
                lib.lse_tsdf_vertex_colors(ptr, 4, 4, 4, lo, hi, None, 8, None, ptr, None),
                lib.lse_tsdf_vertex_colors(ptr, 4, 4, 4, lo, hi, ptr, 8, None, None, None)]
        assert bad == [-1] * len(bad), bad
        assert lib.lse_last_error().decode().startswith("lse_tsdf_vertex_colors")
        # nothing to do is not an error and launches nothing; without colours cw and rgb may be null
        assert integ(n=0, poses=None, depth=None, acc=None, rgb=None) == 0
        assert integ(n=0, cw=None, rgb=None) == 0
        assert lib.lse_tsdf_vertex_colors(ptr, 4, 4, 4, lo, hi, None, 0, None, None, None) == 0


def test_ops_refuse_mismatched_tensors_on_the_host():
    from lsenerf_amd import ops
    res, lo, hi = (2, 2, 2), LO, HI
    cam = ops.camera_desc(40.0, 40.0, 3.5, 2.5, 6, 8)
    tw, cw = torch.zeros(27, 2), torch.zeros(27, 4)
    poses, depth, acc, rgb = torch.zeros(2, 3, 4), torch.zeros(2, 48), torch.zeros(2, 48), torch.zeros(2, 48, 3)
    call = lambda **kw: ops.tsdf_integrate(**{**dict(tw=tw, cw=cw, res=res, lo=lo, hi=hi, cam_desc=cam, poses=poses, depth=depth, acc=acc,
                                                     rgb=rgb, truncation=0.5), **kw})
    with pytest.raises(ValueError, match="tw: "):
        call(tw=torch.zeros(26, 2))
    with pytest.raises(ValueError, match="cw: "):
        call(cw=torch.zeros(27, 3))
    with pytest.raises(ValueError, match="poses"):
        call(poses=torch.zeros(2, 4, 4))
    with pytest.raises(ValueError, match="depth: "):
        call(depth=torch.zeros(2, 47))
    with pytest.raises(ValueError, match="acc: "):
        call(acc=torch.zeros(3, 48))
    with pytest.raises(ValueError, match="rgb: "):
        call(rgb=torch.zeros(2, 48))
    with pytest.raises(ValueError, match="truncation"):
        call(truncation=0.0)
    with pytest.raises(ValueError, match="tw: a float32"):
        call(tw=torch.zeros(27, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="depth must be contiguous"):
        call(depth=torch.zeros(48, 2).t())
    with pytest.raises(ValueError, match="tw must live on the GPU"):
        call()
    with pytest.raises(ValueError, match="cw"):
        ops.tsdf_vertex_colors(torch.zeros(27, 3), res, lo, hi, torch.zeros(5, 3))
    with pytest.raises(ValueError, match="vertices"):
        ops.tsdf_vertex_colors(cw, res, lo, hi, torch.zeros(5, 2))


def test_export_refuses_bad_arguments_before_touching_the_model():
    """The checks come before the first use of the model: a placeholder is never read."""
    from lsenerf_amd import tsdf

    class Field:
        aabb = torch.tensor([[-1.0, -1, -1], [1, 1, 1]])

    class Model:
        field = Field()

    views = (None, torch.zeros(2, 3, 4))
    for kw, match in ((dict(bounds=[[0, 0, 0], [1, 0, 1]]), "empty box"), (dict(resolution=0), "resolution"),
                      (dict(resolution=(4, 4)), "resolution"), (dict(truncation=0.0), "truncation"), (dict(truncation=-1.0), "truncation"),
                      (dict(views_per_launch=0), "views_per_launch"), (dict(colors="vertex"), "colors"),
                      (dict(image_indices=[2]), "image index"), (dict(image_indices=[-1]), "image index")):
        with pytest.raises(ValueError, match=match):
            tsdf.export_tsdf_mesh(Model(), views, **kw)


# ---------------------------------------------------------------------------------------------------- the sphere scene, twin alone
@functools.lru_cache(maxsize=None)
def _fused(scene):
    """(tw, cw) of the scene's views fused in one call.  Shared and never modified."""
    poses = np.stack([tr.look_at(e) for e in SCENES[scene]])
    depth, acc, rgb = tr.render_views(CAM, poses)
    tw, cw = tr.new_state(RES)
    tw, cw = tr.integrate(tw, cw, RES, LO, HI, CAM, poses, depth, acc, rgb, TRUNC)
    tw.setflags(write=False), cw.setflags(write=False)
    return tw, cw, (poses, depth, acc, rgb)


@pytest.mark.parametrize("scene", ["six", "one", "oblique"])
def test_masked_mesh_stays_within_one_voxel_edge_of_the_sphere(scene):
    """The bound is a condition -- one voxel edge h -- not a measurement; the unmasked nets on the same field break it for more
    than a tenth of their vertices (the second shell behind the truncation band), which is why the mode exists."""
    tw = _fused(scene)[0]
    sigma = tr.field(tw)
    v, t = tr.surface_nets(sigma, RES, LO, HI, 0.0)
    assert v.shape[0] > 100 and t.shape[0] > 100
    worst = float(tr.sphere_distance(v).max())
    v0, _ = tr.surface_nets(sigma, RES, LO, HI, 0.0, skip_nan=False)
    off = float((tr.sphere_distance(v0) > H_EDGE).mean())
    print("TSDF_TWIN", scene, "vertices", v.shape[0], "worst / h:", worst / H_EDGE, "| unmasked:", v0.shape[0], "beyond h:", off)
    assert worst <= H_EDGE
    assert off > 0.10


def test_six_views_close_the_mesh_and_one_view_leaves_it_open():
    v, t = tr.surface_nets(tr.field(_fused("six")[0]), RES, LO, HI, 0.0)
    assert mr.edge_imbalance(mr.directed_edges(t)) == 0
    assert (mr.undirected_edge_uses(mr.quad_directed_edges(t)) == 2).all()
    vol = mr.signed_volume(v, t)
    assert 0.8 * 4.0 / 3.0 * np.pi * tr.RADIUS ** 3 < vol < 1.1 * 4.0 / 3.0 * np.pi * tr.RADIUS ** 3      # positive: outward normals
    v, t = tr.surface_nets(tr.field(_fused("one")[0]), RES, LO, HI, 0.0)
    assert mr.edge_imbalance(mr.directed_edges(t)) > 0
    assert t.min() >= 0 and t.max() < v.shape[0]


def test_twin_is_batch_invariant():
    tw_all, cw_all, (poses, depth, acc, rgb) = _fused("six")
    tw, cw = tr.new_state(RES)
    for j in range(poses.shape[0]):
        tw, cw = tr.integrate(tw, cw, RES, LO, HI, CAM, poses[j:j + 1], depth[j:j + 1], acc[j:j + 1], rgb[j:j + 1], TRUNC)
    assert np.array_equal(tw.view(np.int32), tw_all.view(np.int32)) and np.array_equal(cw.view(np.int32), cw_all.view(np.int32))
    tw, cw = tr.new_state(RES)
    for a, b in ((0, 2), (2, 5), (5, 6)):
        tw, cw = tr.integrate(tw, cw, RES, LO, HI, CAM, poses[a:b], depth[a:b], acc[a:b], rgb[a:b], TRUNC)
    assert np.array_equal(tw.view(np.int32), tw_all.view(np.int32)) and np.array_equal(cw.view(np.int32), cw_all.view(np.int32))
    assert tw_all[:, 1].max() == 6 and tw_all[:, 1].min() >= 0 and cw_all[:, 3].max() >= 2
    # without a colour state the distances are the same
    tw2, none = tr.integrate(tr.new_state(RES)[0], None, RES, LO, HI, CAM, poses, depth, acc, rgb, TRUNC)
    assert none is None and np.array_equal(tw2.view(np.int32), tw_all.view(np.int32))


def test_field_min_weight_is_nan_exactly_below_it():
    tw = _fused("oblique")[0]
    f1, f2 = tr.field(tw, 1), tr.field(tw, 2)
    assert np.array_equal(np.isnan(f2), tw[:, 1] < 2) and np.array_equal(np.isnan(f1), tw[:, 1] < 1)
    assert 0 < np.isnan(f1).sum() < np.isnan(f2).sum() < f2.shape[0]
    seen = ~np.isnan(f2)
    assert np.array_equal(f2[seen].view(np.int32), (-tw[seen, 0]).view(np.int32))


def test_masked_nets_without_nan_are_the_plain_nets():
    for fld in ("sphere", "torus", "open_noise"):
        s = getattr(mr, fld)(RES)
        v, t = mr.surface_nets(s, RES, LO, HI, 0.0)
        vm, tm = tr.surface_nets(s, RES, LO, HI, 0.0)
        assert np.array_equal(v.view(np.int32), vm.view(np.int32)) and np.array_equal(t, tm)


def test_masked_nets_on_the_seeded_nonfinite_field():
    res = (13, 9, 17)
    s = mr.seeded_nonfinite(res)
    v, t, cells = tr.surface_nets(s, res, LO, HI, 0.0, with_cells=True)
    mixed, bad = tr.cell_masks(s, res)
    assert v.shape[0] == cells.shape[0] > 20 and t.shape[0] > 10
    assert mixed[cells].all() and not bad[cells].any()                      # no vertex belongs to a cell with a NaN corner
    assert np.array_equal(cells, np.flatnonzero(mixed & ~bad))              # and every active cell has one, in order
    assert t.min() >= 0 and t.max() < v.shape[0]                            # every quad's four cells are active
    v0, t0 = mr.surface_nets(s, res, LO, HI, 0.0)
    assert v.shape[0] < v0.shape[0] and t.shape[0] < t0.shape[0]
    # a quad is kept iff its four cells are: count them from the unmasked mesh
    v0c = np.flatnonzero(mixed)
    q0 = t0.reshape(-1, 6)[:, [0, 1, 2, 5]]
    assert t.shape[0] // 2 == int((~bad[v0c[q0]]).all(axis=1).sum())
    assert np.isfinite(v).all()


# 8 products, 16 additions and one division, each within half an ulp (2^-24 relative) of values below 1: under 32 x 2^-24
BLEND_EPS = 32 * 2.0 ** -24


def test_colour_twin_edge_cases():
    res = (3, 2, 4)
    n = 4 * 3 * 5
    rng = np.random.default_rng(0)
    vtx = (rng.random((200, 3)) * 2.4 - 1.2).astype(np.float32)             # some outside the box: clamped into the last cell
    vtx[0], vtx[1] = (1.0, 1.0, 1.0), (-1.0, -1.0, -1.0)
    cw = np.zeros((n, 4), dtype=np.float32)
    cw[:] = (0.25, 0.5, 0.75, 3.0)
    c = tr.vertex_colors(cw, res, LO, HI, vtx)
    assert c.dtype == np.float32 and np.abs(c - np.float32([0.25, 0.5, 0.75])).max() <= BLEND_EPS      # a constant volume
    # zero-weight corners are ignored: whatever colour they hold
    holes = rng.random(n) < 0.5
    cw2 = cw.copy()
    cw2[holes] = (9.0, 9.0, 9.0, 0.0)
    c2 = tr.vertex_colors(cw2, res, LO, HI, vtx)
    lit = c2.any(axis=1)
    assert lit.sum() > 100 and np.abs(c2[lit] - np.float32([0.25, 0.5, 0.75])).max() <= BLEND_EPS
    assert (c2[~lit] == 0).all()
    # no colour anywhere: black
    cw3 = cw.copy()
    cw3[:, 3] = 0
    assert (tr.vertex_colors(cw3, res, LO, HI, vtx) == 0).all()
    # the blend itself: one coloured corner pair along z
    cw4 = np.zeros((n, 4), dtype=np.float32)
    cw4[0], cw4[1] = (1.0, 0.0, 0.0, 1.0), (0.0, 1.0, 0.0, 1.0)             # points (0, 0, 0) and (0, 0, 1)
    p = np.float32([[-1.0, -1.0, -1.0 + 0.25 * 0.5]])                        # a quarter of the way along the first z edge
    assert np.allclose(tr.vertex_colors(cw4, res, LO, HI, p), [[0.75, 0.25, 0.0]], atol=1e-6)


def test_the_tool_checks_its_arguments_before_loading_anything(tmp_path):
    import importlib.util
    path = os.path.join(ROOT, "tools", "export_tsdf_mesh.py")
    spec = importlib.util.spec_from_file_location("export_tsdf_mesh_tool", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    missing = str(tmp_path / "no_such_checkpoint")
    with pytest.raises(SystemExit, match="--bounds"):
        tool.main([missing, str(tmp_path), str(tmp_path / "out.ply"), "--bounds", "0,0,0,1,1"])
    with pytest.raises(SystemExit, match="--resolution"):
        tool.main([missing, str(tmp_path), str(tmp_path / "out.ply"), "--resolution", "64,64"])
    with pytest.raises(SystemExit):
        tool.main([missing, str(tmp_path), str(tmp_path / "out.ply"), "--colors", "vertex"])
    assert not (tmp_path / "out.ply").exists()
