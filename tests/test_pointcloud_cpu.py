"""Point-cloud export without a GPU: the numpy twin (tests/pointcloud_ref.py) on its analytic scene -- a sphere seen by six cameras
plus planted floaters -- and the package's host side: the PLY writer, the argument checks of ``export_point_cloud`` and the ops'
refusal of CPU tensors."""
import types

import numpy as np
import pytest
import torch

from tests import pointcloud_ref as pr


def test_the_scene_gives_the_probed_figures():
    s = pr.scene_cloud()
    assert s["total"] == 6775 + pr.N_PLANTED and s["n_sphere"] == 6775
    assert s["res"] == (40, 40, 40)
    assert len(s["keys"]) == 2142 and int(s["planted_only"].sum()) == pr.N_PLANTED
    assert int(s["support"][~s["planted_only"]].min()) >= 24
    assert s["support"][s["planted_only"]].tolist() == [1] * pr.N_PLANTED
    assert int(s["counts"].max()) == 9


def test_unprojected_points_lie_on_the_sphere():
    s = pr.scene_cloud()
    p = s["points"][:s["n_sphere"]].astype(np.float64)
    dist = np.abs(np.linalg.norm(p - np.asarray(pr.CENTRE), axis=1) - pr.RADIUS)
    assert dist.max() <= 1e-6, dist.max()         # measured: 1.501e-7
    planted = s["points"][s["n_sphere"]:].astype(np.float64)
    assert np.abs(planted - pr.planted_points()).max() <= 1e-6
    assert (np.abs(np.linalg.norm(planted - np.asarray(pr.CENTRE), axis=1) - pr.RADIUS) >= 0.25 - 1e-6).all()


def test_merged_voxels_are_ordered_counted_and_inside_their_voxel():
    s = pr.scene_cloud()
    keys, counts, merged, res = s["keys"], s["counts"], s["merged"], s["res"]
    assert (np.diff(keys) > 0).all()
    assert int(counts.sum()) == s["total"] and (counts >= 1).all()
    x, y, z = pr.coords(keys, res)
    ulp = float(np.spacing(np.float32(1.0)))       # 1 ulp of the box scale: |coordinates| <= 1
    for k, v in enumerate((x, y, z)):
        lo = pr.BOX[0][k] + v * pr.VOXEL
        assert (merged[:, k] >= lo - ulp).all() and (merged[:, k] <= lo + pr.VOXEL + ulp).all(), k


def test_support_filter_separates_floaters_from_the_surface():
    s = pr.scene_cloud()
    keep, sup = pr.support_filter(s["keys"], s["counts"], s["res"], 4)
    assert np.array_equal(sup, s["support"])
    assert np.array_equal(keep, ~s["planted_only"])               # exactly the planted-only voxels go, none of the sphere's
    assert int(keep.sum()) == 2142 - pr.N_PLANTED
    keep0, _ = pr.support_filter(s["keys"], s["counts"], s["res"], 0)
    assert keep0.all()


def test_twin_edges():
    # the validity rule: NaN fails every comparison, the box faces are inside
    o = np.zeros((7, 3), np.float32)
    d = np.tile(np.array([1.0, 0.0, 0.0], np.float32), (7, 1))
    depth = np.array([1.0, np.nan, np.inf, 0.0, -1.0, np.nextafter(np.float32(1), np.float32(2)), 0.5], np.float32)
    acc = np.array([1, 1, 1, 1, 1, 1, np.nan], np.float32)
    p, keep = pr.unproject(o, d, depth, acc, (-1, -1, -1), (1, 1, 1), 0.5)
    assert keep.tolist() == [True, False, False, False, False, False, False]
    # keys: clamped into the lattice, NaN -> 0, INT64_MAX behind the count
    pts = np.array([[-1, -1, -1], [1, 1, 1], [5, -5, np.nan], [0.0, 0.0, 0.0]], np.float32)
    k = pr.voxel_keys(pts, (-1, -1, -1), 0.5, (4, 4, 4), count=3)
    assert k.tolist() == [0, 63, 3 * 16, pr.NO_KEY]
    # adjacent keys that are not neighbours
    keys = np.array([(1 * 5 + 2) * 4 + 3, (1 * 5 + 3) * 4 + 0], np.int64)
    assert keys[1] - keys[0] == 1
    assert pr.support(keys, np.array([2, 3]), (3, 5, 4)).tolist() == [2, 3]
    # a zero normal sum stays zero; the mean is sequential
    sk = np.zeros(2, np.int64)
    _, c, mp, _, mn = pr.voxel_merge(sk, np.array([0, 1]), np.ones((2, 3), np.float32), None,
                                     np.array([[0, 0, 1], [0, 0, -1]], np.float32))
    assert c.tolist() == [2] and mp.tolist() == [[1, 1, 1]] and mn.tolist() == [[0, 0, 0]]
    assert pr.ulp_distance(np.float32([1.0, -0.0]), np.float32([np.nextafter(np.float32(1), np.float32(2)), 0.0])) == 1


# ---- the package's host side ----------------------------------------------------------------------------------------------------
def _cloud(n, colors, normals, seed=3):
    from lsenerf_amd.pointcloud import PointCloud
    g = torch.Generator().manual_seed(seed)
    unit = lambda t: t / t.norm(dim=-1, keepdim=True)
    return PointCloud(torch.randn(n, 3, generator=g), torch.rand(n, 3, generator=g) if colors else None,
                      unit(torch.randn(n, 3, generator=g)) if normals else None, torch.ones(n, dtype=torch.int32))


@pytest.mark.parametrize("colors", [False, True])
@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("n", [0, 37])
def test_ply_round_trip(tmp_path, n, colors, normals):
    from lsenerf_amd.pointcloud import write_ply_points
    cloud = _cloud(n, colors, normals)
    path = str(tmp_path / "cloud.ply")
    write_ply_points(path, cloud)
    rec, names = pr.read_ply_points(path)
    assert names == ["x", "y", "z"] + (["nx", "ny", "nz"] if normals else []) + (["red", "green", "blue"] if colors else [])
    assert rec.shape == (n,)
    assert np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], 1), cloud.points.numpy())
    if normals:
        assert np.array_equal(np.stack([rec["nx"], rec["ny"], rec["nz"]], 1), cloud.normals.numpy())
    if colors:
        want = np.rint(np.clip(cloud.colors.numpy(), 0, 1) * 255).astype(np.uint8)
        assert np.array_equal(np.stack([rec["red"], rec["green"], rec["blue"]], 1), want)


def test_invalid_arguments_raise_before_anything_runs():
    from lsenerf_amd.pointcloud import export_point_cloud

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"model.{name} was touched")
    model = types.SimpleNamespace(field=types.SimpleNamespace(aabb=torch.tensor([[-1.0, -1, -1], [1, 1, 1]])))
    model.config = model.scene_aabb = model.occupancy_grid = Untouchable()       # (reading an attribute of these fails the test)
    with pytest.raises(ValueError, match="empty box"):
        export_point_cloud(model, [], bounds=((0.0, 0.0, 0.0), (1.0, 0.0, 1.0)))
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_size"):
            export_point_cloud(model, [], voxel_size=bad)
    with pytest.raises(ValueError, match="min_support needs voxel_size"):
        export_point_cloud(model, [], min_support=3)
    with pytest.raises(ValueError, match="2\\^20"):
        export_point_cloud(model, [], voxel_size=1e-6)                      # 2e6 voxels on an axis
    with pytest.raises(ValueError, match="2\\^20"):
        export_point_cloud(model, [], voxel_size=2.0 / (2 ** 20 + 1))
    with pytest.raises(ValueError, match="image_indices"):
        export_point_cloud(model, [], image_indices=[0])


def test_voxel_lattice_is_the_documented_rule():
    from lsenerf_amd import ops
    assert ops.voxel_lattice((-1, -1, -1), (1, 1, 1), 0.05) == (40, 40, 40) == pr.lattice((-1, -1, -1), (1, 1, 1), 0.05)
    assert ops.voxel_lattice((0, 0, 0), (0.7, 0.01, 30.0), 0.1) == (7, 1, 300)
    assert ops.voxel_lattice((0, 0, 0), (1, 1, 1), 2.0 ** -20) == (2 ** 20,) * 3


def test_ops_refuse_cpu_tensors(monkeypatch):
    from lsenerf_amd import _lib, ops

    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "call", no_library)
    f3 = torch.zeros(4, 3)
    f1 = torch.zeros(4)
    i64, i32 = torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int32)
    total = torch.zeros(1, dtype=torch.int64)
    box = ((-1.0,) * 3, (1.0,) * 3)
    with pytest.raises(_lib.LseHipError, match="must live on the GPU"):
        ops.unproject_append(f3, f3, f1, f1, box[0], box[1], 0.5, f3.clone(), total)
    with pytest.raises(_lib.LseHipError, match="must live on the GPU"):
        ops.voxel_keys(f3, box[0], 0.5, (4, 4, 4))
    with pytest.raises(_lib.LseHipError, match="must live on the GPU"):
        ops.voxel_merge(i64, i64, f3)
    with pytest.raises(_lib.LseHipError, match="must live on the GPU"):
        ops.voxel_support_filter(i64, i32, f3, (4, 4, 4), 1)


def test_the_library_refuses_bad_arguments_before_any_launch():
    """The host-side checks of csrc/pointcloud.hip return LSE_E_INVALID without touching a device: callable without a GPU."""
    import ctypes
    from lsenerf_amd import _lib
    v = ctypes.c_int64(-1)
    for fn in ("lse_unproject_workspace", "lse_voxel_merge_workspace", "lse_voxel_support_workspace"):
        _lib.call(fn, 0, ctypes.byref(v))
        assert v.value == 0
        _lib.call(fn, 1, ctypes.byref(v))
        assert v.value == 8 + 4
        _lib.call(fn, 1025, ctypes.byref(v))
        assert v.value == 2 * 8 + 4 * 1025
        with pytest.raises(_lib.LseHipError, match="extent"):
            _lib.call(fn, -1, ctypes.byref(v))
        with pytest.raises(_lib.LseHipError, match="extent"):
            _lib.call(fn, (1 << 40) + 1, ctypes.byref(v))
    lo = (ctypes.c_float * 3)(-1, -1, -1)
    fake = ctypes.c_void_p(4096)                 # never dereferenced: every call below is refused before a launch
    for res in ((0, 4, 4), (4, (1 << 20) + 1, 4), (4, 4, -1)):
        with pytest.raises(_lib.LseHipError, match=r"every count in \[1, 2\^20\]"):
            _lib.call("lse_voxel_keys", fake, 8, None, lo, 0.5, *res, fake, None)
        with pytest.raises(_lib.LseHipError, match=r"every count in \[1, 2\^20\]"):
            _lib.call("lse_voxel_support_filter", fake, fake, fake, None, None, 8, None, *res, 1, fake, 1 << 20, 8, fake, fake, fake,
                      None, None, None, fake, None)
    for voxel in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.LseHipError, match="voxel size"):
            _lib.call("lse_voxel_keys", fake, 8, None, lo, voxel, 4, 4, 4, fake, None)
    with pytest.raises(_lib.LseHipError, match="workspace of 8 bytes"):
        _lib.call("lse_voxel_merge", fake, fake, fake, None, None, 8, fake, 8, 8, fake, fake, fake, None, None, fake, None)
    with pytest.raises(_lib.LseHipError, match="total must be"):
        _lib.call("lse_unproject_append", fake, fake, fake, fake, None, None, 8, lo, lo, 0.5, fake, 1 << 20, 8, fake, None, None, None,
                  None)
    with pytest.raises(_lib.LseHipError, match="an output without its input"):
        _lib.call("lse_unproject_append", fake, fake, fake, fake, None, None, 8, lo, lo, 0.5, fake, 1 << 20, 8, fake, fake, None, fake,
                  None)
    with pytest.raises(_lib.LseHipError, match="negative capacity"):
        _lib.call("lse_voxel_merge", fake, fake, fake, None, None, 8, fake, 1 << 20, -1, fake, fake, fake, None, None, fake, None)


def test_the_tool_checks_its_arguments_before_loading_anything(tmp_path):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "export_pointcloud.py")
    spec = importlib.util.spec_from_file_location("export_pointcloud_tool", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    missing = str(tmp_path / "no_such_checkpoint")
    with pytest.raises(SystemExit, match="--min-support needs --voxel-size"):
        tool.main([missing, str(tmp_path), str(tmp_path / "out.ply"), "--min-support", "3"])
    with pytest.raises(SystemExit, match="--bounds"):
        tool.main([missing, str(tmp_path), str(tmp_path / "out.ply"), "--bounds", "0,0,0,1,1"])
    assert not (tmp_path / "out.ply").exists()
