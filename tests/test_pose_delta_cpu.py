"""Host side of the device pose deltas (lsenerf_amd.pose_delta_dev, BatchComposer.attach_camera_optimizers): the C-ABI surface, the
refusals made before any launch, and the float64 restatement of tests/pose_delta_fixtures.py against cameras.py itself."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from tests import pose_delta_fixtures as F
from tests.spline_fixtures import make_spline
from tests.test_compose_cpu import COL_TIMES, N_COL, N_FRAMES, make_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lse_pose_delta_tables", "lse_pose_delta_tables_bwd")


# ---------------------------------------------------------------------------------------------------- 1. C-ABI surface
def _exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r" T (lse_\w+)", nm))


def test_header_libraries_and_binding_carry_the_pose_delta_entry_points():
    from lsenerf_amd import _lib
    with open(os.path.join(ROOT, "include", "lse_hip.h")) as fh:
        header = fh.read()
    shipped, dev = _exported(_lib.LIB_PATH), _exported(_lib.DEV_LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in shipped and name in dev, name
        assert name in _lib.SIGNATURES, name
    assert "typedef struct lse_pose_delta_desc" in header
    assert "ns_camera_optimizer.py:214-414" in header and "camera_tables" in header          # the call sites they replace
    assert _lib.load().lse_abi_version() == 6 == _lib.LSE_ABI_VERSION
    assert int(re.search(r"#define LSE_ABI_VERSION (\d+)", header).group(1)) == 6
    assert (_lib.LSE_POSE_SO3XR3, _lib.LSE_POSE_SE3) == tuple(int(re.search(r"#define %s (\d+)" % n, header).group(1))
                                                              for n in ("LSE_POSE_SO3XR3", "LSE_POSE_SE3"))


def test_pose_delta_descriptor_has_the_layout_the_header_declares():
    """The ctypes mirror against the C compiler's view of include/lse_hip.h (size and probe fields)."""
    import shutil
    import tempfile
    from lsenerf_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "the build needs a C compiler anyway (oracle/c)"
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "lse_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n",' \
          "sizeof(lse_pose_delta_desc), offsetof(lse_pose_delta_desc, mode), offsetof(lse_pose_delta_desc, shared_prev_next)," \
          "offsetof(lse_pose_delta_desc, base), offsetof(lse_pose_delta_desc, adj), offsetof(lse_pose_delta_desc, frozen));return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "p.c"), "w") as fh:
            fh.write(src)
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")], check=True)
        got = [int(v) for v in subprocess.run([os.path.join(d, "p")], capture_output=True, text=True, check=True).stdout.split()]
    S = _lib.PoseDeltaDesc
    assert got == [ctypes.sizeof(S), S.mode.offset, S.shared_prev_next.offset, S.base.offset, S.adj.offset, S.frozen.offset]


def test_inconsistent_descriptors_are_refused_through_lse_last_error():
    """Every refusal happens on the host, before anything is launched (so this runs without a device)."""
    from lsenerf_amd import _lib
    buf = ctypes.create_string_buffer(64)             # stands in for device memory: a refused call never reads it
    p = ctypes.addressof(buf)
    i3 = lambda *v: (ctypes.c_int32 * 3)(*v)
    p3 = lambda *v: (ctypes.c_void_p * 3)(*v)

    def desc(**kw):
        d = dict(n_cam=i3(2, 1, 0), mode=i3(0, 1, 0), shared_prev_next=0, base=p3(p, p, None), adj=p3(p, p, None), frozen=p3(None, None, None))
        d.update(kw)
        return _lib.PoseDeltaDesc(**d)

    P = ctypes.c_void_p(p)

    def fwd(d, tables=(P, P, None)):
        _lib.call("lse_pose_delta_tables", ctypes.byref(d), *tables, None)

    def bwd(d, grads=(P, P, None), out=(P, P, None)):
        _lib.call("lse_pose_delta_tables_bwd", ctypes.byref(d), *grads, *out, None)
    for call in (fwd, bwd):
        with pytest.raises(_lib.LseHipError, match=r"n_cam\[1\] < 0"):
            call(desc(n_cam=i3(2, -1, 0)))
        with pytest.raises(_lib.LseHipError, match="unknown mode 2 of segment 0"):
            call(desc(mode=i3(2, 1, 0)))
        with pytest.raises(_lib.LseHipError, match="0 rows"):
            call(desc(n_cam=i3(0, 0, 0)))
        with pytest.raises(_lib.LseHipError, match="null base poses or parameters of segment 1"):
            call(desc(adj=p3(p, None, None)))
        with pytest.raises(_lib.LseHipError, match="shared parameter block"):
            call(desc(shared_prev_next=1))
        with pytest.raises(_lib.LseHipError, match="shared_prev_next must be 0 or 1"):
            call(desc(shared_prev_next=2))
    with pytest.raises(_lib.LseHipError, match="null pose table of segment 1"):
        fwd(desc(), (P, None, None))
    with pytest.raises(_lib.LseHipError, match="null table gradient of segment 0"):
        bwd(desc(), (None, P, None))
    with pytest.raises(_lib.LseHipError, match="null output of segment 1"):
        bwd(desc(), out=(P, None, None))


# ---------------------------------------------------------------------------------------------------- 2. the restatement
@pytest.mark.parametrize("mode,C", F.FIXTURES)
def test_restatement_equals_cameras_py_in_float64(mode, C):
    p, base, masked = F.make_params(C), F.make_base(C), F.masked_cameras(C)
    F.check_fixture(p)
    seen = {m for m in F.MAGS[:min(C, 8)]}
    assert C == 1 or seen == set(F.MAGS)
    d = F.random_table_grad(C)
    want, want_g = F.cameras_py(p, base, mode, masked, d, torch.float64)
    got = F.tables_f64(p, base, mode, masked)
    got_g = F.autograd_f64(p, base, mode, masked, d)
    assert want.dtype == got.dtype == torch.float64
    assert float((got - want).abs().max()) <= 1e-12 and float((got_g - want_g).abs().max()) <= 1e-12
    assert bool(torch.isfinite(got_g).all())
    if masked is not None:
        assert torch.equal(got[masked], base.double()[masked]) and float(got_g[masked].abs().max()) == 0.0
        assert float(got_g[1].abs().max()) > 0                      # the zero row: trainable, with a gradient


# ---------------------------------------------------------------------------------------------------- 3. attach, refusals
def _composer(tmp_path, deblur=False, prevnext=False):
    """A composer over a scene held in HOST memory: construction and attaching launch nothing."""
    from lsenerf_amd.data import BatchComposer, DeviceScene
    col_ds, evs_ds = make_scene(tmp_path, prevnext=prevnext)
    scene = DeviceScene.from_datasets(col_ds, evs_ds, "cpu", rgb_times=torch.tensor(COL_TIMES))
    return col_ds, evs_ds, BatchComposer(scene, 12, 8, deblur=deblur, event_pairing="prevnext" if prevnext else "consec", num_embd=8)


def _optim(n, mode="SO3xR3", kind="ns", **kw):
    from lsenerf_amd import cameras as cam
    return cam.CameraOptimizerConfig(mode=mode, optim_type=kind, **kw).setup(num_cameras=n, device="cpu")


def test_attach_camera_optimizers_plans_the_tables_of_the_composer(tmp_path):
    from lsenerf_amd import cameras as cam
    # consec: col + the one event table
    col_ds, evs_ds, comp = _composer(tmp_path)
    frozen = torch.tensor([0, 3])
    col = cam.CameraOptimizer(cam.CameraOptimizerConfig(mode="SE3"), N_COL, non_trainable_camera_indices=frozen)
    evs = _optim(N_FRAMES + 1)
    poses = comp.attach_camera_optimizers(col=col, evs=evs)
    assert comp.deltas is poses and poses.fed == [True, True, False] and not poses.shared
    assert list(poses.blocks) == ["col", "prev"] and poses.n_cam == [N_COL, N_FRAMES + 1, 0]
    assert poses.frozen[0].tolist() == [1, 0, 0, 1, 0, 0] and poses.frozen[1] is None
    assert torch.equal(poses.base[0], col_ds.cameras.camera_to_worlds) and poses.base[0] is not col_ds.cameras.camera_to_worlds
    assert [tuple(g.shape) for g in poses.grads.values()] == [(N_COL, 6), (N_FRAMES + 1, 6)]
    assert poses.parameters()[0] is col.pose_adjustment and poses.parameters()[1] is evs.pose_adjustment
    with pytest.raises(ValueError, match="fed by the attached camera optimiser"):
        comp.set_poses(col=comp.pose_tables[0].clone())
    with pytest.raises(ValueError, match="camera optimiser attached"):
        comp.compose(tables=[t for t in comp.pose_tables if t is not None])
    with pytest.raises(ValueError, match="already fed by an attached camera optimiser"):
        comp.attach_spline(make_spline(col_ds.cameras))
    # only evs: the colour table stays the caller's
    _, _, comp2 = _composer(tmp_path)
    comp2.attach_camera_optimizers(evs=_optim(N_FRAMES + 1))
    comp2.set_poses(col=comp2.pose_tables[0].clone())
    with pytest.raises(ValueError, match="fed by the attached camera optimiser"):
        comp2.set_poses(prev=comp2.pose_tables[1].clone())
    # prevnext: two optimisers, or one shared block over two base-pose sets
    _, evs_pn, comp3 = _composer(tmp_path, prevnext=True)
    pn = _optim(N_FRAMES, kind="prevnext")
    poses3 = comp3.attach_camera_optimizers(evs=pn)
    assert poses3.fed == [False, True, True] and not poses3.shared and list(poses3.blocks) == ["prev", "nxt"]
    assert poses3.parameters()[0] is pn.prev_optim.pose_adjustment and poses3.parameters()[1] is pn.next_optim.pose_adjustment
    assert torch.equal(poses3.base[2], evs_pn.out.next_cameras.camera_to_worlds)
    _, _, comp4 = _composer(tmp_path, prevnext=True)
    one = _optim(N_FRAMES)
    poses4 = comp4.attach_camera_optimizers(evs=one)
    assert poses4.shared and list(poses4.blocks) == ["prev"] and poses4.fed == [False, True, True]
    assert not torch.equal(poses4.base[1], poses4.base[2]) and len(poses4.parameters()) == 1


def test_attach_camera_optimizers_refuses_what_it_cannot_feed(tmp_path):
    col_ds, _, comp = _composer(tmp_path)
    with pytest.raises(ValueError, match="col=, evs= or both"):
        comp.attach_camera_optimizers()
    with pytest.raises(ValueError, match=f"has {N_COL + 1} cameras, the colour table {N_COL}"):
        comp.attach_camera_optimizers(col=_optim(N_COL + 1))
    with pytest.raises(ValueError, match="cameras, the table"):
        comp.attach_camera_optimizers(evs=_optim(N_FRAMES))                    # consec: one more camera than frames
    with pytest.raises(ValueError, match="needs event_pairing='prevnext'"):
        comp.attach_camera_optimizers(evs=_optim(N_FRAMES + 1, kind="prevnext"))
    with pytest.raises(ValueError, match="attach_spline"):
        comp.attach_camera_optimizers(col=make_spline(col_ds.cameras))
    # off, and "delayed" before turn_on(): the wording of attach_spline
    with pytest.raises(ValueError, match="mode is 'off'"):
        comp.attach_camera_optimizers(col=_optim(N_COL, mode="off"))
    delayed = _optim(N_FRAMES + 1, scheme="delayed")
    assert delayed.config.mode == "off"
    with pytest.raises(ValueError, match="turn_on"):
        comp.attach_camera_optimizers(evs=delayed)
    assert comp.deltas is None
    comp.set_poses(prev=comp.pose_tables[1].clone())                           # nothing attached: the tables are still the caller's
    with pytest.raises(ValueError, match="no camera optimiser attached"):
        comp.delta_grads((None, None, None))
    with pytest.raises(ValueError, match="no camera optimiser attached"):
        comp.delta_pose_tables()
    delayed.turn_on()
    assert comp.attach_camera_optimizers(evs=delayed) is comp.deltas
    _, _, comp_pn = _composer(tmp_path, prevnext=True)
    half = _optim(N_FRAMES, kind="prevnext", scheme="delayed")
    half.prev_optim.turn_on()
    with pytest.raises(ValueError, match="'nxt' optimiser's mode is 'off'"):
        comp_pn.attach_camera_optimizers(evs=half)
    # deblur rays exist only with the spline
    _, _, comp_d = _composer(tmp_path, deblur=True)
    with pytest.raises(ValueError, match="G == 4"):
        comp_d.attach_camera_optimizers(col=_optim(N_COL))
    # a table a spline feeds already; a spline on "col" beside per-camera optimisers on the event tables is what the reference builds
    comp_d.attach_spline(make_spline(col_ds.cameras), tables=("col", "prev"))
    with pytest.raises(ValueError, match="already fed by the attached spline"):
        comp_d.attach_camera_optimizers(evs=_optim(N_FRAMES + 1))
    _, _, comp_m = _composer(tmp_path, deblur=True)
    comp_m.attach_spline(make_spline(col_ds.cameras), tables=("col",))
    poses = comp_m.attach_camera_optimizers(evs=_optim(N_FRAMES + 1))
    assert comp_m.spline.fed == [True, False, False] and poses.fed == [False, True, False]
    # a mask that names no camera of the set, parameters of the wrong shape
    from lsenerf_amd import cameras as cam
    bad = cam.CameraOptimizer(cam.CameraOptimizerConfig(mode="SO3xR3"), N_COL, non_trainable_camera_indices=torch.tensor([N_COL]))
    with pytest.raises(ValueError, match="non_trainable_camera_indices"):
        comp.attach_camera_optimizers(col=bad)
    wrong = _optim(N_COL)
    wrong.pose_adjustment = torch.nn.Parameter(torch.zeros(N_COL, 6, dtype=torch.float64))
    with pytest.raises(ValueError, match="contiguous float32"):
        comp.attach_camera_optimizers(col=wrong)


def test_parameters_that_moved_since_attach_are_refused_before_a_launch(tmp_path):
    """``FlatParams`` re-points ``.data``: built after attaching it leaves the kernels' pointers behind (also for the spline, whose
    check compares addresses, not Parameter objects)."""
    from lsenerf_amd.optim import FlatParams
    col_ds, _, comp = _composer(tmp_path)
    col = _optim(N_COL)
    poses = comp.attach_camera_optimizers(col=col)
    poses._current_desc()
    FlatParams([col.pose_adjustment])
    with pytest.raises(ValueError, match="have moved since attach_camera_optimizers"):
        poses.forward(comp.pose_tables)
    with pytest.raises(ValueError, match="have moved"):
        comp.delta_grads(comp._pose_grads)
    _, _, comp_s = _composer(tmp_path, deblur=True)
    spl = make_spline(col_ds.cameras)
    sp = comp_s.attach_spline(spl)
    sp._current_desc()
    FlatParams([spl.ctrl_tangents, spl.scale])
    with pytest.raises(ValueError, match="have moved since attach_spline"):
        sp.forward(comp_s.pose_tables)
