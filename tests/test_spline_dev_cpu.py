"""Host side of the device spline poses (lsenerf_amd.spline_dev, BatchComposer.attach_spline): the C-ABI surface, the precomputed
brackets / query lists / deblur times against what cameras.py computes, and the refusals (fixtures: tests/spline_fixtures.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.spline_fixtures import FIXTURES, check_fixture, make_spline
from tests.test_compose_cpu import COL_HW, COL_TIMES, EVS_TIMES, N_COL, _cams, make_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lse_spline_poses", "lse_spline_poses_bwd")


# ---------------------------------------------------------------------------------------------------- 1. C-ABI surface
def _exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r" T (lse_\w+)", nm))


def test_header_libraries_and_binding_carry_the_spline_entry_points():
    from lsenerf_amd import _lib
    with open(os.path.join(ROOT, "include", "lse_hip.h")) as fh:
        header = fh.read()
    shipped, dev = _exported(_lib.LIB_PATH), _exported(_lib.DEV_LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in shipped and name in dev, name
        assert name in _lib.SIGNATURES, name
    assert "typedef struct lse_spline_desc" in header
    assert "ns_camera_optimizer.py:130-197" in header and "cameras.py" in header          # the call sites they replace
    assert _lib.load().lse_abi_version() == 6 == _lib.LSE_ABI_VERSION
    assert int(re.search(r"#define LSE_ABI_VERSION (\d+)", header).group(1)) == 6


def test_spline_descriptor_has_the_layout_the_header_declares():
    """The ctypes mirror against the C compiler's view of include/lse_hip.h (size and probe fields)."""
    import shutil
    import tempfile
    from lsenerf_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "the build needs a C compiler anyway (oracle/c)"
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "lse_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n",' \
          "sizeof(lse_spline_desc), offsetof(lse_spline_desc, evs), offsetof(lse_spline_desc, dM)," \
          "offsetof(lse_spline_desc, ctrl_tangents), offsetof(lse_spline_desc, frac), offsetof(lse_spline_desc, csr_query));return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "p.c"), "w") as fh:
            fh.write(src)
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")], check=True)
        got = [int(v) for v in subprocess.run([os.path.join(d, "p")], capture_output=True, text=True, check=True).stdout.split()]
    S = _lib.SplineDesc
    assert got == [ctypes.sizeof(S), S.evs.offset, S.dM.offset, S.ctrl_tangents.offset, S.frac.offset, S.csr_query.offset]


# ---------------------------------------------------------------------------------------------------- 2. the fixtures
def test_fixtures_meet_their_conditions_and_cover_every_branch():
    from lsenerf_amd.spline_dev import SplinePlan
    seen = set()
    for name, make in FIXTURES.items():
        spl, segments, shapes = make()
        dots = check_fixture(spl)
        plan = SplinePlan(spl.ctrl_ts, segments, spl.exp_t)
        assert plan.n_query == [0 if s is None else int(np.prod(s[:-2])) for s in shapes], name
        used = dots[torch.unique(plan.idx)]                              # the pairs some query interpolates between
        seen |= {"slerp"} if bool((used.abs() < 0.9995).any()) else set()
        seen |= {"lerp"} if bool((used.abs() > 0.9995).any()) else set()
        seen |= {"flip"} if bool((used < 0).any()) else set()
        seen |= {"zero_rotvec"} if bool((spl.ctrl_tangents[:, 3:].abs().amax(1) == 0).any()) else set()
        times = torch.cat([t for t in plan.times if t is not None])
        seen |= {"clip_lo"} if bool((times < spl.ctrl_ts[0]).any()) else set()
        seen |= {"clip_hi"} if bool((times > spl.ctrl_ts[-1]).any()) else set()
        seen |= {"at_last_ctrl"} if bool((times == spl.ctrl_ts[-1]).any()) else set()
        seen |= {"at_inner_ctrl"} if bool(torch.isin(times, spl.ctrl_ts[1:-1]).any()) else set()
        seen.add(f"factor{spl.pnt_factor}")
        seen |= {"evs"} if "evs" in plan.kinds else set()
        seen |= {k for k in plan.kinds if k}
        assert float(spl.scale.detach()) != 1.0 and float((spl.dM - torch.eye(4)).abs().max()) > 0.01
    assert seen >= {"slerp", "lerp", "flip", "zero_rotvec", "clip_lo", "clip_hi", "at_last_ctrl", "at_inner_ctrl", "factor1", "factor3",
                    "evs", "rgb", "deblur"}, seen
    # the two synthetic shapes: a list longer than a wave; more control points than a block has waves, some on no list
    k5 = SplinePlan(FIXTURES["k5_q300"]()[0].ctrl_ts, FIXTURES["k5_q300"]()[1], 0.3)
    assert sum(k5.n_query) == 300 and k5.n_ctrl == 5 and int(torch.diff(k5.csr_start).max()) > 64
    k70 = SplinePlan(FIXTURES["k70_q130"]()[0].ctrl_ts, FIXTURES["k70_q130"]()[1], 0.3)
    empty = torch.diff(k70.csr_start) == 0
    assert sum(k70.n_query) == 130 and k70.n_ctrl == 70 and bool(empty[22:40].all()) and not bool(empty[:22].any())


# ---------------------------------------------------------------------------------------------------- 3. the precomputation
@pytest.mark.parametrize("name", list(FIXTURES))
def test_brackets_are_what_the_interpolation_computes_internally(name, monkeypatch):
    """``idx`` / ``frac`` against the lines of ``vectorized_generalized_interpolation`` restated, and against the call itself: the
    fraction and the two control quaternions it hands to ``slerp`` (which pins the index) are bit-equal."""
    from lsenerf_amd import cameras as cam
    from lsenerf_amd.spline_dev import SplinePlan
    spl, segments, _ = FIXTURES[name]()
    plan = SplinePlan(spl.ctrl_ts, segments, spl.exp_t)
    times = torch.cat([t for t in plan.times if t is not None])
    ts = torch.clip(times, spl.ctrl_ts[0], spl.ctrl_ts[-1]).reshape(-1)
    idx = torch.clamp(torch.searchsorted(spl.ctrl_ts, ts, right=True), 1, len(spl.ctrl_ts) - 1) - 1
    t = (ts - spl.ctrl_ts[idx]) / (spl.ctrl_ts[idx + 1] - spl.ctrl_ts[idx])
    assert plan.idx.dtype == torch.int64 and torch.equal(plan.idx, idx)
    assert plan.frac.dtype == torch.float32 and torch.equal(plan.frac, t)
    assert int(plan.idx.min()) >= 0 and int(plan.idx.max()) <= plan.n_ctrl - 2
    assert float(plan.frac.min()) >= 0.0 and float(plan.frac.max()) <= 1.0
    seen = {}
    real = cam.slerp
    monkeypatch.setattr(cam, "slerp", lambda v0, v1, tt: (seen.update(v0=v0, v1=v1, t=tt), real(v0, v1, tt))[1])
    spl.get_rgb_cameras(times)
    quats = cam.exp_map_to_quat(spl.ctrl_tangents[:, 3:])
    assert torch.equal(seen["t"].reshape(-1), plan.frac)
    assert torch.equal(seen["v0"], quats[plan.idx]) and torch.equal(seen["v1"], quats[plan.idx + 1])


@pytest.mark.parametrize("name", list(FIXTURES))
def test_query_lists_name_exactly_the_bracketed_queries_in_ascending_order(name):
    from lsenerf_amd.spline_dev import SplinePlan
    spl, segments, _ = FIXTURES[name]()
    plan = SplinePlan(spl.ctrl_ts, segments, spl.exp_t)
    start, query = plan.csr_start.tolist(), plan.csr_query.tolist()
    assert plan.csr_start.dtype == plan.csr_query.dtype == torch.int32
    assert len(start) == plan.n_ctrl + 1 and start[0] == 0 and start[-1] == len(query) == 2 * sum(plan.n_query)
    idx = plan.idx.tolist()
    for k in range(plan.n_ctrl):
        assert query[start[k]:start[k + 1]] == [q for q, i in enumerate(idx) if i == k or i + 1 == k], k


def test_deblur_times_are_bit_equal_to_get_deblur_cameras(monkeypatch):
    from lsenerf_amd.spline_dev import SplinePlan, deblur_times
    for factor, exp_t in ((1, 0.3), (3, 0.07)):
        spl = make_spline(_cams(N_COL, COL_HW, 2, COL_TIMES, 31.0), factor=factor, exp_t=exp_t)
        cam_ts = torch.tensor(COL_TIMES).reshape(-1, 1)
        seen = {}
        real = spl.get_rgb_cameras
        monkeypatch.setattr(spl, "get_rgb_cameras", lambda times: (seen.update(times=times), real(times))[1])
        spl.get_deblur_cameras(cam_ts)
        plan = SplinePlan(spl.ctrl_ts, [("deblur", cam_ts), None, None], spl.exp_t, spl.n_deblur_rays)
        assert seen["times"].shape == (4 * N_COL,) and torch.equal(plan.times[0], seen["times"])
        assert torch.equal(deblur_times(cam_ts, exp_t), seen["times"])


# ---------------------------------------------------------------------------------------------------- 4. attach_spline, refusals
def _cpu_composer(tmp_path, deblur=True, prevnext=False):
    """A composer over a scene held in HOST memory: construction and ``attach_spline`` launch nothing."""
    from lsenerf_amd.data import BatchComposer, DeviceScene
    col_ds, evs_ds = make_scene(tmp_path, prevnext=prevnext)
    scene = DeviceScene.from_datasets(col_ds, evs_ds, "cpu", rgb_times=torch.tensor(COL_TIMES))
    return col_ds, BatchComposer(scene, 12, 8, deblur=deblur, event_pairing="prevnext" if prevnext else "consec", num_embd=8)


@pytest.mark.parametrize("deblur,prevnext", [(True, False), (False, True)])
def test_attach_spline_plans_the_tables_of_the_composer(tmp_path, deblur, prevnext):
    from lsenerf_amd.spline_dev import SplinePlan
    col_ds, comp = _cpu_composer(tmp_path, deblur, prevnext)
    spl = make_spline(col_ds.cameras, factor=3)
    poses = comp.attach_spline(spl)
    assert comp.spline is poses
    evs = torch.tensor(EVS_TIMES)
    want = [("deblur" if deblur else "rgb", torch.tensor(COL_TIMES)), ("evs", evs[:9] if prevnext else evs), ("evs", evs[1:10]) if prevnext else None]
    ref = SplinePlan(spl.ctrl_ts, want, spl.exp_t)
    assert poses.plan.kinds == ref.kinds and poses.plan.n_query == ref.n_query
    assert torch.equal(poses.plan.idx, ref.idx) and torch.equal(poses.plan.frac, ref.frac)
    assert torch.equal(poses.plan.csr_query, ref.csr_query)
    assert poses.grads["ctrl_tangents"].shape == spl.ctrl_tangents.shape and poses.grads["scale"].shape == (1,)
    # fed tables refuse poses from elsewhere (before anything is copied or launched)
    with pytest.raises(ValueError, match="fed by the attached spline"):
        comp.set_poses(col=comp.pose_tables[0].clone())
    with pytest.raises(ValueError, match="spline attached"):
        comp.compose(tables=[t for t in comp.pose_tables if t is not None])
    # a subset: the other tables stay the caller's
    _, comp2 = _cpu_composer(tmp_path, deblur, prevnext)
    comp2.attach_spline(spl, tables=("col",))
    assert comp2.spline.fed == [True, False, False]
    comp2.set_poses(prev=comp2.pose_tables[1].clone())
    with pytest.raises(ValueError, match="no 'nxt' pose table" if not prevnext else "fed by"):
        comp2.attach_spline(spl, tables=("nxt",)) if not prevnext else comp2.set_poses(col=comp2.pose_tables[0].clone())


def test_a_spline_that_is_off_is_refused(tmp_path):
    col_ds, comp = _cpu_composer(tmp_path)
    frozen = make_spline(col_ds.cameras, mode="off")
    with pytest.raises(ValueError, match="mode is 'off'"):
        comp.attach_spline(frozen)
    delayed = make_spline(col_ds.cameras, scheme="delayed")
    assert delayed.config.mode == "off"
    with pytest.raises(ValueError, match="turn_on"):
        comp.attach_spline(delayed)
    assert comp.spline is None
    comp.set_poses(col=comp.pose_tables[0].clone())              # nothing attached: the tables are still the caller's
    delayed.turn_on()
    assert comp.attach_spline(delayed) is comp.spline
    with pytest.raises(ValueError, match="no spline attached"):
        _cpu_composer(tmp_path)[1].spline_grads((None, None, None))


# ---------------------------------------------------------------------------------------------------- 5. descriptor checks
def test_inconsistent_descriptors_are_refused_through_lse_last_error():
    """Every refusal happens on the host, before anything is launched (so this runs without a device)."""
    from lsenerf_amd import _lib
    buf = ctypes.create_string_buffer(64)             # stands in for device memory: a refused call never reads it
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def desc(**kw):
        d = dict(n_ctrl=4, n_query=(ctypes.c_int32 * 3)(2, 1, 0), evs=(ctypes.c_int32 * 3)(0, 1, 0), csr_len=6, ctrl_tangents=p, scale=p,
                 idx=p, frac=p, csr_start=p, csr_query=p)
        d.update(kw)
        return _lib.SplineDesc(**d)

    def fwd(d, tables=(p, p, None)):
        _lib.call("lse_spline_poses", ctypes.byref(d), *tables, None)

    def bwd(d, grads=(p, p, None), out=(p, p)):
        _lib.call("lse_spline_poses_bwd", ctypes.byref(d), *grads, *out, None)
    for call in (fwd, bwd):
        with pytest.raises(_lib.LseHipError, match="at least two control points"):
            call(desc(n_ctrl=1))
        with pytest.raises(_lib.LseHipError, match=r"n_query\[1\] < 0"):
            call(desc(n_query=(ctypes.c_int32 * 3)(2, -1, 0)))
        with pytest.raises(_lib.LseHipError, match=r"evs\[0\] must be 0 or 1"):
            call(desc(evs=(ctypes.c_int32 * 3)(2, 1, 0)))
        with pytest.raises(_lib.LseHipError, match="0 queries"):
            call(desc(n_query=(ctypes.c_int32 * 3)(0, 0, 0)))
        with pytest.raises(_lib.LseHipError, match="null parameter or bracket table"):
            call(desc(scale=None))
    with pytest.raises(_lib.LseHipError, match="null pose table of segment 1"):
        fwd(desc(), (p, None, None))
    with pytest.raises(_lib.LseHipError, match="null table gradient of segment 0"):
        bwd(desc(), (None, p, None))
    with pytest.raises(_lib.LseHipError, match="null output"):
        bwd(desc(), out=(p, None))
    with pytest.raises(_lib.LseHipError, match="null query lists"):
        bwd(desc(csr_query=None))
    with pytest.raises(_lib.LseHipError, match="csr_len 5"):
        bwd(desc(csr_len=5))
