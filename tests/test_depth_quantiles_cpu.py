"""Quantile depths without a device: the numpy twins (tests/depth_quantiles_ref.py) on hand-made rays and against each other at
trained-scene densities, the host-side settings and refusals, and header / binding / library agreement."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import depth_quantiles_ref as dr
from tests.util import SURFACE_SIGMAS, trained_scene_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QS = (0.25, 0.5, 0.75)
TAUS = dr.taus_of(QS)
F = np.float32


def _ray(sigmas, t0=1.0, dt=0.1):
    """One ray of contiguous samples of length dt (float32 edges) with the given densities; several: packed in order."""
    rays = sigmas if isinstance(sigmas[0], (list, tuple)) else [sigmas]
    ts, te, sg, cnt = [], [], [], []
    for s in rays:
        e = (t0 + dt * np.arange(len(s) + 1)).astype(F)
        ts.append(e[:-1]); te.append(e[1:]); sg.append(np.asarray(s, F)); cnt.append(len(s))
    cnt = np.asarray(cnt, np.int64)
    packed = np.stack([np.cumsum(cnt) - cnt, cnt], -1)
    return np.concatenate(ts), np.concatenate(te), np.concatenate(sg), packed


def two_surface_ray():
    """Ten samples: a front surface of alpha = 0.6 in sample 2, an opaque one in sample 7, nothing else."""
    s = [0.0] * 10
    s[2] = float(-math.log(0.4) / np.float64(F(1.3) - F(1.2)))
    s[7] = 1e4
    return _ray(s)


def _both(args, interpolate=False):
    return dr.reference(*args, TAUS, interpolate=interpolate), dr.emulate_f32(*args, TAUS, interpolate=interpolate)


def test_two_surfaces_the_median_sits_on_the_front_one_and_the_mean_between_them():
    args = two_surface_ray()
    ts, te, sg, _ = args
    mid = (ts + te) * F(0.5)
    for out in _both(args):
        assert out["index"].tolist() == [[2, 2, 7]] and out["reached"].tolist() == [7]
        assert out["depth"][0, 1] == mid[2] and out["depth"][0, 2] == mid[7]
    sd = sg.astype(np.float64) * (te - ts).astype(np.float64)
    w = np.exp(-(np.cumsum(sd) - sd)) * (1 - np.exp(-sd))
    expected = float((w * mid).sum() / (w.sum() + 1e-10))
    assert abs(w[2] - 0.6) < 1e-6 and abs(w[7] - 0.4) < 1e-6
    assert te[2] < expected < ts[7]                        # in the empty space between the two surfaces
    ref, em = _both(args, interpolate=True)
    for out in (ref, em):
        assert ts[2] <= out["depth"][0, 0] < out["depth"][0, 1] <= te[2] and ts[7] <= out["depth"][0, 2] <= te[7]
    # alpha reaches 0.5 after ln 2 / sigma of the front sample (tau_q is ln 2 rounded to float32: 3e-8 of it, over sigma = 9.2)
    assert abs(ref["depth"][0, 1] - (ts[2] + math.log(2.0) / sg[2])) < 1e-7 and abs(em["depth"][0, 1] - ref["depth"][0, 1]) < 1e-6


def test_never_reached_empty_infinite_and_nan():
    thin = [0.1] * 70                                        # tau = 0.7 at the end: 0.25 and 0.5 are crossed, 0.75 is not
    args = _ray([thin, [], [0.0, 0.0, float("inf"), 0.0], [0.0, 5.0, float("nan"), 50.0, 0.0], [1e-3] * 5])
    ts, te, _, packed = args
    mid = (ts + te) * F(0.5)
    last = lambda r: mid[packed[r, 0] + packed[r, 1] - 1]
    for interp in (False, True):
        ref, em = _both(args, interp)
        for out in (ref, em):
            assert out["reached"].tolist() == [3, 0, 7, 1, 0]
            assert out["index"][0].tolist()[2] == 69 and out["depth"][0, 2] == last(0)        # the clamp to the last sample
            assert out["index"][1].tolist() == [-1] * 3 and np.all(out["depth"][1] == 0.0)      # an empty ray
            assert out["index"][2].tolist() == [2] * 3
            # sigma = inf: the crossing is the sample's near edge; mid-point otherwise
            assert np.all(out["depth"][2] == (ts[packed[2, 0] + 2] if interp else mid[packed[2, 0] + 2]))
            # a NaN density is never crossed, nor anything behind it: 0.25 is found in front of it (tau = 0.5), the rest clamp
            assert out["index"][3].tolist() == [1, 4, 4] and np.all(out["depth"][3, 1:] == last(3))
            assert out["index"][4].tolist() == [4] * 3 and np.all(out["depth"][4] == last(4))
        assert np.array_equal(ref["index"], em["index"])
    # the carry crosses the 64-lane group: found masks and indices of ray 0 come from two groups
    assert dr.emulate_f32(*args, TAUS)["index"][0].tolist()[:2] == dr.reference(*args, TAUS)["index"][0].tolist()[:2]
    assert dr.reference(*args, TAUS)["index"][0, 1] >= 64


def test_depth_select():
    dq = np.asarray([[1.0, 2.0, 3.0], [1.0, 2.0, 9.0], [1.0, 2.0, 3.0], [1.0, 2.0, 3.0]], F)
    reached = np.asarray([7, 7, 3, 5], np.uint8)
    sel = dr.depth_select(dq, reached, 1)
    assert np.array_equal(np.isnan(sel), [False, False, False, True]) and sel[:3].tolist() == [2.0, 2.0, 2.0]
    sel = dr.depth_select(dq, reached, 1, max_spread=2.0)
    assert np.array_equal(np.isnan(sel), [False, True, True, True]) and sel[0] == 2.0
    assert np.array_equal(dr.depth_select(dq, reached, 1, max_spread=float("inf")), dr.depth_select(dq, reached, 1), equal_nan=True)


CASES = [(sg, step, onset) for sg in SURFACE_SIGMAS for step in ("const", "cone") for onset in ("abrupt", "ramp")]


@pytest.mark.parametrize("sg,step,onset", CASES, ids=[f"{sg:g}-{st}-{on}" for sg, st, on in CASES])
def test_emulation_against_reference_at_trained_scene_densities(sg, step, onset):
    never = 0
    for seed in range(3):
        inp = trained_scene_rays(sg, seed=seed, step=step, onset=onset)
        args = tuple(inp[k].numpy() for k in ("ts", "te", "sigma", "packed_info"))
        ref, em = _both(args)
        decided = ~ref["undecided"]
        share = 1.0 - decided.mean()
        print(f"DEPTHQ_EMU sigma {sg:g} {step} {onset} seed {seed}: undecided {int((~decided).sum())} of {decided.size}")
        assert share <= 0.02
        assert np.array_equal(em["index"][decided], ref["index"][decided])
        assert np.array_equal(em["reached"][decided], ref["reached"][decided])
        assert np.array_equal(em["depth"][decided].astype(np.float64), ref["depth"][decided])      # the same float32 mid-points
        assert np.all(np.diff(em["depth"], axis=1) >= 0)
        never += int(sum((((ref["reached"] >> j) & 1) == 0).sum() for j in range(3)))
        # interpolated: inside the crossing sample, and within the bound the scan's tolerance gives
        ref, em = _both(args, interpolate=True)
        assert np.array_equal(em["index"][decided], ref["index"][decided])
        hit = (((ref["reached"][:, None] >> np.arange(3)[None, :]) & 1) == 1) & decided[:, None]
        t = em["depth"].astype(np.float64)
        assert np.all((t >= ref["a"])[hit]) and np.all((t <= ref["b"])[hit])
        ratio = (np.abs(t - ref["depth"]) / dr.interp_bound(ref, TAUS))[decided]
        print(f"DEPTHQ_EMU   interpolated: worst |t - t_ref| / bound = {float(ratio.max()):.3f}")
        assert float(ratio.max()) <= 1.0
        # ascending over the quantiles that were reached (an unreached one is the last sample's MID-point by definition, which may
        # lie in front of a crossing interpolated into that sample's far half)
        assert np.all((t[:, 1:] >= t[:, :-1])[hit[:, 1:]])         # (bit j set implies bit j - 1 set: tau_q ascends)
    assert never > 0                                         # the clamp path is covered in every case


def test_depth_tau():
    from lsenerf_amd import ops
    assert ops.depth_tau(0.5) == float(F(math.log(2.0)))
    for q, t in zip(QS, TAUS):
        assert ops.depth_tau(q) == float(t) == float(F(-math.log(1.0 - q)))
    assert ops.depth_tau(1 - 1e-4) == ops.eval_tau_stop(1e-4)            # the same threshold, seen from the other side
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="depth_tau"):
            ops.depth_tau(bad)


def test_config_fields_and_their_validation():
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig
    from lsenerf_amd.evaluation import depth_quantile_settings
    cfg = LSENeRFModelConfig()
    assert cfg.eval_depth_quantiles == () and cfg.eval_depth_interpolate is False
    assert depth_quantile_settings(cfg) == ((), False)
    box = torch.tensor([[-1.0, -1, -1], [1, 1, 1]])
    small = dict(grid_levels=1, grid_resolution=16, log2_hashmap_size=12)
    for bad in ((0.0, 0.5), (0.5, 1.0), (0.5, 0.25), (0.5, 0.5), (0.1, 0.2, 0.3, 0.4, 0.5), (float("nan"),), (-0.5,)):
        with pytest.raises(ValueError, match="eval_depth_quantiles"):
            LSENeRFModel(LSENeRFModelConfig(eval_depth_quantiles=bad, **small), box, 4)
    with pytest.raises(ValueError, match="1 - q >= eps"):
        LSENeRFModel(LSENeRFModelConfig(eval_depth_quantiles=(0.5, 0.95), eval_early_stop_eps=0.1, **small), box, 4)
    m = LSENeRFModel(LSENeRFModelConfig(eval_depth_quantiles=(0.5, 0.8), eval_early_stop_eps=0.1, eval_depth_interpolate=True, **small),
                     box, 4)
    assert depth_quantile_settings(m.config) == ((0.5, 0.8), True)
    LSENeRFModel(LSENeRFModelConfig(eval_depth_quantiles=[0.1, 0.2, 0.3, 0.4], eval_normals="world", **small), box, 4)


def test_the_forward_loop_refuses_instead_of_omitting_the_keys():
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig, RayBundle, evaluation
    box = torch.tensor([[-1.0, -1, -1], [1, 1, 1]])
    m = LSENeRFModel(LSENeRFModelConfig(eval_depth_quantiles=(0.5,), grid_levels=1, grid_resolution=16, log2_hashmap_size=12), box, 4)
    rb = RayBundle(origins=torch.zeros(4, 3), directions=torch.tensor([[0.0, 0, 1]]).repeat(4, 1))
    assert m.training and not evaluation.uses_count_free_route(m, 4)
    with pytest.raises(ValueError, match="eval_depth_quantiles"):
        evaluation.render_flat(m, rb)
    m.config.eval_depth_quantiles = (0.5, 0.4)               # set behind the constructor's back: refused at render time
    with pytest.raises(ValueError, match="ascending"):
        evaluation.render_flat(m, rb)


def test_exporter_arguments():
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig, pointcloud
    assert pointcloud.depth_mode("expected", None) == (False, None) and pointcloud.depth_mode("median", None) == (True, None)
    assert pointcloud.depth_mode("median", 0.25) == (True, 0.25)
    assert pointcloud.MEDIAN_QUANTILES[pointcloud.MEDIAN_COLUMN] == 0.5
    m = LSENeRFModel(LSENeRFModelConfig(grid_levels=1, grid_resolution=16, log2_hashmap_size=12),
                     torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 4)
    before = dict(vars(m.config))
    for export in (m.export_point_cloud, m.export_tsdf_mesh):
        with pytest.raises(ValueError, match="depth"):
            export([], depth="mean")
        with pytest.raises(ValueError, match="max_depth_spread"):
            export([], max_depth_spread=0.1)
        with pytest.raises(ValueError, match="max_depth_spread"):
            export([], depth="median", max_depth_spread=-1.0)
    assert dict(vars(m.config)) == before and m.training
    cfg = m.config
    with pytest.raises(RuntimeError, match="boom"):
        with pointcloud.median_settings(cfg, True):
            assert (cfg.eval_depth_quantiles, cfg.eval_depth_interpolate) == ((0.25, 0.5, 0.75), True)
            raise RuntimeError("boom")
    assert dict(vars(cfg)) == before


def _declared(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lse_hip.h")).read(), flags=re.S)
    m = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
    assert m, f"include/lse_hip.h does not declare {name}"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_binding_and_library_agree():
    from lsenerf_amd import _lib
    lib = _lib.load()
    assert lib.lse_abi_version() == 6 == _lib.LSE_ABI_VERSION                # additive: the ABI number stays
    args = _declared("lse_eval_depth_quantiles")
    assert len(args) == 13 == len(_lib.SIGNATURES["lse_eval_depth_quantiles"])
    assert args[5:9] == ["int32_t n_q", "const float *h_tau_q", "int32_t flags", "float max_spread"]
    assert args[9:] == ["float *depth_q", "uint8_t *reached", "float *depth_sel", "lse_stream_t stream"]
    seg = _declared("lse_eval_depth_quantiles_segment")
    assert len(seg) == 14 == len(_lib.SIGNATURES["lse_eval_depth_quantiles_segment"])
    assert seg[3] == "const int64_t *seg_packed" and seg[9] == "void *state" and seg[10:] == args[9:]
    for name in ("lse_eval_depth_quantiles", "lse_eval_depth_quantiles_segment"):
        assert hasattr(lib, name) and hasattr(ctypes.CDLL(_lib.DEV_LIB_PATH), name), name
    hdr = open(os.path.join(ROOT, "include", "lse_hip.h")).read()
    assert "#define LSE_DEPTH_INTERPOLATE 1" in hdr and _lib.LSE_DEPTH_INTERPOLATE == 1
    assert "median" in hdr


def test_argument_checks_need_no_device():
    from lsenerf_amd import _lib, ops
    lib = _lib.load()
    one = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    arr = lambda *v: (ctypes.c_float * len(v))(*v)

    def full(n_q=3, taus=arr(*TAUS), flags=0, spread=float("inf"), n=0, out=one):
        return lib.lse_eval_depth_quantiles(one, one, one, one, n, n_q, taus, flags, spread, out, one, None, None)

    def seg(n_q=3, taus=arr(*TAUS), flags=0, spread=float("inf"), n=0, state=one):
        return lib.lse_eval_depth_quantiles_segment(one, one, one, one, n, n_q, taus, flags, spread, state, one, one, None, None)

    for call, who in ((full, b"lse_eval_depth_quantiles"), (seg, b"lse_eval_depth_quantiles_segment")):
        assert call() == 0 and call(n_q=1) == 0 and call(n_q=4, taus=arr(0.1, 0.2, 0.3, float("inf"))) == 0
        assert call(flags=_lib.LSE_DEPTH_INTERPOLATE | (2 << 8), spread=0.5) == 0
        refused = {"n_q 0": dict(n_q=0), "n_q 5": dict(n_q=5, taus=arr(1, 2, 3, 4, 5)), "descending": dict(taus=arr(0.3, 0.2, 0.7)),
                   "equal": dict(taus=arr(0.3, 0.3, 0.7)), "zero": dict(taus=arr(0.0, 0.3, 0.7)), "nan": dict(taus=arr(0.1, float("nan"), 0.7)),
                   "null taus": dict(taus=None), "unknown flag": dict(flags=2), "sel beyond n_q": dict(flags=3 << 8),
                   "negative spread": dict(spread=-1.0), "nan spread": dict(spread=float("nan")), "negative n": dict(n=-1)}
        for what, kw in refused.items():
            assert call(**kw) == -1, what
            assert who in lib.lse_last_error(), what
    assert full(n=4, out=None) == -1 and b"null pointer" in lib.lse_last_error()
    assert seg(n=4, state=None) == -1 and b"null pointer" in lib.lse_last_error()
    # the wrappers: tensors that are not on the device, and shapes
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)
    packed = z(2, 2, dt=torch.int64)
    with pytest.raises(_lib.LseHipError, match="must live on the GPU"):
        ops.eval_depth_quantiles(z(4), z(4), z(4), packed, TAUS, z(2, 3), z(2, dt=torch.uint8))
    with pytest.raises(_lib.LseHipError, match="must live on the GPU"):
        ops.eval_depth_quantiles_segment(z(4), z(4), z(4), packed, TAUS, z(2, 2), z(2, 3), z(2, dt=torch.uint8))
    with pytest.raises(ValueError, match="depth_q"):
        ops.eval_depth_quantiles(z(4), z(4), z(4), packed, TAUS, z(2, 2), z(2, dt=torch.uint8))
    with pytest.raises(ValueError, match="state"):
        ops.eval_depth_quantiles_segment(z(4), z(4), z(4), packed, TAUS, z(3, 2), z(2, 3), z(2, dt=torch.uint8))
