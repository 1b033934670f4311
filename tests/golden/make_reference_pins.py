"""Record outputs of the reference's OWN code for the functions cameras.py, csrc/spline.hip, csrc/pose_delta.hip (SO3xR3),
log_scale_correct_kernel (csrc/metrics.hip) and the closed-form mappers of csrc/epilogue.hip restate:

    python tests/golden/make_reference_pins.py [--reference DIR] [--out DIR]

writes ref_pin_spline.npz, ref_pin_pose_delta.npz, ref_pin_scale_fit.npz and ref_pin_mappers.npz (CPU only).  Three reference modules
are plain torch / scipy behind a few imports that are not installed: ``lse_nerf/utils.py``, ``lse_nerf/interpolation_utils.py`` and
``lse_nerf/intensity_mappers.py``.  They are loaded by path under an ``lse_nerf`` package shell, a stand-in module taking the place
of every import that really fails, and then CALLED -- no line of them is restated here.  Each file holds the inputs, the reference's
outputs, for every output the reference's own distance from a float64 evaluation of the same inputs (in the metric the tests use),
``torch.__version__``, the CPU capability torch computed with and the sha256 of every reference file that was loaded.

What is loaded never sees the time clip of ``get_rgb_cameras`` (lse_nerf/ns_camera_optimizer.py does not load): the stored query
times lie inside the control times."""
import argparse
import hashlib
import importlib
import importlib.util
import json
import os
import sys
import types
from unittest import mock

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FILES = ("ref_pin_spline.npz", "ref_pin_pose_delta.npz", "ref_pin_scale_fit.npz", "ref_pin_mappers.npz")
MAX_BYTES = 100 * 1000
REFERENCE_MODULES = ("utils", "interpolation_utils", "intensity_mappers")          # in load order
# what the three files import that may be missing: stubbed only where the real import fails
THIRD_PARTY = ("nerfstudio", "nerfstudio.cameras", "nerfstudio.cameras.rays", "nerfstudio.utils", "nerfstudio.utils.writer",
               "nerfstudio.utils.rich_utils", "nerfstudio.field_components", "nerfstudio.field_components.mlp", "jax", "cv2",
               "matplotlib", "matplotlib.pyplot", "tqdm")
WELL_CONDITIONED_CAP = 1e-5


class Reference:
    """The three loaded modules (``utils``, ``interp``, ``mappers``), the names that were stubbed and the files' sha256."""

    def __init__(self, ref_dir: str):
        pkg_dir = os.path.join(ref_dir, "lse_nerf")
        if not os.path.isdir(pkg_dir):
            raise FileNotFoundError(f"no reference at {ref_dir!r} (expected {pkg_dir}): pass --reference DIR")
        dont_write = sys.dont_write_bytecode
        sys.dont_write_bytecode = True
        self.stubbed, self.sha256 = [], {}
        try:
            for name in THIRD_PARTY:
                try:
                    importlib.import_module(name)
                except Exception:
                    sys.modules[name] = mock.MagicMock(name=name)
                    self.stubbed.append(name)
            shell = types.ModuleType("lse_nerf")
            shell.__path__ = [pkg_dir]
            sys.modules["lse_nerf"] = shell
            loaded = {}
            for short in REFERENCE_MODULES:
                path = os.path.join(pkg_dir, short + ".py")
                with open(path, "rb") as f:
                    self.sha256[f"lse_nerf/{short}.py"] = hashlib.sha256(f.read()).hexdigest()
                spec = importlib.util.spec_from_file_location(f"lse_nerf.{short}", path)
                mod = importlib.util.module_from_spec(spec)
                sys.modules[spec.name] = mod
                spec.loader.exec_module(mod)
                loaded[short] = mod
        finally:                                     # the stand-ins and the shell leave sys.modules again
            sys.dont_write_bytecode = dont_write
            for k in list(sys.modules):
                if k in self.stubbed or k == "lse_nerf" or k.startswith("lse_nerf."):
                    del sys.modules[k]
        self.utils, self.interp, self.mappers = loaded["utils"], loaded["interpolation_utils"], loaded["intensity_mappers"]


def reference_sha256(ref_dir: str) -> dict:
    out = {}
    for short in REFERENCE_MODULES:
        with open(os.path.join(ref_dir, "lse_nerf", short + ".py"), "rb") as f:
            out[f"lse_nerf/{short}.py"] = hashlib.sha256(f.read()).hexdigest()
    return out


def _meta(ref: Reference) -> dict:
    return {"torch_version": np.array(torch.__version__), "cpu_capability": np.array(torch.backends.cpu.get_cpu_capability()),
            "sha256": np.array(json.dumps(ref.sha256, sort_keys=True))}


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _nmax(a, b, floor=1e-6) -> float:
    from tests.util import nmax_err
    return nmax_err(torch.as_tensor(a), torch.as_tensor(b), floor)


# ---------------------------------------------------------------------------------------------------- spline
SPLINE_QUERIES = {"k5_q300": 300, "k70_q130": 130, "k2": 40, "k6_edges": 120}
K2 = [[0.1, 0.2, 0.3, 0.0, 0.0, 0.0], [1.0, -2.0, 3.0, 0.4, -0.2, 0.9]]
# rotation parts 0, 0, (0,0,4), (0,0,4), (.3,4.5,-.2), (0,6,0): identical neighbours (dot = 1: clamped, the lerp branch), |v| > pi
# (a negative w) and a flipped pair
K6_EDGES = [[0.5, -1.0, 2.0, 0.0, 0.0, 0.0], [1.5, 0.2, -0.7, 0.0, 0.0, 0.0], [-2.0, 3.0, 0.1, 0.0, 0.0, 4.0],
            [0.0, -4.0, 1.0, 0.0, 0.0, 4.0], [3.5, 1.0, -2.5, 0.3, 4.5, -0.2], [-1.0, -1.0, 4.0, 0.0, 6.0, 0.0]]


def spline_tangents() -> dict:
    from tests import spline_fixtures as sf
    return {"k5_q300": sf._k5()[0].ctrl_tangents.detach().clone(), "k70_q130": sf._k70()[0].ctrl_tangents.detach().clone(),
            "k2": torch.tensor(K2), "k6_edges": torch.tensor(K6_EDGES)}


def spline_queries(K: int, Q: int, seed: int) -> torch.Tensor:
    """The first K on the control times 0 .. K - 1, the rest uniform in [0, K - 1]: the clip of get_rgb_cameras has nothing to do."""
    g = torch.Generator().manual_seed(seed)
    ts = torch.rand(Q, generator=g) * float(K - 1)
    ts[:K] = torch.arange(K, dtype=torch.float32)
    assert float(ts.min()) >= 0.0 and float(ts.max()) <= K - 1
    return ts


def reference_spline_chain(iu, ctrl, ctrl_ts, ts):
    return iu.quat_map_to_mtx(iu.vectorized_generalized_interpolation(iu.exp_map_to_quat_map(ctrl), ctrl_ts, ts))[:, :3, :4]


def make_spline(ref: Reference) -> dict:
    from tests import spline_fixtures as sf
    iu = ref.interp
    out = _meta(ref)
    out["fixtures"] = np.array(json.dumps(list(SPLINE_QUERIES)))
    for i, (name, tang) in enumerate(spline_tangents().items()):
        K, Q = tang.shape[0], SPLINE_QUERIES[name]
        spl = sf._synthetic_spline(tang)
        sf.check_fixture(spl)
        ctrl_ts = spl.ctrl_ts.detach().clone()
        assert torch.equal(ctrl_ts, torch.arange(K, dtype=torch.float32))
        ts = spline_queries(K, Q, seed=40 + i)
        d = sf.random_table_grads([(Q, 3, 4)], seed=7)[0]
        ctrl = tang.clone().requires_grad_(True)
        tables = reference_spline_chain(iu, ctrl, ctrl_ts, ts)
        g_ctrl, = torch.autograd.grad((tables * d).sum(), [ctrl])
        assert bool(torch.isfinite(tables).all()) and bool(torch.isfinite(g_ctrl).all())
        segments = [("rgb", ts)]
        t64 = sf.tables_f64(sf.double_copy(spl), segments)[0].detach()
        g64 = sf.autograd_f64(spl, segments, [d])[0]
        out.update({f"{name}.ctrl": _np(tang), f"{name}.ctrl_ts": _np(ctrl_ts), f"{name}.ts": _np(ts), f"{name}.tables": _np(tables),
                    f"{name}.d_tables": _np(d), f"{name}.d_ctrl": _np(g_ctrl),
                    f"{name}.dev_tables": np.float64((tables.detach().double() - t64).abs().max()),
                    f"{name}.dev_d_ctrl": np.float64(_nmax(g_ctrl, g64))})
    # the single functions, on the rotation vectors of the edge fixtures: quaternions, slerp of neighbours, matrices, tangents
    rot = torch.cat([torch.tensor(K6_EDGES)[:, 3:], spline_tangents()["k5_q300"][:, 3:], torch.tensor(K2)[:, 3:]])
    quat = iu.exp_map_to_quat(rot)
    out["fn.rotvec"], out["fn.quat"] = _np(rot), _np(quat)
    out["fn.rot_mat"] = _np(iu.quat_to_rot_mat(quat))
    out["fn.slerp_t"] = np.array([0.0, 1.0, 0.5, 0.123], dtype=np.float32)
    out["fn.slerp"] = np.stack([_np(iu.slerp(quat[:-1], quat[1:], torch.full((len(quat) - 1, 1), float(t)))) for t in out["fn.slerp_t"]])
    tang = torch.cat([torch.tensor(K6_EDGES), spline_tangents()["k5_q300"], torch.tensor(K2)])
    mats = iu.hom_exp_map_SO3xR3(tang)
    out["fn.matrix"] = _np(mats)
    out["fn.tangent"] = np.stack([_np(iu.matrix_to_tangent_vector(M)) for M in mats]).astype(np.float32)
    return out


# ---------------------------------------------------------------------------------------------------- pose delta
POSE_MAGS = (0.0101, None, 0.005, 0.011, 0.02, 0.3, 1.0, 3.1, 0.0099, 1e-3, 0.05, 2.0, 1e-5, 0.00999, 0.7, 0.1)


def pose_adjustments(C: int = 64) -> torch.Tensor:
    """[C, 6] = (v, w): |w| by POSE_MAGS on random axes (|w|^2 on both sides of the 1e-4 clamp), translations uniform in +-3; row 1
    is all zeros, row 17 has w = 0 and v != 0."""
    g = torch.Generator().manual_seed(64)
    axis = torch.randn(C, 3, generator=g, dtype=torch.float64)
    axis = axis / axis.norm(dim=1, keepdim=True)
    v = (torch.rand(C, 3, generator=g, dtype=torch.float64) * 2 - 1) * 3
    p = torch.zeros(C, 6, dtype=torch.float64)
    for c in range(C):
        m = POSE_MAGS[c % len(POSE_MAGS)]
        p[c, :3] = v[c]
        if m is not None:
            p[c, 3:] = axis[c] * m
    p[1] = 0.0
    p = p.float()
    t2 = (p[:, 3:] * p[:, 3:]).sum(1)
    assert int((t2 < 1e-4).sum()) >= 8 and int((t2 > 1e-4).sum()) >= 8
    assert float(p[1].abs().max()) == 0.0 and float(p[17, 3:].abs().max()) == 0.0 and float(p[17, :3].abs().min()) > 0.0
    return p


def make_pose_delta(ref: Reference) -> dict:
    from tests import pose_delta_fixtures as pf
    p = pose_adjustments()
    C = p.shape[0]
    d = pf.random_table_grad(C)
    leaf = p.clone().requires_grad_(True)
    tables = ref.interp.hom_exp_map_SO3xR3(leaf)[:, :3, :4]
    g, = torch.autograd.grad((tables * d).sum(), [leaf])
    assert bool(torch.isfinite(tables).all()) and bool(torch.isfinite(g).all())
    base = torch.eye(4)[:3][None].repeat(C, 1, 1)
    t64 = pf.tables_f64(p, base, "SO3xR3")
    g64 = pf.autograd_f64(p, base, "SO3xR3", None, d)
    out = _meta(ref)
    out.update({"adj": _np(p), "tables": _np(tables), "d_tables": _np(d), "d_adj": _np(g),
                "dev_tables": np.float64((tables.detach().double() - t64).abs().max()), "dev_d_adj": np.float64(_nmax(g, g64))})
    return out


# ---------------------------------------------------------------------------------------------------- scale fit
def _fit_f64(gt: np.ndarray, pred: np.ndarray):
    """``(a, b, corrected, gray)`` in float64 at the float32 inputs: torch.linalg.lstsq of log(gray + EPS) ~ a log(r + g + EPS) + b."""
    gt64, pred64 = torch.from_numpy(gt).double(), torch.from_numpy(pred).double()
    gray = gt64[..., 0] * 0.2989 + gt64[..., 1] * 0.5870 + gt64[..., 2] * 0.1140
    x = torch.log(pred64[..., 0] + pred64[..., 1] + 1e-6).reshape(-1)
    y = torch.log(gray + 1e-6).reshape(-1)
    X = torch.stack([torch.ones_like(x), x], 1)
    beta = torch.linalg.lstsq(X, y[:, None]).solution[:, 0]
    b, a = float(beta[0]), float(beta[1])
    return a, b, torch.exp(a * x + b).reshape(gray.shape).numpy(), gray.numpy()


PRED_LEVELS = 32


def scale_fit_inputs(seed: int = 0) -> dict:
    """The stored images, kept small: the well-conditioned predictions are stored as their numerators ``*_n32`` (uint8 [H, W, 2]: red
    and green are n / 32 exactly, blue, which the fit never reads, is 0: ``prediction``), and the 8-bit ground truths are a grey
    level in steps of 16 with a tint of +-1 per channel.  The small float32 ground truth is arbitrary float32."""
    rng = np.random.default_rng(seed)
    out = {}
    for tag, (h, w) in (("s24", (24, 40)), ("s72", (72, 120))):
        n = rng.integers(1, PRED_LEVELS, (h, w, 2)).astype(np.uint8)
        law = 0.7 * (0.5 * n.sum(-1) / PRED_LEVELS) ** 1.3 * rng.uniform(0.8, 1.25, (h, w))
        tint = rng.integers(-1, 2, (h, w, 3))
        u8 = np.clip(16 * np.round(law[..., None] * 255.0 / 16) + tint, 1, 255).astype(np.uint8)
        out[f"pred_{tag}_n32"], out[f"gt_{tag}_u8"] = n, u8
    h, w = 24, 40
    law = 0.7 * (0.5 * out["pred_s24_n32"].sum(-1) / PRED_LEVELS) ** 1.3
    out["gt_s24_f32"] = np.clip(law[..., None] * rng.uniform(0.8, 1.25, (h, w, 3)), 0.0, 1.0).astype(np.float32)
    zeros = out["gt_s24_u8"].copy()
    zeros[9:15, 20:30] = 0                                     # what a mask leaves: log(0 + EPS)
    out["gt_s24_u8_zeros"] = zeros
    ill = np.zeros((h, w, 3), dtype=np.float32)
    ill[..., :2] = (0.3 + 1e-3 * rng.uniform(size=(h, w, 2))).astype(np.float32)
    out["pred_s24_ill"] = ill
    return out


def prediction(arr: np.ndarray) -> np.ndarray:
    """The float32 [H, W, 3] prediction of a stored array: numerators over 32 (exact in float32), or the array itself."""
    if arr.dtype != np.uint8:
        return arr
    pred = np.zeros(arr.shape[:2] + (3,), dtype=np.float32)
    pred[..., :2] = arr.astype(np.float32) / np.float32(PRED_LEVELS)
    return pred


# name -> (ground truth array, prediction array, gt as float32 = u8 / 255, ill conditioned)
SCALE_CASES = {"s24_f32": ("gt_s24_f32", "pred_s24_n32", False), "s24_u8": ("gt_s24_u8", "pred_s24_n32", False),
               "s24_u8_zeros": ("gt_s24_u8_zeros", "pred_s24_n32", False), "s72_u8": ("gt_s72_u8", "pred_s72_n32", False),
               "s24_ill": ("gt_s24_u8", "pred_s24_ill", True)}


def gt_as_float(gt: np.ndarray) -> np.ndarray:
    """uint8 / 255 as a dataset hands it over (a true float32 division); float32 as it is."""
    return gt if gt.dtype == np.float32 else (torch.from_numpy(gt).float() / 255.0).numpy()


def make_scale_fit(ref: Reference, seed: int = 0) -> dict:
    U = ref.utils
    arrays = scale_fit_inputs(seed)
    out = _meta(ref)
    out.update(arrays)
    cases = []
    for name, (gt_key, pred_key, ill) in SCALE_CASES.items():
        gt, pred = gt_as_float(arrays[gt_key]), prediction(arrays[pred_key])
        gt_t, pred_t = torch.from_numpy(gt), torch.from_numpy(pred)
        gray = U.to_gray(gt_t)                                                     # [H, W, 1]
        x_in = pred_t[..., 0:1] + pred_t[..., 1:2]
        gt_log, pred_log = torch.log(gray + U.EPS), torch.log(x_in + U.EPS)
        a, b = U.solve_normal_equations(pred_log, gt_log)
        corrected = U.correct_img_scale(gray, x_in)
        a64, b64, corr64, gray64 = _fit_f64(gt, pred)
        dev = {"gray": float(np.abs(_np(gray)[..., 0].astype(np.float64) - gray64).max()), "a": abs(float(a) - a64), "b": abs(float(b) - b64),
               "corrected": float((np.abs(_np(corrected)[..., 0].astype(np.float64) - corr64) / corr64).max())}
        if not ill:
            worst = max(dev["corrected"], dev["a"] / abs(a64), dev["b"] / abs(b64))
            assert worst <= WELL_CONDITIONED_CAP, f"{name}: the reference is {worst:.2e} from the float64 fit: change the seed, not the cap"
        h, w = gt.shape[:2]
        cases.append({"name": name, "gt": gt_key, "pred": pred_key, "H": h, "W": w, "ill_conditioned": ill, "dev": dev})
        if not ill:                                   # (the ill-conditioned case shares its ground truth with s24_u8)
            out[f"{name}.gray"] = _np(gray)[..., 0]
        out[f"{name}.coef"] = np.array([float(a), float(b)], dtype=np.float32)
        out[f"{name}.corrected"] = _np(corrected)[..., 0]
    out["cases"] = np.array(json.dumps(cases))
    return out


# ---------------------------------------------------------------------------------------------------- mappers
POWS = (0.6, 1.0, 1.7)
MAPPER_NAMES = ("identity", "gt") + tuple(f"powpow_{p}" for p in POWS)


def mapper_inputs():
    """x [258, 3]: 257 rays in [0.002, 1.2] -- above the clamp at 1e-5 that lsenerf.py (not loadable) puts in front of and behind the
    mapper, and so is every mapped value (0.002^1.7 = 2.6e-5) -- plus the row (0, 0, 0); targets uniform in [0, 1)."""
    g = torch.Generator().manual_seed(257)
    x = 0.002 + torch.rand(258, 3, generator=g) * 1.198
    x[:3] = torch.tensor([[0.002, 1.2, 1.0], [1.0, 1.0, 1.0], [0.5, 0.002, 1.2]])
    x[257] = 0.0
    return x.float(), torch.rand(258, 3, generator=g)


def _mapper_eval(make, x, gt, rows, dtype):
    """(y, loss, dx, dpow) of one mapper over x[:rows] in ``dtype``; ``make(dtype)`` -> (callable, parameter or None)."""
    leaf = x[:rows].to(dtype).clone().requires_grad_(True)
    fn, param = make(dtype)
    y = fn(leaf)
    loss = F.mse_loss(y, gt[:rows].to(dtype))
    grads = torch.autograd.grad(loss, [leaf] + ([param] if param is not None else []))
    return y.detach(), loss.detach(), grads[0], (grads[1] if param is not None else None)


def make_mappers(ref: Reference) -> dict:
    M = ref.mappers
    x, gt = mapper_inputs()
    out = _meta(ref)
    out.update({"x": _np(x), "gt": _np(gt), "names": np.array(json.dumps(list(MAPPER_NAMES)))})

    def reference_mapper(name):
        def make(dtype):
            assert dtype == torch.float32
            if name == "identity":
                return M.IdentityMapper(), None
            if name == "gt":
                return M.GT_Mapper(), None
            m = M.Powpow()
            with torch.no_grad():
                m.pow_coeff.fill_(float(name.split("_")[1]))
            return m, m.pow_coeff
        return make

    def float64_mapper(name):
        def make(dtype):
            if name == "identity":
                return (lambda v: v), None
            if name == "gt":
                return (lambda v: v ** (1 / 2.4)), None
            p = torch.tensor([float(name.split("_")[1])]).to(dtype).requires_grad_(True)       # the float32 coefficient, widened
            return (lambda v: v ** p), p
        return make

    for name in MAPPER_NAMES:
        for tag, rows in (("all", 258), ("pos", 257)):
            y, loss, dx, dpow = _mapper_eval(reference_mapper(name), x, gt, rows, torch.float32)
            y64, loss64, dx64, dpow64 = _mapper_eval(float64_mapper(name), x, gt, rows, torch.float64)
            finite = torch.isfinite(dx)
            assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(loss))
            assert torch.equal(finite, torch.isfinite(dx64)) and (tag == "all" or bool(finite.all()))
            if tag == "all":
                out[f"{name}.y"] = _np(y)
                out[f"{name}.dev_y"] = np.float64((y.double() - y64).abs().max())
            out[f"{name}.loss_{tag}"] = np.float32(loss)
            out[f"{name}.dx_{tag}"] = _np(dx)
            out[f"{name}.dev_loss_{tag}"] = np.float64(abs(float(loss) - float(loss64)) / float(loss64))
            out[f"{name}.dev_dx_{tag}"] = np.float64(_nmax(dx[finite], dx64[finite]))
            if dpow is not None:
                assert bool(torch.isfinite(dpow).all())
                out[f"{name}.dpow_{tag}"] = _np(dpow)
                out[f"{name}.dev_dpow_{tag}"] = np.float64(_nmax(dpow, dpow64))
    return out


# ---------------------------------------------------------------------------------------------------- all four
MAKERS = {"ref_pin_spline.npz": make_spline, "ref_pin_pose_delta.npz": make_pose_delta, "ref_pin_scale_fit.npz": make_scale_fit,
          "ref_pin_mappers.npz": make_mappers}


def generate(ref_dir: str, only=None, verbose: bool = False) -> dict:
    """{file name: {key: numpy array}} of every pin, computed on one thread (the reference's normal equations are a float32 matrix
    product whose summation order follows the thread count)."""
    ref = Reference(ref_dir)
    if verbose:
        print("stubbed (their import failed):", ", ".join(ref.stubbed) if ref.stubbed else "nothing")
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return {name: make(ref) for name, make in MAKERS.items() if only is None or name in only}
    finally:
        torch.set_num_threads(threads)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", default="/root/reference", help="the checkout of ubc-vision/LSENeRF to load (default: %(default)s)")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    if not os.path.isdir(os.path.join(args.reference, "lse_nerf")):
        sys.exit(f"make_reference_pins: no reference at {args.reference!r} (expected {args.reference}/lse_nerf): pass --reference DIR")
    pins = generate(args.reference, verbose=True)
    for name, arrays in pins.items():
        path = os.path.join(args.out, name)
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        devs = {k: float(v) for k, v in arrays.items() if ".dev_" in k or k.startswith("dev_")}
        print(f"{name}: {size} bytes", {k: f"{v:.2e}" for k, v in devs.items()})
        if name == "ref_pin_scale_fit.npz":
            for c in json.loads(str(arrays["cases"])):
                print("   ", c["name"], "ill" if c["ill_conditioned"] else "", {k: f"{v:.2e}" for k, v in c["dev"].items()})
        assert size <= MAX_BYTES, f"{name} is {size} bytes, the limit is {MAX_BYTES}"


if __name__ == "__main__":
    main()
