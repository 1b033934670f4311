"""The recorded outputs of the reference's own code (tests/golden/ref_pin_*.npz) on the CPU: the generator reproduces the committed
files; cameras.py and model.py against them; the float64 twins the GPU tests are held to against them, within the reference's own
recorded deviation from float64; and every comparison of tests/reference_pins.py shown to reject mutated copies of the data."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pose_delta_fixtures as pf
from tests import reference_pins as rp
from tests import spline_fixtures as sf
from tests.test_eval_set_cpu import scale_fit_f64
from tests.util import nmax_err

REFERENCE = os.environ.get("LSE_REFERENCE_DIR", "/root/reference")
SPLINE, POSE, SCALE, MAPPERS = (rp.load(f) for f in rp.FILES)


def _generator():
    spec = importlib.util.spec_from_file_location("make_reference_pins", os.path.join(rp.GOLDEN, "make_reference_pins.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------------------------------------------- 1. the files, regeneration
def test_the_committed_files_are_small_and_say_what_they_were_recorded_with():
    for name in rp.FILES:
        assert os.path.getsize(os.path.join(rp.GOLDEN, name)) <= rp.MAX_BYTES, name
        rec = rp.recorded_with(rp.load(name))
        assert rec["torch_version"] and rec["cpu_capability"]
        assert set(rec["sha256"]) == {"lse_nerf/utils.py", "lse_nerf/interpolation_utils.py", "lse_nerf/intensity_mappers.py"}
        assert all(len(v) == 64 for v in rec["sha256"].values())
    assert rp.spline_fixtures() == ["k5_q300", "k70_q130", "k2", "k6_edges"]
    assert [c["name"] for c in rp.scale_cases(ill=True)] == ["s24_ill"] and len(rp.scale_cases(ill=False)) == 4
    assert rp.mapper_names() == ["identity", "gt", "powpow_0.6", "powpow_1.0", "powpow_1.7"]


def _deviation_of(pin, key):
    """The recorded deviation that bounds output ``key`` of a file when torch differs from the recording one, or None for an input
    (always equal).  Deviations are in the metric of the output: max abs (tables, y, gray), nmax_err (gradients), relative (loss,
    corrected), absolute (coef)."""
    head, _, leaf = key.rpartition(".")
    prefix = head + "." if head else ""
    for out, dev, metric in (("tables", "dev_tables", "abs"), ("d_ctrl", "dev_d_ctrl", "nmax"), ("d_adj", "dev_d_adj", "nmax"), ("y", "dev_y", "abs")):
        if leaf == out:
            return float(pin[prefix + dev]), metric
    for stem, metric in (("loss_", "rel"), ("dx_", "nmax"), ("dpow_", "nmax")):
        if leaf.startswith(stem) and prefix + "dev_" + leaf in pin:
            return float(pin[prefix + "dev_" + leaf]), metric
    return None


def test_the_generator_reproduces_the_committed_files():
    """Bit for bit where torch's version and CPU capability are the recording ones; otherwise every output within the reference's
    recorded deviation from float64 (another torch is another float32 evaluation of the same expressions)."""
    if not os.path.isdir(os.path.join(REFERENCE, "lse_nerf")):
        pytest.skip(f"no reference checkout at {REFERENCE}")
    gen = _generator()
    recorded = rp.recorded_with(SPLINE)
    now = gen.reference_sha256(REFERENCE)
    if now != recorded["sha256"]:
        pytest.skip(f"the reference at {REFERENCE} is not the recorded one: sha256 {now} against {recorded['sha256']}")
    fresh = gen.generate(REFERENCE)
    same_arithmetic = (recorded["torch_version"] == torch.__version__ and recorded["cpu_capability"] == torch.backends.cpu.get_cpu_capability())
    assert set(fresh) == set(rp.FILES)
    for name in rp.FILES:
        pin, new = rp.load(name), fresh[name]
        assert set(new) == set(pin), (name, set(new) ^ set(pin))
        cases = {c["name"]: c for c in json.loads(str(pin["cases"]))} if "cases" in pin else {}
        for k in pin:
            a, b = np.asarray(new[k]), pin[k]
            if same_arithmetic or k in ("sha256", "fixtures", "names"):
                assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (name, k)
                continue
            if k in ("torch_version", "cpu_capability", "cases") or "dev_" in k:
                continue
            assert a.shape == b.shape, (name, k)
            dev = _deviation_of(pin, k)
            case = cases.get(k.rpartition(".")[0])
            if case is not None:
                leaf = k.rpartition(".")[2]
                if leaf == "coef":
                    assert abs(float(a[0]) - float(b[0])) <= case["dev"]["a"] and abs(float(a[1]) - float(b[1])) <= case["dev"]["b"], (name, k)
                elif leaf == "gray":
                    assert float(np.abs(a.astype(np.float64) - b).max()) <= case["dev"]["gray"], (name, k)
                else:
                    assert float((np.abs(a.astype(np.float64) - b) / b).max()) <= case["dev"]["corrected"], (name, k)
            elif dev is None:
                assert np.array_equal(a, b), (name, k)          # an input
            else:
                bar, metric = dev
                fin = np.isfinite(b)
                assert np.array_equal(np.isfinite(a), fin), (name, k)
                a64, b64 = a[fin].astype(np.float64), b[fin].astype(np.float64)
                err = float(np.abs(a64 - b64).max()) if a64.size else 0.0
                scale = {"abs": 1.0, "rel": float(np.abs(b64).max()), "nmax": max(1e-6, float(np.abs(b64).max()))}[metric]
                assert err <= bar * scale, (name, k, err, bar, metric)


def test_the_generator_names_a_missing_reference(tmp_path):
    gen = _generator()
    with pytest.raises(FileNotFoundError, match="no reference at"):
        gen.Reference(str(tmp_path))


# ---------------------------------------------------------------------------------------------------- 2. cameras.py and model.py
def _cameras_chain(fx, dtype=torch.float32, grad=False):
    from lsenerf_amd import cameras as cam
    ctrl = rp.t(SPLINE[f"{fx}.ctrl"]).to(dtype).requires_grad_(grad)
    ctrl_ts, ts = rp.t(SPLINE[f"{fx}.ctrl_ts"]), rp.t(SPLINE[f"{fx}.ts"])
    ts = torch.clip(ts, ctrl_ts[0], ctrl_ts[-1])                 # get_rgb_cameras' clip: the recorded times already lie inside
    assert torch.equal(ts, rp.t(SPLINE[f"{fx}.ts"]))
    tables = cam.quat_map_to_mtx(cam.vectorized_generalized_interpolation(cam.exp_map_to_quat_map(ctrl), ctrl_ts, ts))[:, :3, :4]
    return ctrl, tables


@pytest.mark.parametrize("fx", rp.spline_fixtures())
def test_cameras_py_spline_chain_equals_the_recorded_tables_bit_for_bit(fx):
    ctrl, tables = _cameras_chain(fx, grad=True)
    rp.spline_tables_match(tables.detach(), SPLINE, fx, 0.0)
    # and get_rgb_cameras itself, over a spline with these control points
    spl = sf._synthetic_spline(rp.t(SPLINE[f"{fx}.ctrl"]))
    sf.check_fixture(spl)
    assert torch.equal(spl.ctrl_ts, rp.t(SPLINE[f"{fx}.ctrl_ts"]))
    rp.spline_tables_match(spl.get_rgb_cameras(rp.t(SPLINE[f"{fx}.ts"])).detach(), SPLINE, fx, 0.0)
    # its float32 autograd: another order of the same sums
    g, = torch.autograd.grad((tables * rp.t(SPLINE[f"{fx}.d_tables"])).sum(), [ctrl])
    err = rp.spline_grad_match(g, SPLINE, fx, rp.spline_grad_bar(SPLINE, fx))
    print(fx, "cameras.py float32 autograd against the recorded one:", err)


def test_cameras_py_single_functions_equal_the_recorded_outputs_bit_for_bit():
    from lsenerf_amd import cameras as cam
    rot = rp.t(SPLINE["fn.rotvec"])
    quat = cam.exp_map_to_quat(rot)
    rp.max_abs_within(quat, SPLINE["fn.quat"], 0.0, "exp_map_to_quat")
    rp.max_abs_within(cam.quat_to_rot_mat(quat), SPLINE["fn.rot_mat"], 0.0, "quat_to_rot_mat")
    for i, tt in enumerate(SPLINE["fn.slerp_t"].tolist()):
        got = cam.slerp(quat[:-1], quat[1:], torch.full((len(quat) - 1, 1), float(tt)))
        rp.max_abs_within(got, SPLINE["fn.slerp"][i], 0.0, f"slerp t = {tt}")
    mats = rp.t(SPLINE["fn.matrix"])
    got = torch.stack([cam.matrix_to_tangent_vector(M) for M in mats])
    rp.max_abs_within(got, SPLINE["fn.tangent"], 0.0, "matrix_to_tangent_vector")
    assert float(rot[0].abs().max()) == 0.0 and float(rp.t(SPLINE["fn.tangent"])[0, 3:].abs().max()) == 0.0      # the zero rotation is among them


def test_cameras_py_so3xr3_is_within_twice_the_references_own_deviation():
    from lsenerf_amd import cameras as cam
    adj = rp.t(POSE["adj"]).requires_grad_(True)
    tables = cam.hom_exp_map_SO3xR3(adj)[:, :3, :4]
    err = rp.pose_tables_match(tables.detach(), POSE, 2.0 * float(POSE["dev_tables"]))
    g, = torch.autograd.grad((tables * rp.t(POSE["d_tables"])).sum(), [adj])
    gerr = rp.pose_grad_match(g, POSE, 2.0 * float(POSE["dev_d_adj"]))
    print("hom_exp_map_SO3xR3 against the recorded tables", err, "bar", 2.0 * float(POSE["dev_tables"]), "gradient", gerr)
    t2 = (adj.detach()[:, 3:] ** 2).sum(1)
    assert int((t2 < 1e-4).sum()) >= 8 and int((t2 > 1e-4).sum()) >= 8
    assert float(adj.detach()[1].abs().max()) == 0.0 and float(adj.detach()[17, 3:].abs().max()) == 0.0 < float(adj.detach()[17, :3].abs().min())


def _module_eval(make, name, tag):
    x, gt = rp.t(MAPPERS["x"]), rp.t(MAPPERS["gt"])
    rows = 258 if tag == "all" else 257
    leaf = x[:rows].clone().requires_grad_(True)
    m = make()
    p = rp.mapper_pow(name)
    params = []
    if p is not None:
        with torch.no_grad():
            m.pow_coeff.fill_(p)
        params = [m.pow_coeff]
    y = m(leaf)
    loss = F.mse_loss(y, gt[:rows])
    grads = torch.autograd.grad(loss, [leaf] + params)
    return {"y": y.detach(), "loss": loss.detach(), "dx": grads[0], "dpow": grads[1] if params else None}


@pytest.mark.parametrize("tag", ["all", "pos"])
@pytest.mark.parametrize("name", rp.mapper_names())
def test_model_py_mappers_are_within_twice_the_references_own_deviation(name, tag):
    from lsenerf_amd import model as mdl
    make = {"identity": mdl.IdentityMapper, "gt": mdl.GT_Mapper}.get(name, mdl.Powpow)
    bars = {"loss": 2.0 * float(MAPPERS[f"{name}.dev_loss_{tag}"]), "dx": 2.0 * float(MAPPERS[f"{name}.dev_dx_{tag}"]),
            "y": 2.0 * float(MAPPERS[f"{name}.dev_y"])}
    if rp.mapper_pow(name) is not None:
        bars["dpow"] = 2.0 * float(MAPPERS[f"{name}.dev_dpow_{tag}"])
    res = rp.mapper_match(_module_eval(make, name, tag), MAPPERS, name, tag, bars)
    print(name, tag, res)
    if tag == "all" and name in ("gt", "powpow_0.6"):           # an exponent below 1: d x^p / d x is infinite at 0, recorded as it came
        assert not bool(np.isfinite(MAPPERS[f"{name}.dx_all"][-1]).any())


@pytest.mark.parametrize("case", rp.scale_cases(ill=False), ids=lambda c: c["name"])
def test_model_py_to_gray_is_within_twice_the_references_own_deviation(case):
    from lsenerf_amd import model as mdl
    _, gt_f, _ = rp.scale_inputs(SCALE, case)
    bar = 2.0 * case["dev"]["gray"]
    e1 = rp.gray_match(mdl.to_gray(torch.from_numpy(gt_f))[..., 0], SCALE, case, bar)
    e2 = rp.gray_match(mdl.ToGrayGT()(torch.from_numpy(gt_f))[..., 0], SCALE, case, bar)
    print(case["name"], "to_gray", e1, "ToGrayGT", e2, "bar", bar)


# ---------------------------------------------------------------------------------------------------- 3. the float64 twins
@pytest.mark.parametrize("fx", rp.spline_fixtures())
def test_spline_float64_twin_is_within_the_recorded_deviation(fx):
    spl = sf._synthetic_spline(rp.t(SPLINE[f"{fx}.ctrl"]))
    segments = [("rgb", rp.t(SPLINE[f"{fx}.ts"]))]
    t64 = sf.tables_f64(sf.double_copy(spl), segments)[0].detach()
    dev = float(SPLINE[f"{fx}.dev_tables"])
    err = float((t64 - rp.t(SPLINE[f"{fx}.tables"]).double()).abs().max())
    g64 = sf.autograd_f64(spl, segments, [rp.t(SPLINE[f"{fx}.d_tables"])])[0]
    gerr = nmax_err(rp.t(SPLINE[f"{fx}.d_ctrl"]), g64)
    print(fx, "tables_f64", err, "recorded", dev, "autograd_f64", gerr, "recorded", float(SPLINE[f"{fx}.dev_d_ctrl"]))
    assert err <= dev <= 1e-6 and gerr <= float(SPLINE[f"{fx}.dev_d_ctrl"]) <= 1e-6
    assert torch.equal(g64[rp.zero_rotation_points(SPLINE, fx), 3:], torch.zeros_like(g64[rp.zero_rotation_points(SPLINE, fx), 3:]))


def test_pose_delta_float64_twin_is_within_the_recorded_deviation():
    adj, d = rp.t(POSE["adj"]), rp.t(POSE["d_tables"])
    base = torch.eye(4)[:3][None].repeat(adj.shape[0], 1, 1)
    err = float((pf.tables_f64(adj, base, "SO3xR3") - rp.t(POSE["tables"]).double()).abs().max())
    gerr = nmax_err(rp.t(POSE["d_adj"]), pf.autograd_f64(adj, base, "SO3xR3", None, d))
    print("pose delta twin: tables", err, "recorded", float(POSE["dev_tables"]), "gradient", gerr, "recorded", float(POSE["dev_d_adj"]))
    assert err <= float(POSE["dev_tables"]) <= 1e-6 and gerr <= float(POSE["dev_d_adj"]) <= 2e-6


@pytest.mark.parametrize("case", rp.scale_cases(), ids=lambda c: c["name"])
def test_scale_fit_float64_twin_is_within_the_recorded_deviation(case):
    """scale_fit_f64 solves the normal equations in float64, the recorded deviations are against torch.linalg.lstsq in float64: the
    two agree to 1e-9 of the deviation's scale where the system is well conditioned."""
    _, gt_f, pred = rp.scale_inputs(SCALE, case)
    a64, b64, corr64, gray64 = scale_fit_f64(gt_f, pred)
    slack = 1e-9 if not case["ill_conditioned"] else 1e-6
    dev = case["dev"]
    ea, eb = rp.coef_match(torch.tensor([a64, b64], dtype=torch.float64), SCALE, case, dev["a"] + slack, dev["b"] + slack)
    ec = rp.corrected_match(torch.from_numpy(corr64), SCALE, case, corr64, dev["corrected"] + slack)
    print(case["name"], "twin against the recorded fit: a", ea, "b", eb, "corrected", ec, "recorded", dev)
    if case["ill_conditioned"]:
        assert dev["corrected"] > 1e-3                          # the reference's float32 normal equations, written down
    else:
        rp.gray_match(torch.from_numpy(gray64), SCALE, case, dev["gray"] + 1e-12)
        assert max(dev["corrected"], dev["a"] / abs(a64), dev["b"] / abs(b64)) <= 1e-5


EPILOGUE_DESCRIPTOR = {"identity": "plain_rgb_key", "gt": "evs_rgb_gt_gray", "powpow_0.6": "co_map_powpow_learned"}


@pytest.mark.filterwarnings("ignore:Using a target size")        # (the two throw-away event rays of the descriptors without ev_one_dim)
@pytest.mark.parametrize("name", list(EPILOGUE_DESCRIPTOR))
def test_epilogue_float64_reference_is_within_the_recorded_deviation(name):
    """tests/epilogue_cases.evaluate (oracle/losses.py in float64: what the loss-epilogue kernels are held to), colour side, on the
    257 recorded rays above the clamp, where the clamps of lsenerf.py are the identity."""
    from tests import epilogue_cases as ec
    x, gt = rp.t(MAPPERS["x"])[:257], rp.t(MAPPERS["gt"])[:257]
    inp = dict(ec.make_inputs(EPILOGUE_DESCRIPTOR[name], 257, 2))
    inp.update(col=x, col_gt=gt, pow_rgb=torch.tensor([0.6]))
    ref = ec.evaluate(EPILOGUE_DESCRIPTOR[name], inp, torch.float64)
    up = ec.UPSTREAM[0]
    assert abs(float(ref["rgb_loss"]) - float(MAPPERS[f"{name}.loss_pos"])) / float(ref["rgb_loss"]) <= float(MAPPERS[f"{name}.dev_loss_pos"]) + 1e-12
    assert nmax_err(rp.t(MAPPERS[f"{name}.dx_pos"]), ref["d_col"] / up) <= float(MAPPERS[f"{name}.dev_dx_pos"]) + 1e-12
    if name.startswith("powpow"):
        assert nmax_err(rp.t(MAPPERS[f"{name}.dpow_pos"]), ref["d_pow_rgb"] / up) <= float(MAPPERS[f"{name}.dev_dpow_pos"]) + 1e-12


# ---------------------------------------------------------------------------------------------------- 4. mutations
def _rejects(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


def test_the_spline_comparisons_reject_mutated_data():
    fx = "k6_edges"
    tables = rp.t(SPLINE[f"{fx}.tables"])
    rp.spline_tables_match(tables, SPLINE, fx, 0.0)
    K = SPLINE[f"{fx}.ctrl"].shape[0]
    swapped = tables.clone()
    swapped[[K, K + 1]] = tables[[K + 1, K]]                     # a table row swapped with its neighbour
    unflipped = tables.clone()                                   # the flipped pair (control points 1, 2) taken the long way round:
    ts = rp.t(SPLINE[f"{fx}.ts"])                                # slerp without the shortest-arc negation, in float64
    from lsenerf_amd import cameras as cam
    q = cam.exp_map_to_quat(rp.t(SPLINE[f"{fx}.ctrl"]).double()[:, 3:])
    inside = (ts > 1.0) & (ts < 2.0)
    assert int(inside.sum()) >= 5 and float((q[1] * q[2]).sum()) < 0
    th = torch.acos((q[1] * q[2]).sum())
    f = (ts[inside].double() - 1.0)[:, None]
    long_way = (torch.sin(th - th * f) * q[1] + torch.sin(th * f) * q[2]) / torch.sin(th)
    unflipped[inside, :, :3] = cam.quat_to_rot_mat(long_way).float()
    for bar in (0.0, 1e-5):
        _rejects(rp.spline_tables_match, swapped, SPLINE, fx, bar)
        _rejects(rp.spline_tables_match, unflipped, SPLINE, fx, bar)
    grad = rp.t(SPLINE[f"{fx}.d_ctrl"])
    bar = rp.spline_grad_bar(SPLINE, fx)
    rp.spline_grad_match(grad, SPLINE, fx, bar)
    leak = grad.clone()
    leak[0, 3:] = 1e-12                                          # a nonzero rotation gradient on the zero-rotation control point
    _rejects(rp.spline_grad_match, leak, SPLINE, fx, bar)
    lost = grad.clone()
    lost[K - 1] = grad[K - 1] * (1.0 - 1e-4)                     # the last control point lost one query in ten thousand
    assert float(grad[K - 1].abs().max()) > 0.05 * float(grad.abs().max())
    _rejects(rp.spline_grad_match, lost, SPLINE, fx, bar)


def test_the_pose_delta_comparisons_reject_mutated_data():
    tables, grad = rp.t(POSE["tables"]), rp.t(POSE["d_adj"])
    bar_t, bar_g = 1e-5 + float(POSE["dev_tables"]), 1e-6 + 4e-6 + float(POSE["dev_d_adj"])
    rp.pose_tables_match(tables, POSE, bar_t)
    rp.pose_grad_match(grad, POSE, bar_g)
    transposed = tables.clone()
    transposed[:, :, :3] = tables[:, :, :3].transpose(1, 2)      # exp(-w) in place of exp(w)
    _rejects(rp.pose_tables_match, transposed, POSE, bar_t)
    se3 = tables.clone()                                         # the translation of the SE3 exponential, V v, in place of v
    se3[:, :, 3] = pf.exp_map(rp.t(POSE["adj"]).double(), "SE3")[1].float()
    assert int(((se3 - tables).abs().amax((1, 2)) > bar_t).sum()) < tables.shape[0]      # (rows with w = 0 agree)
    _rejects(rp.pose_tables_match, se3, POSE, bar_t)
    swapped = grad.clone()
    swapped[:, :3], swapped[:, 3:] = grad[:, 3:], grad[:, :3]    # (v, w) gradients in each other's place
    _rejects(rp.pose_grad_match, swapped, POSE, bar_g)
    dropped = grad.clone()
    dropped[17] = 0.0                                            # the row with w = 0, v != 0 skipped as if it were the all-zero row
    _rejects(rp.pose_grad_match, dropped, POSE, bar_g)


def test_the_scale_fit_comparisons_reject_mutated_data():
    case = next(c for c in rp.scale_cases() if c["name"] == "s72_u8")
    _, gt_f, pred = rp.scale_inputs(SCALE, case)
    a64, b64, corr64, _ = scale_fit_f64(gt_f, pred)
    dev = case["dev"]
    coef, corrected, gray = rp.t(SCALE["s72_u8.coef"]), rp.t(SCALE["s72_u8.corrected"]), rp.t(SCALE["s72_u8.gray"])
    bars = (1e-6 + dev["a"], 1e-6 + dev["b"])
    rp.coef_match(coef, SCALE, case, *bars)
    rp.corrected_match(corrected, SCALE, case, corr64, 4e-6 + dev["corrected"])
    rp.gray_match(gray, SCALE, case, dev["gray"], ulps=1.0)
    _rejects(rp.coef_match, coef.flip(0), SCALE, case, *bars)                          # (a, b) swapped
    # the fit over the first two stats blocks only (2 x 4096 of the 8640 pixels)
    part = scale_fit_f64(gt_f.reshape(-1, 3)[:8192].reshape(64, 128, 3), pred.reshape(-1, 3)[:8192].reshape(64, 128, 3))
    _rejects(rp.coef_match, torch.tensor(part[:2], dtype=torch.float64), SCALE, case, *bars)
    x = np.log(pred[..., 0].astype(np.float64) + pred[..., 1] + 1e-6)
    _rejects(rp.corrected_match, torch.from_numpy(np.exp(part[0] * x + part[1])), SCALE, case, corr64, 4e-6 + dev["corrected"])
    _rejects(rp.corrected_match, torch.from_numpy(np.exp(a64 * np.log(pred[..., 0].astype(np.float64) + pred[..., 1]) + b64)), SCALE, case, corr64,
             4e-6 + dev["corrected"])                                                  # the EPS inside the logarithm left out
    bt601 = torch.from_numpy(gt_f) @ torch.tensor([0.299, 0.587, 0.114])               # the weights everyone else uses
    _rejects(rp.gray_match, bt601, SCALE, case, dev["gray"], ulps=1.0)
    shifted = gray.clone()
    shifted[40, 60] += 4 * float(np.spacing(np.float32(gray[40, 60])))
    _rejects(rp.gray_match, shifted, SCALE, case, dev["gray"], ulps=1.0)


def test_the_mapper_comparison_rejects_mutated_data():
    bars = {"loss": 1e-5, "dx": 1e-5, "dpow": 1e-4, "y": 1e-6}
    own = lambda name, tag: {"loss": MAPPERS[f"{name}.loss_{tag}"], "dx": rp.t(MAPPERS[f"{name}.dx_{tag}"]), "y": rp.t(MAPPERS[f"{name}.y"])[:258 if tag == "all" else 257],
                             "dpow": rp.t(MAPPERS[f"{name}.dpow_{tag}"]) if rp.mapper_pow(name) is not None else None}
    for name in rp.mapper_names():
        for tag in ("all", "pos"):
            rp.mapper_match(own(name, tag), MAPPERS, name, tag, bars)
    _rejects(rp.mapper_match, own("powpow_0.6", "pos"), MAPPERS, "powpow_1.0", "pos", bars)      # p = 0.6 data under p = 1.0
    _rejects(rp.mapper_match, own("gt", "pos"), MAPPERS, "powpow_0.6", "pos", bars)             # 1 / 2.4 = 0.4167 under p = 0.6
    wrong_n = own("powpow_1.7", "pos")
    wrong_n["loss"] = wrong_n["loss"] * (257.0 / 258.0)                                       # the mean over one ray too many
    _rejects(rp.mapper_match, wrong_n, MAPPERS, "powpow_1.7", "pos", bars)
    finite_at_zero = own("gt", "all")
    finite_at_zero["dx"][-1] = 0.0                                                             # the reference's expression is infinite there
    _rejects(rp.mapper_match, finite_at_zero, MAPPERS, "gt", "all", bars)
    # the clamped candidate (the kernels): a gradient on the clamped row, a wrong one elsewhere
    clamped = own("gt", "all")
    clamped["dx"][-1] = 0.0
    rp.mapper_match(clamped, MAPPERS, "gt", "all", bars, at_zero_row="clamped")
    _rejects(rp.mapper_match, own("gt", "all"), MAPPERS, "gt", "all", bars, at_zero_row="clamped")
    leak = own("identity", "all")                                                              # finite in the reference, zero behind the clamp
    _rejects(rp.mapper_match, leak, MAPPERS, "identity", "all", bars, at_zero_row="clamped")
    clamped["dx"][5] *= 1.0 + 1e-3
    _rejects(rp.mapper_match, clamped, MAPPERS, "gt", "all", bars, at_zero_row="clamped")
