"""Shared by tests/test_reference_pins_cpu.py and tests/test_gpu_reference_pins.py: the loader of the four ``tests/golden/ref_pin_*.npz``
files (outputs of the reference's own code, recorded by tests/golden/make_reference_pins.py) and the comparisons both tiers hold
their candidates to.  Not a test file; it never sees a kernel and reads nothing but tests/golden/.

Every comparison takes the candidate first and the recorded data second, asserts, and returns the figure it measured.  A bar of
exactly 0 asks for equal bits."""
from __future__ import annotations

import functools
import json
import os
from typing import Dict

import numpy as np
import torch

from tests.util import nmax_err

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = ("ref_pin_spline.npz", "ref_pin_pose_delta.npz", "ref_pin_scale_fit.npz", "ref_pin_mappers.npz")
MAX_BYTES = 100 * 1000
PRED_LEVELS = 32


@functools.lru_cache(maxsize=None)
def load(name: str) -> Dict[str, np.ndarray]:
    """One pin file as {key: array}: read once per process, shared, never modified (``t`` hands out copies)."""
    with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as z:
        out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def recorded_with(pin) -> dict:
    """What the file was recorded with: torch's version, the CPU capability it computed with, the reference files' sha256."""
    return {"torch_version": str(pin["torch_version"]), "cpu_capability": str(pin["cpu_capability"]), "sha256": json.loads(str(pin["sha256"]))}


def t(a) -> torch.Tensor:
    """A recorded array as a fresh (writable) tensor."""
    return torch.from_numpy(np.array(a, copy=True))


def _cpu(x) -> torch.Tensor:
    return x.detach().cpu() if torch.is_tensor(x) else torch.from_numpy(np.array(x, copy=True))


# ---------------------------------------------------------------------------------------------------- the two metrics
def max_abs_within(got, want, bar: float, what: str = "") -> float:
    """max |got - want| <= bar over same-shaped finite arrays; ``bar == 0``: the same bits."""
    got, want = _cpu(got), _cpu(want)
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    assert bool(torch.isfinite(got).all()), f"{what}: a non-finite entry"
    if bar == 0:
        assert got.dtype == want.dtype and torch.equal(got, want), f"{what}: not bit-equal, max abs {float((got.double() - want.double()).abs().max()):.3e}"
        return 0.0
    err = float((got.double() - want.double()).abs().max())
    assert err <= bar, f"{what}: max abs {err:.3e} > {bar:.3e}"
    return err


def nmax_within(got, want, bar: float, what: str = "", floor: float = 1e-6) -> float:
    """tests.util.nmax_err(got, want) <= bar over same-shaped finite arrays; ``bar == 0``: the same bits."""
    got, want = _cpu(got), _cpu(want)
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    assert bool(torch.isfinite(got).all()), f"{what}: a non-finite entry"
    if bar == 0:
        assert got.dtype == want.dtype and torch.equal(got, want), f"{what}: not bit-equal, nmax {nmax_err(got, want, floor):.3e}"
        return 0.0
    err = nmax_err(got, want, floor)
    assert err <= bar, f"{what}: nmax_err {err:.3e} > {bar:.3e}"
    return err


# ---------------------------------------------------------------------------------------------------- spline
def spline_fixtures():
    return json.loads(str(load(FILES[0])["fixtures"]))


def spline_tables_match(got, pin, fx: str, bar: float) -> float:
    return max_abs_within(got, pin[f"{fx}.tables"], bar, f"{fx} tables")


def zero_rotation_points(pin, fx: str) -> torch.Tensor:
    return t(pin[f"{fx}.ctrl"])[:, 3:].abs().amax(1) == 0


def spline_grad_match(got, pin, fx: str, bar: float) -> float:
    """d ctrl_tangents within ``bar`` (nmax_err); a control point whose rotation vector is exactly zero has an exactly zero rotation
    gradient in the candidate, as it has in the recorded one."""
    want = t(pin[f"{fx}.d_ctrl"])
    err = nmax_within(got, want, bar, f"{fx} d ctrl_tangents")
    zero = zero_rotation_points(pin, fx)
    if bool(zero.any()):
        assert float(want[zero, 3:].abs().max()) == 0.0
        assert float(_cpu(got)[zero, 3:].abs().max()) == 0.0, f"{fx}: a rotation gradient on a zero-rotation control point"
        assert float(_cpu(got)[zero, :3].abs().max()) > 0.0
    return err


def spline_grad_bar(pin, fx: str) -> float:
    """max(5 b, 1e-6), b = the reference's float32 autograd against float64: the kernels are held to max(4 b', 1e-6) of float64
    (tests/test_gpu_spline_dev.py, b' the same figure for cameras.py) and the reference is b from float64."""
    return max(5.0 * float(pin[f"{fx}.dev_d_ctrl"]), 1e-6)


# ---------------------------------------------------------------------------------------------------- pose delta
def pose_tables_match(got, pin, bar: float) -> float:
    return max_abs_within(got, pin["tables"], bar, "pose delta tables")


def pose_grad_match(got, pin, bar: float) -> float:
    return nmax_within(got, pin["d_adj"], bar, "d pose_adjustment")


# ---------------------------------------------------------------------------------------------------- scale fit
def scale_cases(ill=None):
    cases = json.loads(str(load(FILES[2])["cases"]))
    return [c for c in cases if ill is None or c["ill_conditioned"] == ill]


def scale_inputs(pin, case: dict):
    """``(gt as stored (uint8 or float32) [H, W, 3], gt as float32, prediction float32 [H, W, 3])`` of one case."""
    gt = np.array(pin[case["gt"]], copy=True)
    gt_f = gt if gt.dtype == np.float32 else (torch.from_numpy(gt).float() / 255.0).numpy()       # a true float32 division
    p = pin[case["pred"]]
    if p.dtype == np.uint8:                                   # numerators over 32: exact in float32; blue is never read
        pred = np.zeros(p.shape[:2] + (3,), dtype=np.float32)
        pred[..., :2] = p.astype(np.float32) / np.float32(PRED_LEVELS)
    else:
        pred = np.array(p, copy=True)
    return gt, gt_f, pred


def gray_match(got, pin, case: dict, extra: float, ulps: float = 0.0) -> float:
    """|got - recorded| <= extra + ulps * (spacing of float32 at the recorded value), entry by entry."""
    want = np.asarray(pin[f"{case['name']}.gray"], dtype=np.float32)
    got = _cpu(got).numpy().reshape(want.shape)
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    allowed = extra + ulps * np.spacing(np.abs(want)).astype(np.float64)
    assert bool((err <= allowed).all()), f"{case['name']} gray: {float(err.max()):.3e} > {float(allowed.min()):.3e}"
    return float(err.max())


def coef_match(got, pin, case: dict, bar_a: float, bar_b: float):
    want = pin[f"{case['name']}.coef"]
    got = _cpu(got).double().numpy().reshape(-1)
    assert got.shape == (2,) and np.isfinite(got).all()
    ea, eb = abs(got[0] - float(want[0])), abs(got[1] - float(want[1]))
    assert (ea <= bar_a and eb <= bar_b) if (bar_a or bar_b) else (ea == 0 and eb == 0), \
        f"{case['name']} (a, b): off by ({ea:.3e}, {eb:.3e}), bars ({bar_a:.3e}, {bar_b:.3e})"
    return float(ea), float(eb)


def corrected_match(got, pin, case: dict, scale64, bar: float) -> float:
    """max |got - recorded| / (the float64 fit's value) <= bar."""
    want = np.asarray(pin[f"{case['name']}.corrected"], dtype=np.float64)
    got = _cpu(got).double().numpy().reshape(want.shape)
    assert np.isfinite(got).all()
    err = float((np.abs(got - want) / np.asarray(scale64, dtype=np.float64).reshape(want.shape)).max())
    assert err <= bar if bar else err == 0, f"{case['name']} corrected: {err:.3e} > {bar:.3e}"
    return err


# ---------------------------------------------------------------------------------------------------- mappers
def mapper_names():
    return json.loads(str(load(FILES[3])["names"]))


def mapper_pow(name: str):
    return float(name.split("_")[1]) if name.startswith("powpow") else None


def mapper_match(got: dict, pin, name: str, tag: str, bars: dict, at_zero_row: str = "same") -> Dict[str, float]:
    """``got`` = {"loss", "dx", "dpow" (powpow only), optionally "y"} of mapper ``name`` over the rows of ``tag`` ("all": 258 rows,
    the last one (0, 0, 0); "pos": the first 257) against the recorded values; ``bars`` = {"loss": relative, "dx": nmax_err, "dpow":
    nmax_err, "y": max abs}, 0 = equal bits.  The recorded d x is compared where it is finite.  ``at_zero_row``: "same" -- the
    candidate is the reference's expression and is non-finite exactly where the recorded gradient is, with the same values;
    "clamped" -- the candidate clamps its input at 1e-5 as lsenerf.py does in front of the mapper (csrc/epilogue.hip;
    tests/epilogue_cases.py holds its gradient to float64 there): the row (0, 0, 0) gets a finite, exactly zero gradient, and only
    d x of the other rows is compared."""
    res = {}
    want_dx = t(pin[f"{name}.dx_{tag}"])
    got_dx = _cpu(got["dx"])
    assert tuple(got_dx.shape) == tuple(want_dx.shape)
    finite = torch.isfinite(want_dx)
    if at_zero_row == "clamped":
        assert tag == "all"
        assert bool(torch.isfinite(got_dx).all()) and float(got_dx[-1].abs().max()) == 0.0, f"{name}: the clamped row has a gradient"
        assert bool(finite[:-1].all())
        res["dx"] = nmax_within(got_dx[:-1], want_dx[:-1], bars["dx"], f"{name} d x ({tag})")
        return res
    assert torch.equal(torch.isfinite(got_dx), finite), f"{name}: non-finite entries of d x differ from the recorded ones"
    assert torch.equal(got_dx[~finite], want_dx[~finite])
    res["dx"] = nmax_within(got_dx[finite], want_dx[finite], bars["dx"], f"{name} d x ({tag})")
    loss, want = float(got["loss"]), float(pin[f"{name}.loss_{tag}"])
    res["loss"] = abs(loss - want) / abs(want)
    assert np.isfinite(loss) and (res["loss"] <= bars["loss"] if bars["loss"] else np.float32(loss) == np.float32(want)), \
        f"{name} loss ({tag}): {loss!r} against {want!r}, relative {res['loss']:.3e} > {bars['loss']:.3e}"
    if mapper_pow(name) is not None:
        res["dpow"] = nmax_within(_cpu(got["dpow"]).reshape(-1), t(pin[f"{name}.dpow_{tag}"]).reshape(-1), bars["dpow"], f"{name} d pow_coeff ({tag})")
    if "y" in got and got["y"] is not None:
        rows = want_dx.shape[0]
        res["y"] = max_abs_within(got["y"], pin[f"{name}.y"][:rows], bars["y"], f"{name} m(x)")
    return res
