"""A training run that is stopped, written to a checkpoint, loaded into freshly built objects and continued, held to the run that
never stopped (INTEGRATION.md "checkpoint": training "resumes with its Adam moments and learning-rate schedule position").

Much of a run's state lives on the device and outside ``state_dict()`` so that a replayed graph reads nothing the host writes: the
flat parameter buffer the parameters are views of, the Adam clock and schedule constants, ``occs.mean()`` at a fixed address, the
composer's draw position, the camera optimisers outside the model.  The harness is that of tests/test_gpu_analytic_scene.py
(``analytic_scene.CONFIG``: a 64^3 one-level grid, a 2^17 table, 1024 rays per step; ``DeviceScene.from_arrays``, ``BatchComposer``,
``FlatAdam(FlatParams(...))``, ``GraphedTrainStep(composer=, jitter="input")``, ``update_occupancy_grid`` in front of every step),
with a decaying learning rate so that the schedule position shows, and with the jitter of step k drawn from a CPU generator seeded
from (7, k): a function of the step number, not of what the process did before.

* The LIVE run trains steps 0 .. K+M-1 (K = 264, M = 32: across the end of the occupancy warm-up at 256 and the refreshes at 256, 272
  and 288), writes a checkpoint after step K-1 with the reference's convention ("step": K-1, R:lse_nerf/lse_trainer.py:98 resumes at
  step + 1), and keeps copies of its state at that moment and of what step K drew, marched and computed.
* The RESUMED run is built under another ``torch.manual_seed`` -- whatever is not restored is visibly different -- with its own
  ``FlatParams`` / ``FlatAdam`` / ``BatchComposer`` / ``GraphedTrainStep`` (captured from the loaded, non-zero state), and loads from
  the file alone.
* The TWIN is ``copy.deepcopy`` of the live model at K with cloned optimizer tensors and a graph of its own: no file, no
  checkpoint.py.  Two continuations of identical state differ by float-atomic noise; the twin measures how much.

(a) the state after the load and (c) the forward-only paths are held bit for bit, as is everything of the first resumed step that no
float atomic touches (b); losses, gradients and the parameter update of that step take the bars tests/test_gpu_graph.py uses for
"same parameters, other process".  (d) M further steps: resumed against live may differ by three times what twin against live
differs by (one sample of the noise) plus the float32 resolution of the quantity.  (e) every omission a loader could make is caught by
one of the EXACT checks, named.  (f) the same for BASELINE config 4: per-camera / spline pose parameters and their Adam, inside the
captured step.  The shared checks return the list of what they missed (``Figures`` of test_gpu_analytic_scene.py does the same), every
figure is printed (``RESUME ...`` lines) before anything is asserted, and profiles/resume_equivalence.txt holds one run's.

The parameter-update criterion (share of elements off by more than 1e-5 x max|parameters| below 0.02) is checked on the CPU for this
configuration by tools/resume_noise_share.py: ``oracle.model.ModelOracle`` trained to step 264, step 264 taken twice, once on a
gradient off by 3e-5 relative -- share 0.000000 (largest difference of an update 2.5e-7 against the element threshold 2.8e-5).  With
every touched element off by 3e-5 of its TENSOR's largest gradient (the worst nmax_err < 3e-5 admits) the share is 0.060: the
criterion is the tighter of the two readings and is kept.

The occupancy refresh of this configuration is the eager ``_update`` (generator seeded from (update_seed, step), EMA-max by an
integer atomicMax, one torch mean): no order-dependent sum, so it is held bit for bit like the cell draw of csrc/occ_refresh.hip.
"""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import analytic_scene as sc
from tests import test_gpu_analytic_scene as A
from tests.util import nmax_err

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error:The AccumulateGrad node's stream")]

CFG = sc.CONFIG
K, M = 264, 32
LIVE_SEED, RESUME_SEED = A.GPU_SEED, 9071
SCHEDULE = dict(lr=CFG["lr"], eps=CFG["eps"], lr_final=1e-3, max_steps=1000)       # lr(264) = 0.545 lr(0): the position shows
REFRESH_STEP = 272
F32 = float(np.finfo(np.float32).eps)
OMISSIONS = {           # what a loader leaves out -> the exact check that must name it
    "no_moments": "a: exp_avg",
    "no_step": "a: step_count",
    "no_composer_step": "b: drawn (c, y, x)",
    "no_grid": "a: occs",
    "stale_occ_mean": "a: _occ_mean_dev == occs.mean()",
    "no_flat_views": "a: parameters are views of flat.data",
}


_DIR = {}


@pytest.fixture(scope="module", autouse=True)
def _checkpoint_dir(tmp_path_factory):
    """Where the live run writes its one checkpoint; the cached runs (and their device memory) go when the module is done."""
    _DIR["path"] = str(tmp_path_factory.mktemp("resume"))
    yield
    for cached in (_live, _resumed, _twin, _scene, _jitter):
        cached.cache_clear()


# ---------------------------------------------------------------------------------------------------- the pieces of a run
@functools.lru_cache(maxsize=None)
def _jitter():
    """[K + M, rays] on the device: row k from a CPU generator seeded from (7, k)."""
    rows = [torch.rand(CFG["rays_per_step"], generator=torch.Generator().manual_seed((7 << 32) + k)) for k in range(K + M)]
    return torch.stack(rows).cuda()


@functools.lru_cache(maxsize=None)
def _scene():
    from lsenerf_amd.data import DeviceScene
    poses, truth = A._truth("train")
    return DeviceScene.from_arrays("cuda", col_images=truth["rgb8"], col_cameras=A._cameras(poses),
                                   col_appearance_ids=torch.zeros(len(poses), dtype=torch.int64))


def _model(seed):
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig
    from lsenerf_amd.field import LSEEmbeddingConfig
    torch.manual_seed(seed)
    cfg = LSENeRFModelConfig(grid_resolution=CFG["grid_resolution"], grid_levels=CFG["grid_levels"], log2_hashmap_size=CFG["log2_hashmap_size"],
                             alpha_thre=CFG["alpha_thre"], cone_angle=CFG["cone_angle"], near_plane=CFG["near_plane"],
                             render_step_size=CFG["render_step_size"], background_color=CFG["background"],
                             embed_config=LSEEmbeddingConfig(eval_mode="mean"), eval_num_rays_per_chunk=A.H * A.W,
                             eval_depth_quantiles=(0.5,), eval_normals="off")
    return LSENeRFModel(cfg, torch.tensor(A.BOUNDS), CFG["num_embeddings"]).cuda().train()


class Run:
    """A model with everything a training run builds around it."""

    def __init__(self, model):
        from lsenerf_amd.data import BatchComposer
        from lsenerf_amd.optim import FlatAdam, FlatParams
        self.model = model
        self.comp = BatchComposer(_scene(), CFG["rays_per_step"], 0, seed=CFG["draw_seed"])
        self.opt = FlatAdam(FlatParams(model.get_param_groups()["fields"]), **SCHEDULE)
        self.step = None

    def capture(self):
        from lsenerf_amd.graph import GraphedTrainStep
        self.step = GraphedTrainStep(self.model, self.opt, composer=self.comp, jitter="input")
        return self.step

    def train(self, k):
        """Step k of the run -> its rgb loss, on the device."""
        self.model.update_occupancy_grid(k)
        if self.step is None:
            self.capture()
        return self.step(jitter=_jitter()[k])["rgb_loss"].detach()

    def first_step_record(self):
        """What the step just replayed drew, marched and computed (copies: the next replay overwrites the originals)."""
        out = self.step.outputs["col_out"]
        return {"indices": self.comp.batch["col_batch"]["indices"].clone(), "image": self.comp.batch["col_batch"]["image"].clone(),
                "samples_per_ray": out["num_samples_per_ray"].clone(), "samples": int(out["num_samples_per_ray"].sum()),
                "hyper": self.opt._hyper_dev.clone(), "grad": self.opt.flat.grad.clone(), "loss": float(self.step.losses["rgb_loss"]),
                "composer_step": int(self.comp.step_dev)}

    def finish(self):
        self.step.check_overflow()
        self.step.close()


def _state(run):
    """Copies of every tensor a resumed run must find again."""
    est, opt = run.model.occupancy_grid, run.opt
    return {"flat.data": opt.flat.data.clone(), "exp_avg": opt.exp_avg.clone(), "exp_avg_sq": opt.exp_avg_sq.clone(),
            "step_count": opt.step_count, "current_lr": opt.current_lr(), "occs": est.occs.clone(), "binaries": est.binaries.clone(),
            "_occ_mean_dev": est.__dict__["_occ_mean_dev"].clone()}


def _forward_only(model):
    """The forward-only paths from the state ``model`` is in, on a deep copy (the refresh writes the grid): the eval render of
    held-out view 0, ``update_occupancy_grid(REFRESH_STEP)``, and the cell draw of csrc/occ_refresh.hip at that step."""
    from lsenerf_amd import evaluation
    from lsenerf_amd.occ_refresh import DeviceGridRefresher
    m = copy.deepcopy(model)
    m.deferred_counts, m.deferred_max_slots = True, 1 << 24       # (a model inside a captured step carries the step's settings)
    out = {}
    with torch.no_grad():
        m.eval()
        r = evaluation.render_flat(m, A._bundle("heldout", 0))
        out.update(rgb=r["rgb"].clone(), accumulation=r["accumulation"].clone(), depth=r["depth"].clone(),
                   median_depth=r["depth_quantiles"].clone())
        m.train()
        ref = DeviceGridRefresher(m.occupancy_grid, m.field, m.config.render_step_size)
        ref.step_dev.fill_(REFRESH_STEP)
        ref.list_occupied()
        ids, pos = ref.draw_level(0, False)
        n = int(ref.n_dev)
        out.update(drawn_n=n, drawn_cells=ids[:n].clone(), drawn_positions=pos[:n].clone())
        m.update_occupancy_grid(REFRESH_STEP)
        out.update(refreshed_occs=m.occupancy_grid.occs.clone(), refreshed_binaries=m.occupancy_grid.binaries.clone())
    return out


def _psnr_view0(model):
    from lsenerf_amd import evaluation
    model.eval()
    with torch.no_grad():
        rgb = evaluation.render_flat(model, A._bundle("heldout", 0))["rgb"].cpu().numpy().astype(np.float64)
    model.train()
    return sc.psnr(rgb, A._truth("heldout")[1]["rgb8"][0].reshape(-1, 3) / 255.0)


# ---------------------------------------------------------------------------------------------------- the live run, once
@functools.lru_cache(maxsize=None)
def _live():
    from lsenerf_amd.checkpoint import save_nerfstudio_checkpoint
    run = Run(_model(LIVE_SEED))
    curve = torch.zeros(K + M, device="cuda")
    res = {"dir": _DIR["path"]}
    for k in range(K + M):
        if k == K:
            before = run.opt.flat.data.clone()
        curve[k] = run.train(k)
        if k == K - 1:
            res["path"] = save_nerfstudio_checkpoint(res["dir"], run.model, step=K - 1, optimizers={"fields": run.opt})
            res["state"] = _state(run)
            res["forward"] = _forward_only(run.model)
            res["twin_model"] = copy.deepcopy(run.model)
            res["twin_model"].deferred_counts, res["twin_model"].deferred_max_slots = run.step._deferred_before
        if k == K:
            res["first"] = run.first_step_record()
            res["first"]["delta"] = run.opt.flat.data - before
    run.finish()
    assert int(run.comp.step_dev) == K + M and run.opt.step_count == K + M
    res["curve"] = curve.cpu().numpy().astype(np.float64)
    assert np.isfinite(res["curve"]).all()
    res["psnr"] = _psnr_view0(run.model)
    res["spans"] = [(o, o + p.numel()) for p, o in zip(run.opt.flat.params, run.opt.flat.offsets)]
    res["scale"] = float(res["state"]["flat.data"].abs().max())
    return res


# ---------------------------------------------------------------------------------------------------- the checks, as lists of misses
def _bits(name, a, b, missed):
    ok = a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    if not ok:
        missed.append(name)
    return ok


def check_state(run, live, tag="a"):
    """(a): the loaded state against the live run's at K, bit for bit -> names of what differs."""
    want, got, missed = live["state"], _state(run), []
    for k in ("flat.data", "exp_avg", "exp_avg_sq", "occs", "binaries"):
        _bits(f"{tag}: {k}", got[k], want[k], missed)
    for k in ("step_count", "current_lr"):
        if got[k] != want[k]:
            missed.append(f"{tag}: {k}")
    est = run.model.occupancy_grid
    if float(est.__dict__["_occ_mean_dev"]) != float(est.occs.mean()):                  # read as is: no recomputation here
        missed.append(f"{tag}: _occ_mean_dev == occs.mean()")
    _bits(f"{tag}: _occ_mean_dev == the live run's", got["_occ_mean_dev"], want["_occ_mean_dev"], missed)
    flat = run.opt.flat
    params = [p for p in run.model.get_param_groups()["fields"] if p.requires_grad]
    views = len(params) == len(flat.params)
    grads = views
    for p, fp, o in zip(params, flat.params, flat.offsets):
        views = views and p is fp and p.data_ptr() == flat.data.data_ptr() + 4 * o and p.is_contiguous()
        grads = grads and p.grad is not None and p.grad.data_ptr() == flat.grad.data_ptr() + 4 * o
    if not views:
        missed.append(f"{tag}: parameters are views of flat.data")
    if not grads:
        missed.append(f"{tag}: gradients are views of flat.grad")
    return missed


def check_forward(got, live):
    """(c): the forward-only paths from the loaded state against those from the live run's state at K, bit for bit."""
    missed = []
    for k, v in live["forward"].items():
        if torch.is_tensor(v):
            _bits(f"c: {k}", got[k], v, missed)
        elif got[k] != v:
            missed.append(f"c: {k}")
    return missed


def check_first_step(run, live, title):
    """(b): capture the step from the loaded state (which must leave the state alone), replay it once as step K, and hold it to
    the live run's step K -> names of what differs.  Prints the noisy figures."""
    missed = []
    run.capture()
    missed += check_state(run, live, tag="a, after the capture")
    before = run.opt.flat.data.clone()
    loss = float(run.train(K))
    got, want = run.first_step_record(), live["first"]
    drawn = run.comp.indices_host(K)[0]
    if not np.array_equal(got["indices"].cpu().numpy().astype(np.int64), drawn) or not torch.equal(got["indices"], want["indices"]):
        missed.append("b: drawn (c, y, x)")
    _bits("b: batch image", got["image"], want["image"], missed)
    _bits("b: packed_info (samples per ray)", got["samples_per_ray"], want["samples_per_ray"], missed)
    if got["samples"] != want["samples"]:
        missed.append("b: device sample count")
    _bits("b: _hyper_dev after the replay", got["hyper"], want["hyper"], missed)
    if got["composer_step"] != K + 1 or want["composer_step"] != K + 1:
        missed.append("b: composer.step_dev == K + 1")
    ok = abs(loss - want["loss"]) <= 2e-5 * max(1.0, abs(want["loss"]))
    print(f"RESUME {title} step {K}: rgb_loss {loss:.9g} against live {want['loss']:.9g}  {'ok' if ok else 'MISS'}")
    if not ok:
        missed.append("b: rgb_loss")
    worst = 0.0
    for a, b in live["spans"]:
        if float(want["grad"][a:b].abs().max()) == 0.0 and float(got["grad"][a:b].abs().max()) == 0.0:
            continue
        worst = max(worst, nmax_err(got["grad"][a:b], want["grad"][a:b], 1e-12))
    print(f"RESUME {title} step {K}: flat gradient, worst tensor nmax_err {worst:.3g} < 3e-5  {'ok' if worst < 3e-5 else 'MISS'}")
    if not worst < 3e-5:
        missed.append("b: flat gradient")
    d = ((run.opt.flat.data - before) - want["delta"]).abs()
    share = float((d > 1e-5 * live["scale"]).float().mean())
    print(f"RESUME {title} step {K}: share of the parameter update off by more than 1e-5 x {live['scale']:.4g}: {share:.6f} < 0.02, "
          f"largest {float(d.max()):.3g}  {'ok' if share < 0.02 else 'MISS'}")
    if not share < 0.02:
        missed.append("b: parameter update")
    return missed


# ---------------------------------------------------------------------------------------------------- resumed runs
def _load(omit=None):
    """A run built under another seed and loaded from the live run's file alone, with one thing left out when ``omit`` names it."""
    from lsenerf_amd.checkpoint import load_nerfstudio_checkpoint
    live = _live()
    run = Run(_model(RESUME_SEED))
    est = run.model.occupancy_grid
    if omit == "no_flat_views":          # a parameter re-created behind FlatParams' back: the load fills it, the flat buffer keeps its own
        head = run.model.field.mlp_head
        head.params = torch.nn.Parameter(head.params.detach().clone())
    fresh_mean = est._occ_mean_device().clone()      # the fresh grid's mean is on the device before the load: the load must replace it
    info = load_nerfstudio_checkpoint(live["path"], run.model, optimizers={"fields": run.opt})
    assert info["step"] == K - 1 and info["missing"] == [] and info["unexpected"] == [] and info["dropped"] == []
    if omit != "no_composer_step":
        run.comp.set_step(info["step"] + 1)
    with torch.no_grad():
        if omit == "no_moments":
            run.opt.exp_avg.zero_(), run.opt.exp_avg_sq.zero_()
        elif omit == "no_step":
            run.opt.step_count = 0
        elif omit == "no_grid":
            est.occs.zero_(), est.binaries.zero_()
            est._invalidate_occ_mean()
        elif omit == "stale_occ_mean":   # occs written behind the tensor's back, as a kernel writes it: nothing recomputes the mean
            est.__dict__["_occ_mean_dev"].copy_(fresh_mean)
            est.__dict__["_occ_mean_dev_version"] = est.occs._version
    return run


@functools.lru_cache(maxsize=None)
def _resumed():
    """The resumed run, once: the misses of (a), (c) and (b), then M - 1 further steps."""
    live = _live()
    run = _load()
    res = {"a": check_state(run, live), "c": check_forward(_forward_only(run.model), live)}
    res["b"] = check_first_step(run, live, "resumed")
    res["curve"], res["psnr"] = _continue(run)
    return res


def _continue(run):
    """Steps K + 1 .. K + M - 1 of a run that has taken step K -> (rgb losses of steps K + 1 .., held-out PSNR of view 0)."""
    curve = torch.zeros(M - 1, device="cuda")
    for k in range(K + 1, K + M):
        curve[k - K - 1] = run.train(k)
    run.finish()
    assert int(run.comp.step_dev) == K + M and run.opt.step_count == K + M
    curve = curve.cpu().numpy().astype(np.float64)
    assert np.isfinite(curve).all()
    return curve, _psnr_view0(run.model)


@functools.lru_cache(maxsize=None)
def _twin():
    """The live model at K, deep-copied in the process, with cloned optimizer tensors and its own graph: steps K .. K + M - 1."""
    live = _live()
    run = Run(live["twin_model"])
    with torch.no_grad():
        run.opt.exp_avg.copy_(live["state"]["exp_avg"])
        run.opt.exp_avg_sq.copy_(live["state"]["exp_avg_sq"])
    run.opt.step_count = live["state"]["step_count"]
    run.comp.set_step(K)
    res = {"a": check_state(run, live, tag="twin"), "b": check_first_step(run, live, "twin")}
    res["curve"], res["psnr"] = _continue(run)
    return res


# ---------------------------------------------------------------------------------------------------- (a) - (d)
def test_the_live_run_crosses_the_warmup_and_trains():
    live = _live()
    st = live["state"]
    print(f"RESUME live: rgb_loss step 0 {live['curve'][0]:.5g}, step {K} {live['curve'][K]:.5g}, last {live['curve'][-1]:.5g}; lr at {K} "
          f"{st['current_lr']:.6g}; occupied {float(st['binaries'].float().mean()):.4f}; occs.mean() {float(st['_occ_mean_dev']):.6g}; "
          f"samples of step {K}: {live['first']['samples']}; held-out PSNR of view 0 {live['psnr']:.4f}")
    assert st["step_count"] == K and abs(st["current_lr"] - SCHEDULE["lr"] * (SCHEDULE["lr_final"] / SCHEDULE["lr"]) ** (K / 1000)) < 1e-12
    assert live["curve"][-1] < 0.1 * live["curve"][0]
    assert 0.0 < float(st["binaries"].float().mean()) < 0.5            # past the warm-up: the grid has been carved
    assert float(st["exp_avg"].abs().max()) > 0 and live["first"]["samples"] > CFG["rays_per_step"]
    assert float(live["first"]["hyper"][0]) != float(np.float32(SCHEDULE["lr"]))     # the schedule has moved the device's lr


def test_the_loaded_state_equals_the_live_state_bit_for_bit():
    """(a), before and after the step is captured from the loaded state."""
    res = _resumed()
    missed = res["a"] + [m for m in res["b"] if m.startswith("a,")]
    print("RESUME (a) misses:", missed)
    assert not missed, missed


def test_the_first_resumed_step_is_the_live_runs_step_K():
    """(b): draw, batch, samples per ray, sample count, the device's Adam scalars and the composer position exactly; loss, gradient
    and parameter update at the bars of tests/test_gpu_graph.py."""
    missed = [m for m in _resumed()["b"] if m.startswith("b:")]
    print("RESUME (b) misses:", missed)
    assert not missed, missed


def test_the_forward_only_paths_are_bit_equal():
    """(c): eval render of held-out view 0 (rgb, accumulation, expected and median depth), the occupancy refresh of step 272 and the
    device's cell draw at that step, from the loaded state, before any resumed step."""
    missed = _resumed()["c"]
    print("RESUME (c) misses:", missed)
    assert not missed, missed


def test_the_twin_is_a_sound_noise_reference():
    """The deep copy starts from the live state bit for bit and its first step meets the bars of (b): what (d) measures between
    twin and live is the noise of two continuations of identical state and nothing else."""
    res = _twin()
    missed = res["a"] + res["b"]
    print("RESUME twin misses:", missed)
    assert not missed, missed


def test_further_steps_stay_within_the_noise_of_two_continuations():
    """(d).  No number is set in advance: the bar is three times the twin's figure plus the float32 resolution of the quantity."""
    live, res, twin = _live(), _resumed(), _twin()
    tail = live["curve"][-8:]
    fig = {}
    for name, other in (("resumed", res), ("twin", twin)):
        fig[name] = (float(np.abs(other["curve"][-8:] - tail).mean()), abs(other["psnr"] - live["psnr"]))
    bar_loss = 3.0 * fig["twin"][0] + F32 * float(np.abs(tail).mean())
    bar_psnr = 3.0 * fig["twin"][1] + F32 * abs(live["psnr"])
    print(f"RESUME (d) mean |d rgb_loss| over the last 8 steps: resumed - live {fig['resumed'][0]:.4g}, twin - live {fig['twin'][0]:.4g}, "
          f"bar {bar_loss:.4g}  (rgb_loss there {float(tail.mean()):.4g})")
    print(f"RESUME (d) held-out PSNR of view 0: live {live['psnr']:.5f}; |resumed - live| {fig['resumed'][1]:.4g}, |twin - live| "
          f"{fig['twin'][1]:.4g}, bar {bar_psnr:.4g}")
    assert fig["resumed"][0] <= bar_loss, (fig, bar_loss)
    assert fig["resumed"][1] <= bar_psnr, (fig, bar_psnr)


# ---------------------------------------------------------------------------------------------------- (e) omissions
@pytest.mark.parametrize("omit", list(OMISSIONS))
def test_an_omission_is_caught_by_an_exact_check(omit):
    """One resumed run per omission; the exact checks of (a) and (b) must name it (the noisy bar of (d) is never asked).  The first
    step runs where the omission shows there or nowhere in (a) (the composer position, the device clock, the moments); a run whose
    grid, alpha cap or parameter views are wrong is caught in (a) and is not trained on."""
    live = _live()
    run = _load(omit)
    missed = check_state(run, live)
    if omit in ("no_moments", "no_step", "no_composer_step"):
        missed += check_first_step(run, live, f"omission {omit}")
        run.finish()
    print(f"RESUME (e) {omit}: caught by {missed}")
    assert OMISSIONS[omit] in missed, (omit, missed)
    if omit == "no_moments":
        assert "b: parameter update" in missed, missed
    if omit == "no_step":
        assert "b: _hyper_dev after the replay" in missed, missed
    if omit == "no_composer_step":
        assert [m for m in missed if m.startswith("a")] == [], missed          # nothing of (a) can see the draw position


# ---------------------------------------------------------------------------------------------------- (f) config 4
def _camera_modules(comp, kind):
    """The modules a data manager keeps as col_ / evs_train_camera_optimizer: the shared spline under both names, as the reference
    stores it (R:lse_nerf/lse_datamanager.py:297)."""
    if kind == "spline":
        return {"col": comp.spline.spline, "evs": comp.spline.spline}
    if kind == "mixed":
        return {"col": comp.spline.spline, "evs": comp.deltas.optims[1]}
    return {"col": comp.deltas.optims[0], "evs": comp.deltas.optims[1]}


def _camera_jitter(n, k):
    return torch.rand(n, generator=torch.Generator().manual_seed((7 << 32) + k)).cuda()


@pytest.mark.parametrize("kind", ["deltas", "spline", "mixed"])
def test_camera_parameters_and_their_adam_resume(tmp_path, kind):
    """BASELINE config 4 on the smallest scene of tests/test_gpu_pose_delta.py: 12 steps, checkpoint, resume, 4 steps.  The pose
    parameters live outside the model and their Adam outside the "fields" group; ``lse_pose_delta_tables`` / ``lse_spline_poses``
    are forward-only, so the first resumed compose writes the live run's tables bit for bit."""
    from lsenerf_amd.checkpoint import load_nerfstudio_checkpoint, save_nerfstudio_checkpoint
    from lsenerf_amd.graph import GraphedTrainStep
    from tests.test_gpu_pose_delta import _setup_camera_adam
    S, EXTRA = 12, 4

    def build(sub):
        (tmp_path / sub).mkdir()
        comp, m, opt, cam_opt, _ = _setup_camera_adam(tmp_path / sub, kind)
        return comp, m, opt, cam_opt

    def cam_state(cam_opt):
        return [cam_opt.flat.data.clone(), cam_opt.exp_avg.clone(), cam_opt.exp_avg_sq.clone()]

    def first(comp, step, opt, cam_opt):
        before = (cam_opt.flat.data.clone(), opt.flat.data.clone())
        losses = {k: float(v) for k, v in step(jitter=_camera_jitter(comp.n_rays, S)).items()}
        return {"tables": [None if t is None else t.clone() for t in comp.pose_tables], "losses": losses,
                "indices": comp.batch["col_batch"]["indices"].clone(),
                "d_cam": cam_opt.flat.data - before[0], "d_field": opt.flat.data - before[1], "hyper": cam_opt._hyper_dev.clone()}

    # the live run
    comp, m, opt, cam_opt = build("live")
    step = GraphedTrainStep(m, opt, composer=comp, ray_grads=True, jitter="input", camera_opt=cam_opt)
    for k in range(S):
        step(jitter=_camera_jitter(comp.n_rays, k))
    mods = _camera_modules(comp, kind)
    path = save_nerfstudio_checkpoint(str(tmp_path / "ckpt"), m, step=S - 1, optimizers={"fields": opt, "camera_opt": cam_opt},
                                      camera_optimizers=mods)
    want_cam, want_field, want_lr = cam_state(cam_opt), opt.flat.data.clone(), cam_opt.current_lr()
    want_named = {w: {k: v.detach().clone() for k, v in mod.state_dict().items()} for w, mod in mods.items()}
    want = first(comp, step, opt, cam_opt)
    for k in range(S + 1, S + EXTRA):
        step(jitter=_camera_jitter(comp.n_rays, k))
    live_after = cam_opt.flat.data.clone()
    step.check_overflow()
    step.close()
    assert cam_opt.step_count == S + EXTRA and float((want_cam[0] - live_after).abs().max()) > 0

    # the resumed run: same construction, every trainable number moved, so that what the load leaves alone shows
    comp2, m2, opt2, cam_opt2 = build("resumed")
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for flat in (opt2.flat, cam_opt2.flat):
            flat.data.add_((torch.randn(flat.numel, generator=g) * 1e-2).cuda() * (flat.data != 0))
    mods2 = _camera_modules(comp2, kind)
    assert not torch.equal(cam_opt2.flat.data, want_cam[0])
    # (the omission this test exists for: a load that is not handed the modules leaves the poses where they were and says so)
    info = load_nerfstudio_checkpoint(path, m2, optimizers={"fields": opt2})
    assert len(info["dropped"]) == sum(len(w) for w in want_named.values()) and not torch.equal(cam_opt2.flat.data, want_cam[0])
    info = load_nerfstudio_checkpoint(path, m2, optimizers={"fields": opt2, "camera_opt": cam_opt2}, camera_optimizers=mods2)
    assert info["step"] == S - 1 and info["dropped"] == [] and info["unexpected"] == [] and info["missing"] == [], info
    comp2.set_step(info["step"] + 1)
    missed = []
    for w, mod in mods2.items():
        for k, v in mod.state_dict().items():
            _bits(f"f: {w}.{k}", v, want_named[w][k], missed)
    for name, a, b in zip(("camera flat.data", "camera exp_avg", "camera exp_avg_sq"), cam_state(cam_opt2), want_cam):
        _bits(f"f: {name}", a, b, missed)
    _bits("f: field flat.data", opt2.flat.data, want_field, missed)
    if (cam_opt2.step_count, opt2.step_count) != (S, S) or cam_opt2.current_lr() != want_lr:
        missed.append("f: step counts")
    for flat in (cam_opt2.flat, opt2.flat):                        # the load went through the views
        if not all(p.data_ptr() == flat.data.data_ptr() + 4 * o for p, o in zip(flat.params, flat.offsets)):
            missed.append("f: parameters are views of flat.data")
    step2 = GraphedTrainStep(m2, opt2, composer=comp2, ray_grads=True, jitter="input", camera_opt=cam_opt2)
    for name, a, b in zip(("camera flat.data", "camera exp_avg", "camera exp_avg_sq"), cam_state(cam_opt2), want_cam):
        _bits(f"f, after the capture: {name}", a, b, missed)
    got = first(comp2, step2, opt2, cam_opt2)
    for i, (a, b) in enumerate(zip(got["tables"], want["tables"])):
        if a is not None:
            _bits(f"f: pose table {i} of the first resumed compose", a, b, missed)
    _bits("f: drawn (c, y, x)", got["indices"], want["indices"], missed)
    _bits("f: camera _hyper_dev after the replay", got["hyper"], want["hyper"], missed)
    for k in want["losses"]:
        if not abs(got["losses"][k] - want["losses"][k]) <= 2e-5 * max(1.0, abs(want["losses"][k])):
            missed.append(f"f: {k}")
    shares = {}
    for name, scale_of in (("d_cam", want_cam[0]), ("d_field", want_field)):
        scale = float(scale_of.abs().max())
        d = (got[name] - want[name]).abs()
        shares[name] = float((d > 1e-5 * scale).float().mean())
        print(f"RESUME (f) {kind} step {S}: share of {name} off by more than 1e-5 x {scale:.4g}: {shares[name]:.6f} < 0.02, largest "
              f"{float(d.max()):.3g}, largest update {float(want[name].abs().max()):.3g}")
        if not shares[name] < 0.02:
            missed.append(f"f: {name}")
    assert float(want["d_cam"].abs().max()) > 0
    for k in range(S + 1, S + EXTRA):
        step2(jitter=_camera_jitter(comp2.n_rays, k))
    step2.check_overflow()
    step2.close()
    d = (cam_opt2.flat.data - live_after).abs()
    print(f"RESUME (f) {kind} after {EXTRA} resumed steps: camera parameters off by at most {float(d.max()):.3g} "
          f"(they moved by {float((live_after - want_cam[0]).abs().max()):.3g} in those steps; recorded, no bar)")
    assert int(comp2.step_dev) == S + EXTRA and cam_opt2.step_count == opt2.step_count == S + EXTRA
    assert bool(torch.isfinite(cam_opt2.flat.data).all()) and bool(torch.isfinite(opt2.flat.data).all())
    print(f"RESUME (f) {kind} misses:", missed)
    assert not missed, missed


def test_camera_entries_without_a_module_are_reported_not_loaded(tmp_path):
    """A config-4 file loaded without ``camera_optimizers=``: every datamanager entry is named in "dropped" and the camera Adam is
    restored only when asked for; ``drop_camera_optimizer`` drops both, as the reference's eval mode does."""
    from lsenerf_amd.checkpoint import load_nerfstudio_checkpoint, save_nerfstudio_checkpoint
    from tests.test_gpu_pose_delta import _setup_camera_adam
    comp, m, opt, cam_opt, _ = _setup_camera_adam(tmp_path, "deltas")
    mods = _camera_modules(comp, "deltas")
    with torch.no_grad():
        cam_opt.exp_avg.add_(1.0)
    cam_opt.step_count = 3
    path = save_nerfstudio_checkpoint(str(tmp_path / "ckpt"), m, step=2, optimizers={"camera_opt": cam_opt}, camera_optimizers=mods)
    keep = cam_opt.flat.data.clone()
    with torch.no_grad():
        for p in cam_opt.flat.params:                              # (through the views: the padding between them stays zero)
            p.add_(0.5)
        cam_opt.exp_avg.zero_()
    cam_opt.step_count = 0
    moved = cam_opt.flat.data.clone()
    info = load_nerfstudio_checkpoint(path, m)
    assert sorted(info["dropped"]) == ["datamanager.col_train_camera_optimizer.pose_adjustment",
                                       "datamanager.evs_train_camera_optimizer.pose_adjustment"]
    assert torch.equal(cam_opt.flat.data, moved)
    info = load_nerfstudio_checkpoint(path, m, drop_camera_optimizer=True, optimizers={"camera_opt": cam_opt}, camera_optimizers=mods)
    assert len(info["dropped"]) == 2 and torch.equal(cam_opt.flat.data, moved) and cam_opt.step_count == 0
    info = load_nerfstudio_checkpoint(path, m, optimizers={"camera_opt": cam_opt}, camera_optimizers=mods)
    assert info["dropped"] == [] and torch.equal(cam_opt.flat.data, keep) and cam_opt.step_count == 3
    assert float(cam_opt.exp_avg[:6].min()) == 1.0
    assert all(p.data_ptr() == cam_opt.flat.data.data_ptr() + 4 * o for p, o in zip(cam_opt.flat.params, cam_opt.flat.offsets))
