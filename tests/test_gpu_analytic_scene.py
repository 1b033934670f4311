"""A field trained on the analytic scene of tests/analytic_scene.py, held to the scene's closed form: renders, depth, occupancy,
normals, the three exporters, event frames, the reduced-precision eval arithmetic and the distortion term.

Every other GPU test holds a kernel to a restatement of itself.  Here the ground truth is a dozen lines of ray-sphere and ray-box
algebra (checked by brute force in tests/test_analytic_scene_cpu.py), and a field that reproduces it has passed through every kernel
of the captured training step and of the eval render with the conventions right: axis order, signs, ray distance against z-depth,
triangle winding, the direction of a normal, the polarity of an event.

The model trains the way a user trains -- ``DeviceScene.from_arrays``, ``BatchComposer``, ``FlatAdam``, ``GraphedTrainStep(composer=)``,
the occupancy refresh of ``update_occupancy_grid`` -- with ``analytic_scene.CONFIG``, the configuration
tests/golden/make_analytic_scene.py trained ``oracle.model.ModelOracle`` with, on the same pixels in the same order
(``draw_indices_host``), from the same initial parameters; the two differ in the jitter stream, the occupancy refresh's draws and
the order of floating-point sums.  No bar is a number chosen here: each metric is held to the same metric of the oracle in
tests/golden/analytic_scene_oracle.json, per held-out view and per configuration -- no worse than the oracle's worst seed by more
than twice the oracle's spread over its three seeds (max - min).  PSNR, coverage, outward share and sign agreement are floors;
errors and the occupied fraction are caps.  Every test prints its figures (``ANALYTIC ...`` lines) before it asserts;
profiles/analytic_scene.txt holds one run's.

What the runs on an MI355X found (profiles/analytic_scene.txt has every figure):

* No convention is wrong.  Renders, both depths (ray distance, not z-depth: twice the error against z), occupancy, rendered and
  vertex normals, triangle winding, signed volume, exported positions and colours and the event polarity all land where the oracle's
  do, and every figure is inside its bar.
* The initialisation decides most of what two trainings differ by.  The HIP model therefore starts from the numbers the oracle's
  first seed started from (``make_analytic_scene.hip_initialisation``: the generator builds ``LSENeRFModel`` on the CPU under
  ``torch.manual_seed(seed)`` and hands its parameters to the oracle; the JSON carries a checksum that ``_trained`` checks).  Started
  alike, the two land within a fraction of the oracle's spread of each other (view 0 with contraction: PSNR 27.26 against the
  oracle's 27.11 for that seed, expected-depth rms 0.0428 against 0.0417).  With an initialisation of its own (the model's seed 96)
  the HIP model missed a dozen bars by 5 - 20 % and three seeds of it differed by more than the oracle's three: the rule's bars are
  tight for an unrelated fourth sample, not for the same start.
* The oracle does not reach the 0.95 the issue wanted of "normals within 90 degrees" and of the outward share: 0.62 - 0.86 of the
  rendered normals, 0.56 - 0.62 of the mesh's vertex normals and 0.70 - 0.78 of its triangles face outwards, after 400 steps as after
  800 (measured; more steps change none of them).  The gradient of a hash-grid density logit is mostly noise at this stage, and a
  density field is unconstrained inside a body, where the isosurface has sheets that face anywhere.  The tests hold the HIP model
  to the oracle's worst seed minus its spread all the same (a flipped sign gives 1 - x, far below), and add the shares over the part
  of the mesh within one lattice cell of the true surface, where 0.92 - 0.94 of the oracle's triangles face outwards.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import analytic_scene as sc
from tests import mesh_ref as mr

pytestmark = pytest.mark.gpu

CFG = sc.CONFIG
H, W = sc.H, sc.W
BOUNDS = [[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]
GPU_SEED = CFG["init_seeds"][0]   # the HIP model starts from the numbers the oracle's first seed started from
T_SCALE = 1.0 / 2.4           # distortion term: the ray length through the scene is about 2.4

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "analytic_scene_oracle.json")) as _f:
    ORACLE = json.load(_f)


# ---------------------------------------------------------------------------------------------------- the bars
def _values(config, key, view=None):
    runs = ORACLE["runs"][config]
    return [float(r[key] if view is None else r["views"][view][key]) for r in runs.values()]


def _spread(config, key, view=None):
    """max - min over the oracle's seeds; a configuration recorded for one seed takes the spread measured with contraction on."""
    if len(ORACLE["runs"][config]) < 2:
        config = "contraction_on"
    v = _values(config, key, view)
    return max(v) - min(v)


def cap(config, key, view=None, factor=2.0):
    return max(_values(config, key, view)) + factor * _spread(config, key, view)


def floor(config, key, view=None, factor=2.0):
    return min(_values(config, key, view)) - factor * _spread(config, key, view)


class Figures:
    """Collects ``(name, value, bar, ok)``, prints every figure, and asserts at the end so that a miss does not hide the rest."""

    def __init__(self, title):
        self.title, self.missed = title, []

    def _note(self, name, got, bar, ok, sign, oracle):
        print(f"ANALYTIC {self.title} {name}: gpu {got:.5g} {sign} bar {bar:.5g}  oracle {['%.5g' % v for v in oracle]}  {'ok' if ok else 'MISS'}")
        if not ok:
            self.missed.append((name, got, bar))

    def at_most(self, name, got, config, key, view=None, factor=2.0):
        bar = cap(config, key, view, factor)
        self._note(name, got, bar, got <= bar, "<=", _values(config, key, view))

    def at_least(self, name, got, config, key, view=None, factor=2.0):
        bar = floor(config, key, view, factor)
        self._note(name, got, bar, got >= bar, ">=", _values(config, key, view))

    def inside(self, name, got, config, key, view=None):
        lo, hi = floor(config, key, view), cap(config, key, view)
        ok = lo <= got <= hi
        print(f"ANALYTIC {self.title} {name}: gpu {got:.5g} in [{lo:.5g}, {hi:.5g}]  oracle {['%.5g' % v for v in _values(config, key, view)]}  "
              f"{'ok' if ok else 'MISS'}")
        if not ok:
            self.missed.append((name, got, (lo, hi)))

    def record(self, name, got):
        print(f"ANALYTIC {self.title} {name}: gpu {got:.5g} (recorded, no bar)")

    def done(self):
        assert not self.missed, self.missed


def _config_name(contraction):
    return "contraction_on" if contraction else "contraction_off"


# ---------------------------------------------------------------------------------------------------- the scene on the device
def _cameras(poses):
    from lsenerf_amd.cameras import EdCameras
    return EdCameras(torch.from_numpy(np.asarray(poses, np.float32)), fx=sc.FX, fy=sc.FY, cx=sc.CX, cy=sc.CY, width=W, height=H,
                     times=torch.zeros(len(poses)))


@functools.lru_cache(maxsize=None)
def _truth(which):
    poses = {"train": sc.train_cameras, "heldout": sc.heldout_cameras, "trajectory": sc.trajectory_cameras}[which]()
    return poses, sc.images(poses)


@functools.lru_cache(maxsize=None)
def _eval_set(which):
    from lsenerf_amd import EvalSet
    poses, truth = _truth(which)
    return EvalSet("cuda", truth["rgb8"], _cameras(poses))


# ---------------------------------------------------------------------------------------------------- training, once per configuration
@functools.lru_cache(maxsize=None)
def _trained(contraction=True, distortion_mult=0.0, draw_seed=CFG["draw_seed"]):
    """(model in eval mode, rgb_loss per step [steps] on the host).  Read-only for the tests."""
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig
    from lsenerf_amd.data import BatchComposer, DeviceScene
    from lsenerf_amd.field import LSEEmbeddingConfig
    from lsenerf_amd.graph import GraphedTrainStep
    from lsenerf_amd.optim import FlatAdam, FlatParams
    torch.manual_seed(GPU_SEED)
    cfg = LSENeRFModelConfig(grid_resolution=CFG["grid_resolution"], grid_levels=CFG["grid_levels"], log2_hashmap_size=CFG["log2_hashmap_size"],
                             alpha_thre=CFG["alpha_thre"], cone_angle=CFG["cone_angle"], near_plane=CFG["near_plane"],
                             render_step_size=CFG["render_step_size"], background_color=CFG["background"],
                             disable_scene_contraction=not contraction, embed_config=LSEEmbeddingConfig(eval_mode="mean"),
                             eval_num_rays_per_chunk=H * W, eval_depth_quantiles=(0.5,), eval_normals="world",
                             distortion_loss_mult=distortion_mult, distortion_t_scale=T_SCALE if distortion_mult > 0 else 1.0)
    model = LSENeRFModel(cfg, torch.tensor(BOUNDS), CFG["num_embeddings"])
    # the oracle of this seed started from these very numbers (make_analytic_scene.hip_initialisation): the two sides are made equal
    # where they can be, so what is left between them is the jitter stream, the refresh's draws and the order of the sums
    fld = model.field
    start = {"grid": fld.mlp_base_grid.params, "base": fld.mlp_base_mlp.params, "head": fld.mlp_head.params,
             "embedding": fld.embedding_appearance.embedding.weight}
    want = ORACLE["runs"][_config_name(contraction)][str(GPU_SEED)]["init_checksum"]
    for k, v in start.items():
        assert abs(float(v.detach().double().sum()) - want[k]) <= 1e-4 * abs(want[k]) + 1e-6, (k, float(v.detach().double().sum()), want[k])
    model = model.cuda().train()
    poses, truth = _truth("train")
    scene = DeviceScene.from_arrays("cuda", col_images=truth["rgb8"], col_cameras=_cameras(poses),
                                    col_appearance_ids=torch.zeros(len(poses), dtype=torch.int64))        # one appearance id
    comp = BatchComposer(scene, CFG["rays_per_step"], 0, seed=draw_seed)
    opt = FlatAdam(FlatParams(model.get_param_groups()["fields"]), lr=CFG["lr"], eps=CFG["eps"])
    assert CFG["occ_every"] == 16 and CFG["occ_warmup_steps"] == 256            # what update_occupancy_grid does
    step, curve = None, torch.zeros(CFG["steps"], device="cuda")
    for k in range(CFG["steps"]):
        model.update_occupancy_grid(k)
        if step is None:
            step = GraphedTrainStep(model, opt, composer=comp)
        curve[k] = step()["rgb_loss"].detach()
    step.check_overflow()
    model.occupancy_grid.check_deferred_overflow()
    assert int(comp.step_dev) == CFG["steps"]
    assert bool(torch.isfinite(opt.flat.data).all())
    step.close()
    curve = curve.cpu().numpy().astype(np.float64)
    assert np.isfinite(curve).all()
    return model.eval(), curve


def _bundle(which, i):
    from lsenerf_amd import evaluation
    from lsenerf_amd.eval_set import camera_bundle
    return evaluation._flatten_bundle(camera_bundle(_eval_set(which), i), device="cuda")


@functools.lru_cache(maxsize=None)
def _renders(key, which="heldout", arith="bf16x6", normals="world"):
    """Eval renders of the views of ``which`` through ``EvalSet`` and ``evaluation.render_flat`` -> numpy arrays [V, H W, ...].
    ``key``: the arguments of ``_trained``.  The two eval settings are put back."""
    from lsenerf_amd import evaluation
    model, _ = _trained(*key)
    saved = (model.config.eval_mlp_arith, model.field.inference_arith, model.config.eval_normals)
    outs = []
    try:
        model.config.eval_mlp_arith = model.field.inference_arith = arith
        model.config.eval_normals = normals
        with torch.no_grad():
            for i in range(len(_truth(which)[0])):
                outs.append({k: v.detach().cpu().numpy().astype(np.float64) for k, v in evaluation.render_flat(model, _bundle(which, i)).items()})
    finally:
        model.config.eval_mlp_arith, model.field.inference_arith, model.config.eval_normals = saved
    return {"rgb": np.stack([o["rgb"] for o in outs]), "acc": np.stack([o["accumulation"][:, 0] for o in outs]),
            "depth": np.stack([o["depth"][:, 0] for o in outs]), "median": np.stack([o["depth_quantiles"][:, 0] for o in outs]),
            "normals": np.stack([o["normals"] for o in outs])}


def _masks(which, v):
    truth = _truth(which)[1]
    hit = truth["hit"][v].ravel()
    inner = sc.interior(truth["body"][v]).ravel()
    return inner, inner & hit, inner & ~hit


def _render_figures(fig, key, config, arith="bf16x6", bars=True):
    """The render and depth figures of one training against the oracle's, per held-out view."""
    r = _renders(key, "heldout", arith)
    truth = _truth("heldout")[1]
    for v in range(CFG["n_heldout"]):
        inner, ih, im = _masks("heldout", v)
        gt = truth["rgb8"][v].reshape(-1, 3) / 255.0
        t = truth["t"][v].ravel()
        figures = [("psnr", sc.psnr(r["rgb"][v], gt), fig.at_least), ("psnr_interior", sc.psnr(r["rgb"][v], gt, inner), fig.at_least),
                   ("acc_hit_gt_0p9", float((r["acc"][v][ih] > 0.9).mean()), fig.at_least),
                   ("acc_miss_lt_0p1", float((r["acc"][v][im] < 0.1).mean()), fig.at_least)]
        for name, depth in (("depth", r["depth"][v]), ("median_depth", r["median"][v])):
            figures += [(f"{name}_{k}", x, fig.at_most) for k, x in sc.err_stats(depth[ih] - t[ih]).items()]
        for name, got, check in figures:
            if bars:
                check(f"view {v} {name}", got, config, name, v)
            else:
                fig.record(f"view {v} {name}", got)
        separated = float(np.concatenate([r["acc"][v][ih] > 0.5, r["acc"][v][im] < 0.5]).mean())
        print(f"ANALYTIC {fig.title} view {v} separated: gpu {separated:.5g} == 1 (every oracle seed: 1)")
        if separated != 1.0:
            fig.missed.append((f"view {v} separated", separated, 1.0))


# ---------------------------------------------------------------------------------------------------- 0. the trainings themselves
@pytest.mark.parametrize("contraction", [True, False])
def test_training_converges_like_the_oracles(contraction):
    model, curve = _trained(contraction)
    config = _config_name(contraction)
    fig = Figures(f"training[{config}]")
    fig.record("first rgb_loss", curve[0])
    fig.record("last rgb_loss", curve[-1])
    fig.at_most("last / first rgb_loss", curve[-1] / curve[0], config, "loss_ratio")
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert not model.training
    fig.done()


# ---------------------------------------------------------------------------------------------------- 1. renders
@pytest.mark.parametrize("contraction", [True, False])
def test_heldout_renders_reach_the_oracles(contraction):
    fig = Figures(f"renders[{_config_name(contraction)}]")
    _render_figures(fig, (contraction,), _config_name(contraction))
    fig.done()


# ---------------------------------------------------------------------------------------------------- 2. depth is ray distance
@pytest.mark.parametrize("contraction", [True, False])
def test_depth_is_the_distance_along_the_ray_not_the_z_depth(contraction):
    """The depth bars themselves are in test 1.  Here the convention is named: against the z-depth t cos(angle to the optical axis)
    the error of both depths is the larger one in every view, so a silent switch of the convention cannot hide in a bar."""
    r = _renders((contraction,))
    poses, truth = _truth("heldout")
    fig = Figures(f"depth convention[{_config_name(contraction)}]")
    for v in range(CFG["n_heldout"]):
        _, ih, _ = _masks("heldout", v)
        _, d = sc.pixel_rays(poses[v])
        t = truth["t"][v].ravel()[ih]
        z = t * (d[ih] @ sc.optical_axis(poses[v]))
        assert (z <= t * (1 + 1e-12)).all() and (t - z).max() > 0.05    # the two conventions differ by more than a depth bar somewhere
        for name in ("depth", "median"):
            got = r[name][v][ih]
            for stat in ("median", "p95", "rmse"):
                along, depthwise = sc.err_stats(got - t)[stat], sc.err_stats(got - z)[stat]
                ok = along < depthwise
                print(f"ANALYTIC {fig.title} view {v} {name} {stat}: against t {along:.5g} < against z {depthwise:.5g}  {'ok' if ok else 'MISS'}")
                if not ok:
                    fig.missed.append((v, name, stat, along, depthwise))
    fig.done()


# ---------------------------------------------------------------------------------------------------- 3. occupancy
@pytest.mark.parametrize("contraction", [True, False])
def test_occupancy_grid_covers_the_surface_and_little_else(contraction):
    model, _ = _trained(contraction)
    config = _config_name(contraction)
    b = model.occupancy_grid.binaries[0].cpu().numpy()
    r = CFG["grid_resolution"]
    assert b.shape == (r, r, r)
    pts, _, _ = sc.surface_samples(4000)
    cells = np.unique(np.clip(np.floor((pts + 1.0) / 2.0 * r).astype(np.int64), 0, r - 1), axis=0)
    fig = Figures(f"occupancy[{config}]")
    fig.at_most("occupied fraction", float(b.mean()), config, "occupied_fraction")
    fig.at_least("surface cells occupied", float(b[cells[:, 0], cells[:, 1], cells[:, 2]].mean()), config, "surface_cells_occupied")
    # and the axis order of the grid is the scene's: the occupied cells' centre of mass lies where the bodies' does, not at a permutation of it
    centre = (np.argwhere(b).mean(0) + 0.5) / r * 2 - 1
    want = (np.argwhere(sc.sdf(((np.indices((r, r, r)).reshape(3, -1).T + 0.5) / r * 2 - 1)).reshape(r, r, r) < 0.03).mean(0) + 0.5) / r * 2 - 1
    print(f"ANALYTIC {fig.title} centre of the occupied cells {centre.round(3).tolist()} against the scene's shell {want.round(3).tolist()}")
    assert np.abs(centre - want).max() < 0.06
    fig.done()


# ---------------------------------------------------------------------------------------------------- 4. normals
@pytest.mark.parametrize("contraction", [True, False])
def test_rendered_normals_point_out_of_the_bodies(contraction):
    config = _config_name(contraction)
    r = _renders((contraction,))
    truth = _truth("heldout")[1]
    fig = Figures(f"normals[{config}]")
    for v in range(CFG["n_heldout"]):
        _, ih, _ = _masks("heldout", v)
        n = r["normals"][v][ih]
        assert np.abs(np.linalg.norm(n, axis=-1) - 1).max() < 1e-3
        cosang = np.clip((n * truth["normal"][v].reshape(-1, 3)[ih]).sum(-1), -1, 1)
        ang = np.degrees(np.arccos(cosang))
        fig.at_most(f"view {v} mean angle", float(ang.mean()), config, "normal_mean_deg", v)
        fig.at_most(f"view {v} p95 angle", float(np.percentile(ang, 95)), config, "normal_p95_deg", v)
        fig.at_least(f"view {v} within 90 degrees", float((cosang > 0).mean()), config, "normal_within_90", v, factor=1.0)
    fig.done()


def test_field_normals_equal_world_normals_in_a_cube_without_contraction():
    """Without contraction the normalisation is the diagonal aabb scaling, and this aabb is a cube: the scaling is uniform and drops
    out of a unit vector."""
    world, fld = _renders((False,))["normals"], _renders((False,), "heldout", "bf16x6", "field")["normals"]
    worst = 0.0
    for v in range(CFG["n_heldout"]):
        _, ih, _ = _masks("heldout", v)
        worst = max(worst, float(np.abs(world[v][ih] - fld[v][ih]).max()))
    print(f"ANALYTIC normals[contraction_off] field against world: largest difference {worst:.3g}")
    assert worst < 1e-5            # two float32 routes to the same unit vector


# ---------------------------------------------------------------------------------------------------- 5. density mesh
@pytest.mark.parametrize("contraction", [True, False])
def test_density_mesh_lies_on_the_surface_and_faces_outwards(contraction):
    from lsenerf_amd import mesh as lm
    model, _ = _trained(contraction)
    config = _config_name(contraction)
    mesh = lm.extract_mesh(model, resolution=CFG["lattice"], bounds=BOUNDS)
    v, t = mesh.vertices.cpu().numpy(), mesh.triangles.cpu().numpy()
    cell = 2.0 / CFG["lattice"]
    s = sc.mesh_stats(v, t, mr.signed_volume, near=cell)
    facing = (mesh.normals.cpu().numpy().astype(np.float64) * sc.outward_normal(v)).sum(-1) > 0
    fig = Figures(f"density mesh[{config}]")
    fig.at_most("|sdf| p50", s["sdf_p50"], config, "density_mesh_sdf_p50")
    fig.at_most("|sdf| p95", s["sdf_p95"], config, "density_mesh_sdf_p95")
    fig.at_least("outward share of the triangles", s["outward_share"], config, "density_mesh_outward_share", factor=1.0)
    fig.at_least("outward share of the triangles within a cell of the surface", s["outward_share_near"], config,
                 "density_mesh_outward_share_near", factor=1.0)
    fig.at_least("vertex normals within 90 degrees", float(facing.mean()), config, "density_mesh_normals_within_90", factor=1.0)
    fig.at_least("vertex normals within 90 degrees, within a cell of the surface", float(facing[np.abs(sc.sdf(v)) < cell].mean()), config,
                 "density_mesh_normals_within_90_near", factor=1.0)
    print(f"ANALYTIC {fig.title} sign of the signed volume: gpu {s['volume_sign']:+.0f}  oracle {_values(config, 'density_mesh_volume_sign')}  "
          f"vertices {s['vertices']}")
    assert s["volume_sign"] == 1.0 and set(_values(config, "density_mesh_volume_sign")) == {1.0}
    fig.done()


# ---------------------------------------------------------------------------------------------------- 6. TSDF mesh and point cloud
@functools.lru_cache(maxsize=None)
def _train_rms_interior(contraction):
    r = _renders((contraction,), "train")
    truth = _truth("train")[1]
    inner = sc.interior(truth["body"]).reshape(CFG["n_train"], -1)
    return float(np.sqrt(((r["rgb"] - truth["rgb8"].reshape(CFG["n_train"], -1, 3) / 255.0)[inner] ** 2).mean()))


def _colour_margin(config, prefix):
    """The exported colours' rms over the same model's interior image rms: the oracle's worst seed plus twice its spread."""
    runs = ORACLE["runs"][config]
    ratio = [r[prefix + "_colour_rms"] / r["train_rms_interior"] for r in runs.values()]
    if len(ratio) < 2:
        other = [r[prefix + "_colour_rms"] / r["train_rms_interior"] for r in ORACLE["runs"]["contraction_on"].values()]
        return max(ratio) + 2 * (max(other) - min(other))
    return max(ratio) + 2 * (max(ratio) - min(ratio))


@pytest.mark.parametrize("depth", ["expected", "median"])
@pytest.mark.parametrize("contraction", [True, False])
def test_tsdf_mesh_and_point_cloud_of_the_training_views(contraction, depth):
    model, _ = _trained(contraction)
    config = _config_name(contraction)
    es = _eval_set("train")
    samples = sc.visible_surface_samples(_truth("train")[0])
    radius = 2 * 2.0 / CFG["lattice"]                                   # two lattice cells
    rms = _train_rms_interior(contraction)
    fig = Figures(f"exports[{config}, {depth}]")
    mesh = model.export_tsdf_mesh(es, resolution=CFG["lattice"], bounds=BOUNDS, depth=depth, normals=False)
    cloud = model.export_point_cloud(es, bounds=BOUNDS, normals=False, depth=depth)
    for prefix, pts, col in (("tsdf", mesh.vertices, mesh.colors), ("cloud", cloud.points, cloud.colors)):
        s = sc.cloud_stats(pts.cpu().numpy(), col.cpu().numpy(), samples, radius)
        key = f"{prefix}_{depth}"
        fig.at_most(f"{prefix} |sdf| p50", s["sdf_p50"], config, key + "_sdf_p50")
        fig.at_most(f"{prefix} |sdf| p95", s["sdf_p95"], config, key + "_sdf_p95")
        fig.at_least(f"{prefix} coverage of the visible surface", s["coverage"], config, key + "_coverage")
        bar = rms * _colour_margin(config, key)
        ok = s["colour_rms"] <= bar
        print(f"ANALYTIC {fig.title} {prefix} colour rms: gpu {s['colour_rms']:.5g} <= {bar:.5g} = interior image rms {rms:.5g} x margin "
              f"{_colour_margin(config, key):.4g}  points {s['points']}  {'ok' if ok else 'MISS'}")
        if not ok:
            fig.missed.append((prefix + " colour rms", s["colour_rms"], bar))
    fig.done()


# ---------------------------------------------------------------------------------------------------- 7. events
def test_event_frames_have_the_polarity_of_the_scene():
    from lsenerf_amd import events
    model, _ = _trained(True)
    poses, truth = _truth("trajectory")
    c = CFG["event_threshold"]
    want = sc.event_frames(truth["rgb8"] / 255.0, c)
    p = torch.from_numpy(np.asarray(poses, np.float32))
    pairs = torch.stack([p[:-1], p[1:]], 1).cuda()                      # [7, 2, 3, 4]: every frame between two consecutive poses
    got = events.predict_event_frames(model, _cameras(poses), pairs, c).cpu().numpy().astype(np.float64)
    assert got.shape == want.shape
    strong = np.abs(want) >= 2
    fig = Figures("events[contraction_on]")
    fig.at_least("sign agreement where |analytic| >= 2", float((np.sign(got[strong]) == np.sign(want[strong])).mean()), "contraction_on",
                 "event_sign_agreement")
    fig.inside("mean of predicted - analytic", float((got - want).mean()), "contraction_on", "event_mean_difference")
    fig.record("share of strong pixels", float(strong.mean()))
    fig.done()


# ---------------------------------------------------------------------------------------------------- 8. reduced-precision eval
def test_bf16x3_eval_stays_inside_the_bf16x6_bars():
    fig = Figures("renders[contraction_on, bf16x3]")
    _render_figures(fig, (True,), "contraction_on", arith="bf16x3")
    fig.done()


def test_bf16x1_eval_still_separates_hit_from_miss():
    """Recorded, not barred: what plain bf16 operands do to a trained scene is a finding (profiles/analytic_scene.txt,
    lsenerf_amd/model.py: eval_mlp_arith), not a number to invent.  Asserted: finite figures, and hit / miss separated on the interior."""
    fig = Figures("renders[contraction_on, bf16x1]")
    _render_figures(fig, (True,), "contraction_on", arith="bf16x1", bars=False)
    r = _renders((True,), "heldout", "bf16x1")
    assert all(np.isfinite(r[k]).all() for k in ("rgb", "acc", "depth", "median"))
    fig.done()


# ---------------------------------------------------------------------------------------------------- 9. the distortion term
def _heldout_distortion(key):
    """Mean per-ray distortion over the held-out rays: ``ops.distortion_loss`` on the samples the eval render marches (the calls of
    ``evaluation._render_count_free``) and the weights of ``ops.volume_render_depth`` on them."""
    from lsenerf_amd import ops
    model, _ = _trained(*key)
    cfg, fld = model.config, model.field
    total, rays = 0.0, 0
    with torch.no_grad():
        for i in range(CFG["n_heldout"]):
            rb = _bundle("heldout", i)
            ri, ts, te, packed, n_dev = model.sampler.sample_packed(rb, near_plane=cfg.near_plane, far_plane=cfg.far_plane,
                                                                    render_step_size=cfg.render_step_size, alpha_thre=cfg.alpha_thre,
                                                                    cone_angle=cfg.cone_angle)
            o, d = rb.origins.contiguous(), rb.directions.contiguous()
            table, eidx = fld._eval_emb(len(rb), o.device)
            sigma, _, _, head = fld.density_rgb_packed(o, d, ri, ts, te, packed, eidx, table, n_dev)
            weights = ops.volume_render_depth(ts, te, sigma, head, packed)[3]
            per_ray = ops.distortion_loss(ts, te, sigma, weights, packed, T_SCALE)
            assert per_ray.shape == (len(rb),)
            total += float(per_ray.double().sum())
            rays += len(rb)
        model.occupancy_grid.check_deferred_overflow()
    return total / rays


def test_distortion_term_concentrates_the_weights_and_keeps_the_render():
    base = _heldout_distortion((True,))
    other = _heldout_distortion((True, 0.0, CFG["draw_seed"] + 1))         # a second baseline: another draw of the pixels
    noise = abs(base - other)
    print(f"ANALYTIC distortion baseline {base:.5g}, second baseline {other:.5g}: difference {noise:.3g}")
    kept = None
    for mult in (0.01, 0.1, 1.0):
        got = _heldout_distortion((True, mult))
        met = base - got > 2 * noise
        print(f"ANALYTIC distortion multiplier {mult}: held-out distortion {got:.5g}, lowered by {base - got:.3g} against 2 x {noise:.3g}  "
              f"{'met' if met else 'not met'}")
        if met:
            kept = mult
            break
    assert kept is not None, "no multiplier lowered the held-out distortion by more than twice the baselines' difference"
    fig = Figures(f"renders[contraction_on, distortion x {kept}]")
    _render_figures(fig, (True, kept), "contraction_on")
    fig.done()
