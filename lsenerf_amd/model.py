"""``LSENeRFModel`` -- the hot-path driver with the reference's model interface.

Mirrors R:lse_nerf/lsenerf.py: ``LSENeRFModelConfig`` (:47-99, plus the nerfstudio ``InstantNGPModelConfig``
defaults the reference inherits), ``populate_modules`` (:158-228), ``forward`` (:265-276),
``exec_get_outputs`` (:278-326), ``get_outputs`` (:329-377), ``get_param_groups`` (:231-249) and the losses
(:392-439).  nerfstudio's ``VolumetricSampler`` is restated as a small module.

The fast path keeps samples packed: one sampler call, one field pass, ONE volume-rendering kernel that yields
weights, rgb, accumulation and the depth numerator (the reference composes pack_info + render_weight_from_density
+ three index_add_ renderers).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from . import evaluation, ops
from .field import LSEEmbeddingConfig, LSEField
from .grid_estimator import LSEOccGridEstimator
from .rays import Frustums, RayBundle, RaySamples, SceneBox, SceneContraction
from .renderer import AccumulationRenderer, DepthRenderer, LinearRenderer, RGBRenderer

EPS = 1e-6   # R:lse_nerf/utils.py:12


@dataclass
class LSENeRFModelConfig:
    # --- InstantNGPModelConfig defaults inherited at R:lse_nerf/lsenerf.py:48
    grid_resolution: int = 128
    grid_levels: int = 4
    max_res: int = 2048
    log2_hashmap_size: int = 19
    alpha_thre: float = 0.01
    cone_angle: float = 0.004
    render_step_size: Optional[float] = None
    near_plane: float = 0.05
    far_plane: float = 1e3
    background_color: str = "random"
    disable_scene_contraction: bool = False
    eval_num_rays_per_chunk: int = 3512          # R:lse_nerf/lse_config.py:27
    # --- R:lse_nerf/lsenerf.py:50-84
    evs_loss_weight: float = 1.0
    emb_norm_weight: float = 1e-2
    event_loss_type: str = "log_loss"
    use_mapping: bool = False
    mapping_method: str = "mlp"                      # (only read when use_mapping is on; the presets pass it explicitly)
    evs_mapping_method: Optional[str] = "None"
    ev_one_dim: object = "learned"
    rgb_loss_type: str = "linspace"
    use_mapper_loss: bool = False                    # carried for call compatibility: nothing in the reference reads these three
    mapper_loss_weight: float = 0.25
    scaler_weight: float = 1.0
    map_mode: str = "ev_rgb"                         # the reference's default spelling; routing only looks at it with use_mapping
    embed_config: LSEEmbeddingConfig = field(default_factory=LSEEmbeddingConfig)
    # --- field size knobs (BASELINE config 1 uses L=4, 2x32)
    num_levels: int = 16
    hidden_dim: int = 64
    hidden_dim_color: int = 64
    # --- refresh the occupancy grid through occ_refresh.DeviceGridRefresher: no host synchronisation, replayable as a HIP graph
    device_grid_refresh: bool = False
    # --- early ray termination of the whole-image eval render (evaluation._render_early_stop).  0 = off: every route
    # and output is what it is without these two fields.  With 0 < eps < 1 a chunk of the count-free eval route is composited in
    # segments of the ray and a ray whose transmittance has dropped to eps or below at the end of a segment (optical depth >=
    # float32(-ln eps)) is not evaluated any further: its outputs are those of the full render for a ray cut at that segment
    # boundary, bit for bit, "num_samples_per_ray" is the number of samples composited, and the weight left behind is below eps.
    # Ignored -- the full ``forward`` loop runs, as with 0 -- wherever the count-free route is not available: training mode, a field
    # other than LSEField, the small-grid base MLP, or a chunk capacity above ``deferred_max_slots``.  Checked at render time
    # (ValueError unless 0 <= eps < 1).  Measured on one MI355X (tools/bench_eval_early_stop.py, 640 x 480, eps 1e-4):
    # with opaque surfaces and chunks of 32768 rays 22.6 ms per image against 38.9 ms; at the default chunk of 3512 rays it LOSES,
    # 72 ms against 43.5 ms, whether 26 % or all of the samples are evaluated (five segments per chunk are five times the launches:
    # what is paid there is issuing them), and on a field without opaque surfaces it costs 3 % at chunk 32768.  Switch it on
    # together with a large ``eval_num_rays_per_chunk``.
    eval_early_stop_eps: float = 0.0
    # base segment length S, a positive multiple of 64 (checked at render time): the segments are S, S, 2S, 4S, ... samples long
    # (evaluation.segment_schedule), each a fixed set of launches whether or not a ray is still alive.
    eval_segment_samples: int = 128
    # the reference's "overlay" image (R:lse_nerf/lsenerf.py:462-475: Canny edges of ground truth and prediction) in the image
    # dictionaries of ``get_image_metrics_and_images`` and ``evaluate_set``'s ``on_image``, after "err_map".  Computed on the
    # device (``ops.canny_edges``; OpenCV's published algorithm restated, parity unpinned).  Off: the dictionaries are as before.
    eval_overlay: bool = False
    # --- arithmetic of the two fused MLPs in the eval render: "bf16x6" (what trains: six bf16 piece products per multiply, f32's
    # error bound), "bf16x3" (two pieces per operand, three products, relative error 2^-16 per multiply) or "bf16x1" (plain bf16
    # operands, 2^-8) -- include/lse_hip.h: lse_mlp_desc.arith.  Sets ``LSEField.inference_arith``: honoured where the field runs in
    # eval mode under torch.no_grad() (get_outputs_for_camera_ray_bundle, the early-stop route, evaluate_set, render_camera, the
    # eager eval ``forward``) and both MLPs are the production shapes; training mode -- occupancy refresh, visibility pre-pass,
    # frozen-field refinement -- always runs bf16x6, and so does a small-grid base MLP or a ``hidden_dim`` other than 64.  An
    # unknown name is a ValueError in ``populate_modules``.  Measured on one MI355X (tools/bench_eval_precision.py, 640 x 480, the
    # bench workload): 38.7 / 34.5 / 31.9 ms per image at chunks of 32768 rays and 43.2 / 39.0 / 37.5 ms at 3512 for
    # bf16x6 / bf16x3 / bf16x1 (the pair kernel alone: 0.506 / 0.320 / 0.226 ms per 4.19 M samples).  Against the bf16x6 image
    # bf16x3 keeps rgb at 128.8 dB (largest difference 2.4e-6) and, with opaque surfaces, at 103.2 dB (1.5e-4); bf16x1 at 72.4 dB
    # (1.6e-3) and 48.9 dB (single pixels move by 0.09, depth by 0.34: the density logit is off by ~0.03).  Prefer "bf16x3".
    # On a trained scene with a ground truth (tests/test_gpu_analytic_scene.py, profiles/analytic_scene.txt: a sphere and a box,
    # 400 steps, four held-out 64 x 48 views) "bf16x1" is not told apart from "bf16x6": PSNR against the analytic image 27.25 /
    # 26.54 / 28.43 / 26.55 dB against 27.26 / 26.54 / 28.43 / 26.55, expected-depth rms error 0.0428 / 0.0340 / 0.0497 / 0.0397
    # against 0.0428 / 0.0340 / 0.0497 / 0.0397, hit and miss separated on every interior pixel -- the field's own error (25 - 28
    # dB) is far above what the arithmetic adds.  A sharper field (more steps, more views) will show it earlier.
    eval_mlp_arith: str = "bf16x6"
    # --- rendered analytic normals in the eval render: "off", "field" (the gradient of the density logit with respect to the
    # normalised position, as nerfstudio's Field.get_normals has it) or "world" (that gradient through the transposed Jacobian of
    # the contraction / aabb normalisation first).  With it on, eval-mode renders carry outputs["normals"] [.., 3]: per sample
    # n = -g / max(|g|, 1e-12), per ray N = sum w n over the render weights, then N / (|N| + 1e-10) -- unit vectors, (0, 0, 0) for
    # a ray without weight.  Per chunk this adds three forward-only launches (lse_density_logit_grad, lse_hash_bwd_input,
    # lse_eval_composite_normals); the gradient always runs bf16x6, whatever ``eval_mlp_arith`` says.  Training mode never computes
    # normals.  Not built for the early-stop segment route: together with ``eval_early_stop_eps > 0`` it is a ValueError in
    # ``populate_modules``, and so is an unknown name.
    eval_normals: str = "off"
    # --- quantile depths in the eval render: up to four values strictly inside (0, 1), ascending; () = off, every route and output
    # as without it.  With it on, eval-mode renders on the count-free routes carry outputs["depth_quantiles"] [.., n_q] -- per q the
    # depth at which the ray's accumulated weight crosses q (0.5: the median depth) -- and outputs["depth_reached"] [.., 1] (uint8,
    # bit j: quantile j was crossed; where not, the depth is the last sample's mid-point, nerfstudio's clamp).  "depth" stays the
    # expected depth.  The crossing is searched on the optical depth the compositor's scan carries (tau >= -ln(1 - q), include/
    # lse_hip.h: lse_eval_depth_quantiles): one extra launch per chunk, or per segment on the early-stop route, where every q needs
    # 1 - q >= eval_early_stop_eps.  The spread between two quantiles says how concentrated a ray's surface is.  The ``forward``
    # loop (training mode, another field, the small-grid base MLP) has no quantile depths: ``render_flat`` raises there.  Checked
    # in ``populate_modules`` and at render time (ValueError).
    eval_depth_quantiles: Tuple[float, ...] = ()
    # the quantile depth is the exact crossing inside the sample under piecewise-constant density, a + (tau_q - tau_front) / sigma
    # clamped to the sample, instead of the sample's mid-point
    eval_depth_interpolate: bool = False
    # --- distortion loss of mip-NeRF 360 in the training step (nerfacc.losses.distortion; the reference has none, so 0 = off: no
    # loss key, no launch, every value as without these two fields).  With a multiplier > 0 a training-mode ``render_packed`` adds
    # outputs["distortion"] [R, 1] -- per ray sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 delta_i over the render weights and the
    # interval mid-points (include/lse_hip.h: lse_distortion_fwd) -- and ``train_step_bundles`` adds
    # loss_dict["distortion_loss"] = mult * its mean over all packed rays (colour, previous and next).  Two launches per step, one
    # forward and one backward that goes straight to d_sigma; both replay inside ``GraphedTrainStep``.  Not computed in eval mode,
    # nor while ``freeze_field`` is in effect (regularising a frozen field would only push the cameras around).  Negative or
    # non-finite values are a ValueError in ``populate_modules``.  Measured on one MI355X (tools/bench_distortion.py, the bench
    # workload of 4096 rays x 1024 samples, profiles/distortion_loss.txt): lse_distortion_fwd 0.018 ms against lse_volrend_fwd's
    # 0.029 ms, lse_distortion_bwd 0.036 ms against lse_volrend_bwd's 0.042 ms; the captured step 5.40 .. 5.42 ms with the
    # multiplier at 0.01 against 5.33 ms at 0 (+0.07 .. 0.10 ms, 1.3 .. 1.8 %).  On the analytic scene of tests/analytic_scene.py
    # (tests/test_gpu_analytic_scene.py, profiles/analytic_scene.txt: 400 steps, ``distortion_t_scale`` = 1 / 2.4, the mean per-ray
    # distortion of the eval weights over four held-out views): 0.0053 without the term and 0.0059 for a second training that draws
    # other pixels; 0.0040 with the multiplier at 0.01 -- less than twice that difference below the baseline, so not told apart from
    # it -- and 0.0016 at 0.1, where held-out PSNR and depth error stay inside the bars the baseline is held to (nerfstudio's nerfacto uses 0.002 on normalised distances, with proposal samplers).
    distortion_loss_mult: float = 0.0
    # the loss is taken on t_scale * t: it scales as t_scale (1 / the scene's extent along a ray makes it independent of the units)
    distortion_t_scale: float = 1.0

    def __post_init__(self):   # R:lse_nerf/lsenerf.py:86-99
        if self.evs_mapping_method is None or str(self.evs_mapping_method).lower() == "none":
            self.evs_mapping_method = None
        if self.map_mode.lower() == "none":
            self.map_mode = "evs_rgb"
        if isinstance(self.ev_one_dim, str):
            if self.ev_one_dim.lower() in ("false", "none"):
                self.ev_one_dim = False
            elif self.ev_one_dim.lower() == "true":
                self.ev_one_dim = "learned"
        if self.rgb_loss_type.lower() == "none":
            self.rgb_loss_type = "linspace"


class GbConfig:
    """R:lse_nerf/utils.py:14-19: process-wide run flags the reference flips from its eval scripts."""
    DO_PRETRAIN = False
    IS_EVAL = False
    IS_RENDER = False


gbconfig = GbConfig()


class _TrainingCallbackLocation:
    """nerfstudio.engine.callbacks.TrainingCallbackLocation (stand-in used only where nerfstudio is not installed)."""
    BEFORE_TRAIN_ITERATION = "before_train_iteration"
    AFTER_TRAIN_ITERATION = "after_train_iteration"
    AFTER_TRAIN = "after_train"


class _TrainingCallback:
    """nerfstudio.engine.callbacks.TrainingCallback stand-in: same constructor, attributes and run methods."""

    def __init__(self, where_to_run, func, update_every_num_iters=None, iters=None, args=None, kwargs=None):
        assert "step" in func.__code__.co_varnames if hasattr(func, "__code__") else True
        self.where_to_run, self.func = where_to_run, func
        self.update_every_num_iters, self.iters = update_every_num_iters, iters
        self.args, self.kwargs = (args if args is not None else []), (kwargs if kwargs is not None else {})

    def run_callback(self, step: int) -> None:
        if self.update_every_num_iters is not None:
            if step % self.update_every_num_iters == 0:
                self.func(*self.args, **self.kwargs, step=step)
        elif self.iters is not None:
            if step in self.iters:
                self.func(*self.args, **self.kwargs, step=step)

    def run_callback_at_location(self, step: int, location) -> None:
        if location in self.where_to_run:
            self.run_callback(step=step)

    def __call__(self, step: int) -> None:
        self.run_callback(step)


class ThreeToOne(nn.Module):
    """R:lse_nerf/lsenerf.py:102-109."""

    def __init__(self) -> None:
        super().__init__()
        self.weights = nn.Parameter(torch.ones(1, 3) / 3)

    def forward(self, x):
        return F.linear(x, F.softmax(self.weights, dim=-1), None)


class ToGrayGT(nn.Module):
    """R:lse_nerf/lsenerf.py:112-119."""

    def __init__(self) -> None:
        super().__init__()
        self.register_buffer("c2g_vec", torch.tensor([0.2989, 0.5870, 0.1140]).reshape(-1, 1))

    def forward(self, img):
        return img @ self.c2g_vec


class IdentityMapper(nn.Module):
    def forward(self, x, **kwargs):
        return x


class GT_Mapper(nn.Module):
    def forward(self, x, **kwargs):
        return x ** (1 / 2.4)


class Powpow(nn.Module):
    """R:lse_nerf/intensity_mappers.py:84-90."""

    def __init__(self) -> None:
        super().__init__()
        self.pow_coeff = nn.Parameter(torch.tensor([1.0], dtype=torch.float32))

    def forward(self, x, **kwargs):
        return x ** self.pow_coeff


class _SmallMLP(nn.Module):
    """nerfstudio ``MLP(in_dim, num_layers=4, layer_width=16, out_dim, ReLU, out_activation=Sigmoid, implementation="torch")``
    as the mappers of R:lse_nerf/intensity_mappers.py:30-62 build it: four ``nn.Linear`` layers (with bias), parameters named
    ``layers.{i}.weight / bias`` like nerfstudio's torch MLP so that a reference checkpoint loads."""

    def __init__(self, in_dim: int, out_dim: int, width: int = 16, num_layers: int = 4) -> None:
        super().__init__()
        dims = [in_dim] + [width] * (num_layers - 1) + [out_dim]
        self.layers = nn.ModuleList([nn.Linear(dims[i], dims[i + 1]) for i in range(num_layers)])

    def forward(self, x):
        for i, layer in enumerate(self.layers):
            x = layer(x)
            x = torch.relu(x) if i + 1 < len(self.layers) else torch.sigmoid(x)
        return x


def identity_init(mlp: nn.Module, in_dim: int = 3, out_dim: int = 3, n_steps: int = 5000) -> nn.Module:
    """R:lse_nerf/intensity_mappers.py:8-26: fit the mapper to the identity on 100 grey levels of [0, 1] (Adam, lr 5e-2, MSE)
    so that training starts from "no tone mapping".  Runs on the module's current device (the reference moves it to the GPU
    and back; it is 100 x 16 numbers)."""
    dev = next(mlp.parameters()).device
    lin = torch.linspace(0, 1, 100, device=dev)[..., None]
    inp, out_gt = torch.cat([lin] * in_dim, dim=-1), torch.cat([lin] * out_dim, dim=-1)
    opt = torch.optim.Adam(mlp.parameters(), lr=5e-2)
    with torch.enable_grad():
        for _ in range(n_steps):
            loss = F.mse_loss(mlp(inp), out_gt)
            opt.zero_grad()
            loss.backward()
            opt.step()
    for p in mlp.parameters():      # the fit's last gradient is not a training gradient: the first step accumulates from nothing
        p.grad = None
    return mlp


class MLP_Mapper(nn.Module):
    """R:lse_nerf/intensity_mappers.py:28-44 (one channel, e.g. behind ``ev_one_dim``)."""
    init_steps = 5000

    def __init__(self) -> None:
        super().__init__()
        self.mlp = identity_init(_SmallMLP(1, 1), 1, 1, self.init_steps)

    def forward(self, x, **kwargs):
        return self.mlp(x)


class RGB_MLP_Mapper(nn.Module):
    """R:lse_nerf/intensity_mappers.py:47-63 (three channels)."""
    init_steps = 5000

    def __init__(self) -> None:
        super().__init__()
        self.mlp = identity_init(_SmallMLP(3, 3), 3, 3, self.init_steps)

    def forward(self, x, **kwargs):
        return self.mlp(x)


# R:lse_nerf/intensity_mappers.py:93-97.  All five run inside the fused loss epilogue (the MLP mappers since ABI 6:
# csrc/epilogue.hip, epilogue_mlp_* kernels); the modules' own forward() serves evaluation and the torch route.
MAPPERS_DICT = {"mlp": MLP_Mapper, "rgb_mlp": RGB_MLP_Mapper, "gt": GT_Mapper, "identity": IdentityMapper, "powpow": Powpow}
format_linear = lambda x: torch.concatenate([x] * 3, dim=-1) if x.shape[-1] == 1 else x


def to_gray(x: Tensor) -> Tensor:
    return (x * x.new_tensor([0.2989, 0.5870, 0.1140])).sum(-1, keepdim=True)


class VolumetricSampler(nn.Module):
    """nerfstudio 0.3.2 ``VolumetricSampler`` (constructed at R:lse_nerf/lsenerf.py:191-194 with
    ``density_fn=self.field.density_fn``).

    ``density_fn`` is nerfstudio's positions -> density callable.  When it is the bound ``density_fn`` of an ``LSEField``
    the pre-pass evaluates that field on the packed samples directly (positions are formed inside ``lse_positions_fwd``
    from per-ray origins / directions -- no [N,3] gathers); any other callable takes nerfstudio's generic route
    (``origins[ray_indices] + directions[ray_indices] * (t_starts + t_ends) / 2`` -> ``density_fn``)."""

    def __init__(self, occupancy_grid: LSEOccGridEstimator, density_fn: Optional[Callable] = None):
        super().__init__()
        assert occupancy_grid is not None
        self.density_fn = density_fn
        self.occupancy_grid = occupancy_grid
        owner = getattr(density_fn, "__self__", None)
        # (the field is registered on the model, not here: keep a plain reference without making it a sub-module)
        object.__setattr__(self, "_packed_field", owner if isinstance(owner, LSEField) and
                           getattr(density_fn, "__func__", None) is LSEField.density_fn else None)

    def get_sigma_fn(self, origins, directions, times=None) -> Optional[Callable]:
        if self.density_fn is None or not self.training:
            return None
        density_fn, fld = self.density_fn, self._packed_field
        if fld is not None:
            return fld.prepass_sigma_fn(origins, directions)

        def sigma_fn(t_starts, t_ends, ray_indices):
            ri = ray_indices.long()
            positions = origins[ri] + directions[ri] * (t_starts + t_ends)[:, None] / 2.0
            if times is None:
                return density_fn(positions).squeeze(-1)
            return density_fn(positions, times[ri]).squeeze(-1)
        return sigma_fn

    def premarch(self, ray_bundle: RayBundle, render_step_size: float, near_plane: float = 0.0, far_plane=None,
                 cone_angle: float = 0.0, jitter: Optional[Tensor] = None, out=None):
        """The marcher of ``sample_packed`` alone (LSEOccGridEstimator.march_deferred): it needs the rays and the grid only, so it
        may be launched ahead of the step that consumes the samples; hand the result to ``sample_packed(premarched=...)``."""
        t_min = ray_bundle.nears.contiguous().reshape(-1) if ray_bundle.nears is not None else None
        t_max = ray_bundle.fars.contiguous().reshape(-1) if ray_bundle.fars is not None else None
        return self.occupancy_grid.march_deferred(
            ray_bundle.origins.detach().contiguous(), ray_bundle.directions.detach().contiguous(), near_plane=near_plane,
            far_plane=1e10 if far_plane is None else far_plane, t_min=t_min, t_max=t_max, render_step_size=render_step_size,
            stratified=self.training, cone_angle=cone_angle, jitter=jitter, out=out)

    def march_slots(self, ray_bundle: RayBundle, render_step_size: float, near_plane: float = 0.0, far_plane=None,
                    cone_angle: float = 0.0, jitter: Optional[Tensor] = None):
        """The marcher of ``sample_packed`` with the samples left in their per-ray slots (LSEOccGridEstimator.march_slots): (cnts,
        t_start_slots, t_end_slots, cap).  No visibility pre-pass and no fake sample: the early-stop eval route, which packs the
        slots a segment at a time, runs in eval mode (no pre-pass there) and inserts the fake sample into its first segment."""
        t_min = ray_bundle.nears.contiguous().reshape(-1) if ray_bundle.nears is not None else None
        t_max = ray_bundle.fars.contiguous().reshape(-1) if ray_bundle.fars is not None else None
        res = self.occupancy_grid.march_slots(
            ray_bundle.origins.detach().contiguous(), ray_bundle.directions.detach().contiguous(), near_plane=near_plane,
            far_plane=1e10 if far_plane is None else far_plane, t_min=t_min, t_max=t_max, render_step_size=render_step_size,
            stratified=self.training, cone_angle=cone_angle, jitter=jitter)
        if self.occupancy_grid.after_march_hook is not None:
            self.occupancy_grid.after_march_hook()
        return res

    def sample_packed(self, ray_bundle: RayBundle, render_step_size: float, near_plane: float = 0.0, far_plane=None,
                      alpha_thre: float = 0.01, cone_angle: float = 0.0, jitter: Optional[Tensor] = None, premarched=None):
        """The sampler call of ``forward`` for the packed fast path, WITHOUT reading a sample count back to the host and without
        building per-sample ``RaySamples`` (gathered origins / directions / camera indices): returns (ray_indices int32,
        t_starts, t_ends, packed_info, n_dev) with capacity-extent arrays (LSEOccGridEstimator.sampling(deferred=True))."""
        rays_o = ray_bundle.origins.contiguous()
        rays_d = ray_bundle.directions.contiguous()
        t_min = ray_bundle.nears.contiguous().reshape(-1) if ray_bundle.nears is not None else None
        t_max = ray_bundle.fars.contiguous().reshape(-1) if ray_bundle.fars is not None else None
        ri, ts, te, packed, n_dev = self.occupancy_grid.sampling(
            rays_o=rays_o.detach(), rays_d=rays_d.detach(), t_min=t_min, t_max=t_max,
            sigma_fn=self.get_sigma_fn(rays_o.detach(), rays_d.detach(), ray_bundle.times),
            render_step_size=render_step_size, near_plane=near_plane, far_plane=1e10 if far_plane is None else far_plane,
            stratified=self.training, cone_angle=cone_angle, alpha_thre=alpha_thre, jitter=jitter, deferred=True,
            premarched=premarched)
        # "create a single fake sample" of forward(), on the device.  The pre-pass features parked for exactly these buffers (the
        # main pass takes them instead of encoding the survivors again) hold nothing for the slot the fake sample lands in
        pp = getattr(self._packed_field, "_prepass", None) if self._packed_field is not None else None
        feats = None
        if pp is not None and pp["key"][:2] == (ts.data_ptr(), ri.data_ptr()) and pp["x01"].shape[0] > 0:
            feats = (pp["x01"], pp["sel"], pp["y"])
        ops.fake_sample_if_empty(packed, n_dev, ri, ts, te, features=feats)
        return ri, ts, te, packed, n_dev

    def forward(self, ray_bundle: RayBundle, render_step_size: float, near_plane: float = 0.0, far_plane=None,
                alpha_thre: float = 0.01, cone_angle: float = 0.0, jitter: Optional[Tensor] = None
                ) -> Tuple[RaySamples, Tensor]:
        rays_o = ray_bundle.origins.contiguous()
        rays_d = ray_bundle.directions.contiguous()
        t_min = ray_bundle.nears.contiguous().reshape(-1) if ray_bundle.nears is not None else None
        t_max = ray_bundle.fars.contiguous().reshape(-1) if ray_bundle.fars is not None else None
        if far_plane is None:
            far_plane = 1e10
        camera_indices = ray_bundle.camera_indices
        ray_indices, starts, ends, packed_info = self.occupancy_grid.sampling(
            rays_o=rays_o, rays_d=rays_d, t_min=t_min, t_max=t_max,
            sigma_fn=self.get_sigma_fn(rays_o, rays_d, ray_bundle.times),
            render_step_size=render_step_size, near_plane=near_plane, far_plane=far_plane, stratified=self.training,
            cone_angle=cone_angle, alpha_thre=alpha_thre, jitter=jitter, return_packed=True)
        num_samples = starts.shape[0]
        if num_samples == 0:   # create a single fake sample (nerfstudio) and update packed_info accordingly
            dev = rays_o.device
            ray_indices = torch.zeros((1,), dtype=torch.int32, device=dev)
            starts = torch.ones((1,), dtype=starts.dtype, device=dev)
            ends = torch.ones((1,), dtype=ends.dtype, device=dev)
            packed_info = torch.zeros((rays_o.shape[0], 2), dtype=torch.int64, device=dev)
            packed_info[0, 1] = 1
        li = ray_indices.long()
        ray_samples = RaySamples(
            frustums=Frustums(origins=rays_o[li], directions=rays_d[li], starts=starts[..., None], ends=ends[..., None],
                              pixel_area=ray_bundle.pixel_area[li] if ray_bundle.pixel_area is not None else None),
            camera_indices=camera_indices[li] if camera_indices is not None else None,
            ray_indices=ray_indices, packed_info=packed_info, ray_bundle=ray_bundle)
        if ray_bundle.times is not None:
            ray_samples.times = ray_bundle.times[li]
        return ray_samples, li


class LSENeRFModel(nn.Module):
    """R:lse_nerf/lsenerf.py:141-439 (NGPModel subclass upstream)."""

    def __init__(self, config: LSENeRFModelConfig, scene_box, num_train_data: int, **kwargs) -> None:
        """``scene_box``: a nerfstudio-style ``SceneBox`` (anything with ``.aabb`` [2,3]) as nerfstudio's
        ``Model.__init__(config, scene_box, num_train_data, **kwargs)`` receives it, or the aabb tensor itself."""
        super().__init__()
        if not isinstance(config, LSENeRFModelConfig):      # nerfstudio hands over ITS config object (ns_plugin entry point)
            from .ns_plugin import convert_model_config
            config = convert_model_config(config)
        self.config = config
        self.scene_box = scene_box if hasattr(scene_box, "aabb") else SceneBox(aabb=scene_box.float().reshape(2, 3))
        self.scene_aabb_2x3 = self.scene_box.aabb.float().reshape(2, 3)
        self.num_train_data = num_train_data
        self.kwargs = kwargs
        self.collider = None                       # enable_collider False for NGP
        # training fast path without host read-backs of the sample counts (LSEOccGridEstimator.sampling(deferred=True)); the
        # values are those of the synchronising path bit for bit (tests/test_gpu_deferred.py).  Buffers are sized by a proven
        # capacity (about 3x the samples in the reference's default configuration, 1.5x for M-march) instead of the exact
        # count; a batch whose capacity would exceed `deferred_max_slots` packed samples takes the synchronising path.
        self.deferred_counts = True
        self.deferred_max_slots = 1 << 24      # (a 4-level grid marched with cone 0 has a loose bound: 8040 slots per ray -- 33 M for
                                               #  4096 rays, whose early-exit workgroups cost 0.27 ms: measured, bench.py inside-box)
        self.populate_modules()
        self.log_losses_dict = {"log_loss": self.log_loss, "enerf_norm_loss": self.enerf_norm_loss}
        self.rgb_losses_dic = {"linspace": self.mse_loss, "deblur": self.mse_loss}
        self.rgb_loss_fn = self.rgb_losses_dic[self.config.rgb_loss_type.lower()]
        self.event_loss = self.log_losses_dict[self.config.event_loss_type.lower()]

    # -- R:lse_nerf/lsenerf.py:158-228 ----------------------------------------------------------------
    def populate_modules(self):
        cfg = self.config
        if cfg.eval_mlp_arith not in ops.MLP_ARITH_ROUTES:
            raise ValueError(f"eval_mlp_arith {cfg.eval_mlp_arith!r}: one of {sorted(ops.MLP_ARITH_ROUTES)}")
        if cfg.eval_normals not in ("off", "field", "world"):
            raise ValueError(f"eval_normals {cfg.eval_normals!r}: one of 'off', 'field', 'world'")
        if cfg.eval_normals != "off" and cfg.eval_early_stop_eps > 0:
            raise ValueError("eval_normals is not built for the early-stop segment route: set eval_early_stop_eps = 0 "
                             f"(got eval_normals={cfg.eval_normals!r}, eval_early_stop_eps={cfg.eval_early_stop_eps})")
        evaluation.depth_quantile_settings(cfg)
        for name in ("distortion_loss_mult", "distortion_t_scale"):
            v = getattr(cfg, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not (0.0 <= v < float("inf")):
                raise ValueError(f"{name} {v!r}: a finite number >= 0")
        scene_contraction = None if cfg.disable_scene_contraction else SceneContraction(order=float("inf"))
        self.field = LSEField(aabb=self.scene_aabb_2x3, num_images=self.num_train_data,
                              log2_hashmap_size=cfg.log2_hashmap_size, max_res=cfg.max_res,
                              spatial_distortion=scene_contraction, embd_config=cfg.embed_config, implementation="tcnn",
                              num_levels=cfg.num_levels, hidden_dim=cfg.hidden_dim,      # (field-size knobs: BASELINE config 1)
                              hidden_dim_color=cfg.hidden_dim_color)
        self.field.inference_arith = cfg.eval_mlp_arith
        self.scene_aabb = nn.Parameter(self.scene_aabb_2x3.flatten(), requires_grad=False)
        if cfg.render_step_size is None:   # auto step size: ~1000 samples in the base level grid
            cfg.render_step_size = ((self.scene_aabb[3:] - self.scene_aabb[:3]) ** 2).sum().sqrt().item() / 1000
        self.occupancy_grid = LSEOccGridEstimator(roi_aabb=self.scene_aabb.data, resolution=cfg.grid_resolution,
                                                  levels=cfg.grid_levels)
        self.sampler = VolumetricSampler(occupancy_grid=self.occupancy_grid, density_fn=self.field.density_fn)
        self.renderer_rgb = RGBRenderer(background_color=cfg.background_color)
        self.renderer_accumulation = AccumulationRenderer()
        self.renderer_depth = DepthRenderer(method="expected")
        self.rgb_loss = nn.MSELoss()
        if cfg.use_mapping:
            init = MAPPERS_DICT.get(cfg.mapping_method.lower())
            assert init is not None, f"{cfg.mapping_method} mapper is not supported"
            self.rgb_mapper = init()
            self.renderer_rgb = LinearRenderer(background_color=cfg.background_color)
        self.evs_mapper = None
        if cfg.evs_mapping_method is not None and cfg.map_mode == "co_map":
            init = MAPPERS_DICT.get(cfg.evs_mapping_method.lower())
            assert init is not None, f"{cfg.evs_mapping_method} mapper is not supported"
            self.evs_mapper = init()
        if cfg.ev_one_dim == "learned":
            self.rgb_to_one = ThreeToOne()
        elif cfg.ev_one_dim == "gt":
            self.rgb_to_one = ToGrayGT()

    def update_occupancy_grid(self, step: int) -> None:
        """The body of NGPModel's training callback: refresh the occupancy grid from ``density * render_step_size``.
        On the steps that refresh (every 16th; they synchronise with the device anyway) the count-free sampler's sticky
        overflow accumulator is read first: a violated per-ray capacity (truncated rays) raises here, in the eager and in the
        graph-replayed training step alike, at most 16 steps after it happened."""
        if self.training and step % 16 == 0:
            self.occupancy_grid.check_deferred_overflow()
        if self.config.device_grid_refresh:
            # the same update rule with every count on the device (lsenerf_amd/occ_refresh.py): nothing below waits for the GPU
            if not self.occupancy_grid.training:
                raise RuntimeError("You should only call this function only during training. "
                                   "Please call _update() directly if you want to update the field during inference.")
            if step % 16 == 0:
                self.grid_refresher().refresh(step)
            return
        self.occupancy_grid.update_every_n_steps(
            step=step, occ_eval_fn=lambda x: self.field.density_fn(x) * self.config.render_step_size)

    def grid_refresher(self):
        """The model's ``occ_refresh.DeviceGridRefresher`` (``config.device_grid_refresh``), built on first use; call its
        ``capture()`` to turn the refresh into one graph replay."""
        r = self.__dict__.get("_grid_refresher")
        if r is None or r.estimator.occs.device != self.occupancy_grid.occs.device:
            from .occ_refresh import DeviceGridRefresher
            r = self.__dict__["_grid_refresher"] = DeviceGridRefresher(self.occupancy_grid, self.field,
                                                                       self.config.render_step_size)
        return r

    def get_training_callbacks(self, training_callback_attributes=None) -> List[object]:
        """nerfstudio 0.3.2 ``NGPModel.get_training_callbacks(training_callback_attributes)`` (inherited by the reference,
        R:lse_nerf/lsenerf.py:141): one callback, before every train iteration, that refreshes the occupancy grid.  With
        nerfstudio importable this is its ``TrainingCallback(where_to_run=[BEFORE_TRAIN_ITERATION], update_every_num_iters=1,
        func=...)`` object, which the Trainer drives through ``run_callback_at_location``; without nerfstudio (this image) a
        ``TrainingCallback`` stand-in with the same attributes and ``run_callback`` / ``run_callback_at_location`` methods,
        which is also directly callable with the step."""
        try:
            from nerfstudio.engine.callbacks import TrainingCallback, TrainingCallbackLocation
        except ModuleNotFoundError:
            TrainingCallback, TrainingCallbackLocation = _TrainingCallback, _TrainingCallbackLocation
        return [TrainingCallback(where_to_run=[TrainingCallbackLocation.BEFORE_TRAIN_ITERATION], update_every_num_iters=1,
                                 func=self.update_occupancy_grid)]

    def get_param_groups(self) -> Dict[str, List[nn.Parameter]]:
        """R:lse_nerf/lsenerf.py:231-249 (NGPModel: {"fields": field parameters}).  In an evaluation run (``gbconfig.IS_EVAL``,
        :246-247) only the appearance embedding is optimised: the radiance field is frozen and the test-time embedding fitted."""
        groups = {"fields": self._training_field_params()}
        if gbconfig.IS_EVAL and self.config.mapping_method != "gt":      # (the reference returns before this line for "gt")
            groups["fields"] = list(self.field.embedding_appearance.parameters())
        return groups

    def _training_field_params(self) -> List[nn.Parameter]:
        """What ``get_param_groups()["fields"]`` lists in a TRAINING run, whatever ``gbconfig.IS_EVAL`` says."""
        fields = list(self.field.parameters())
        if self.config.mapping_method == "gt":
            return fields
        if self.config.use_mapping:
            fields += list(self.rgb_mapper.parameters())
        if self.config.ev_one_dim:
            fields += list(self.rgb_to_one.parameters())
        if self.config.evs_mapping_method is not None and self.evs_mapper is not None:
            fields += list(self.evs_mapper.parameters())
        return fields

    def freeze_field(self, train_embedding: bool = True, input_only_mlp: bool = False) -> List[nn.Parameter]:
        """Freeze the radiance field for a test-time refinement run (R:lse_nerf/lsenerf.py:246-247, R:scripts/emb_eval.sh):
        ``requires_grad_(False)`` on every parameter a training run optimises -- hash table, both MLPs, side heads, mappers,
        ``rgb_to_one`` -- except, with ``train_embedding``, the appearance embedding's (its ``test_emb`` row included once
        ``init_test_params`` has made one).  Returns the parameters left trainable (``[]`` without ``train_embedding``, or without an
        embedding): what the refinement's ``FlatAdam`` is built over.  The step of a frozen field computes no table gradient and
        hands no frozen parameter a gradient (ops._HashFn, ops._MlpPairFn); ``unfreeze_field`` restores the flags.

        ``input_only_mlp`` (opt-in): the backward of the two frozen MLPs is ``lse_mlp_bwd_input`` -- d(input) and d(row_bias)
        alone -- instead of the training kernel with its weight-gradient products parked in a scratch.  The flag sits on this
        model's MLP modules and travels with every call (no other model sees it); no scratch is allocated, so such a model can be
        captured without an eager step first.  Ray, pose and embedding gradients agree with the default route up to the summation
        order of the per-ray bias gradient."""
        if self.__dict__.get("_frozen_flags") is not None:
            raise RuntimeError("freeze_field: the field is frozen already (unfreeze_field first)")
        emb = self.field.embedding_appearance
        keep = {id(p) for p in emb.parameters()} if (train_embedding and emb is not None) else set()
        flags, seen = [], set()
        for p in self._training_field_params():
            if id(p) in seen:
                continue
            seen.add(id(p))
            flags.append((p, p.requires_grad))
            if id(p) not in keep:
                p.requires_grad_(False)
        self.__dict__["_frozen_flags"] = flags
        for mlp in (self.field.mlp_base_mlp, self.field.mlp_head):
            mlp.input_only_bwd = bool(input_only_mlp)
        if self.field.mlp_head.params.is_cuda and not input_only_mlp:
            # where the recomputing MLP backward parks the weight-gradient products of a frozen network: allocated here, outside
            # any graph capture (ops.frozen_wgrad_scratch)
            for mlp in (self.field.mlp_base_mlp, self.field.mlp_head):
                if not mlp.params.requires_grad:
                    ops.frozen_wgrad_scratch(mlp.params)
        return [p for p, _ in flags if p.requires_grad]

    def unfreeze_field(self) -> None:
        """Put back the ``requires_grad`` flags ``freeze_field`` found."""
        flags = self.__dict__.get("_frozen_flags")
        if flags is None:
            return
        for p, was in flags:
            p.requires_grad_(was)
        for mlp in (self.field.mlp_base_mlp, self.field.mlp_head):
            mlp.input_only_bwd = False
        self.__dict__["_frozen_flags"] = None

    def init_test_params(self):   # R:lse_nerf/lsenerf.py:251-252
        self.field.embedding_appearance.init_test_params()

    # -- metrics (R:lse_nerf/lsenerf.py:378-388 over nerfstudio 0.3.2 NGPModel.get_metrics_dict) ------------------
    @staticmethod
    def psnr(preds: Tensor, target: Tensor) -> Tensor:
        """torchmetrics ``PeakSignalNoiseRatio(data_range=1.0)`` as NGPModel holds it: 10 log10(1 / mse)."""
        return 10.0 * torch.log10(1.0 / F.mse_loss(preds, target))

    def ssim(self, preds: Tensor, target: Tensor) -> Tensor:
        """torchmetrics ``structural_similarity_index_measure(preds, target)`` with its defaults (the reference's ``self.ssim``,
        R:lse_nerf/lsenerf.py:206) for [B,C,H,W] images, H and W >= 11: a 0-dim device tensor from one ``lse_image_metrics`` launch.
        Restated from torchmetrics' published algorithm, which is not a dependency here: that parity is unpinned."""
        return ops.image_metrics(preds.float().contiguous(), target.float().contiguous())[0]

    @property
    def lpips(self):
        """torchmetrics ``LearnedPerceptualImagePatchSimilarity(normalize=True)`` (R:lse_nerf/lsenerf.py:207), built on first use.
        Without torchmetrics a callable that raises ModuleNotFoundError naming the missing module (``.available`` is False)."""
        fn = self.__dict__.get("_lpips_fn")
        if fn is None:
            fn = self.__dict__["_lpips_fn"] = evaluation.make_lpips()
        return fn

    # -- evaluation (nerfstudio 0.3.2 Model.get_outputs_for_camera_ray_bundle; R:lse_nerf/lsenerf.py:477-530) ------------------
    @torch.no_grad()
    def get_outputs_for_camera_ray_bundle(self, camera_ray_bundle) -> Dict[str, Tensor]:
        """Render a whole camera bundle (tensors of any leading shape, usually [H, W]; this package's ``RayBundle`` or nerfstudio's)
        in chunks of ``config.eval_num_rays_per_chunk`` rays.  Returns [*leading shape, C] tensors: "rgb", "accumulation", "depth",
        "num_samples_per_ray" and the keys ``route_outputs`` adds in eval mode.  In eval mode with ``LSEField`` the chunks take the
        count-free route (no host synchronisation until one overflow check after the last chunk; ``lse_eval_composite`` writes the
        image rows); otherwise -- training mode, another field, a capacity above ``deferred_max_slots`` -- ``forward`` runs per
        chunk as in nerfstudio.  Both routes give the same values (lsenerf_amd.evaluation).  ``config.eval_early_stop_eps > 0``
        adds early ray termination to the count-free route (see the config field): "num_samples_per_ray" then counts the samples
        composited."""
        return evaluation.render_ray_bundle(self, camera_ray_bundle)

    @torch.no_grad()
    def get_image_metrics_and_images(self, outputs: Dict[str, Tensor], batch: Dict[str, Tensor]):
        """R:lse_nerf/lsenerf.py:477-530: ``(metrics, images)`` for a rendered [H, W, 3] image and ``batch["image"]`` (times
        ``batch["msk"]`` when present).  metrics: "psnr" (10 log10(1 / mse)) and "ssim" from one ``lse_image_metrics`` launch, plus
        "lpips" only where torchmetrics is importable -- the key is omitted otherwise.  images: "img" (ground truth beside the
        unmasked prediction), "err_map", grey "accumulation" and "depth" maps, and "ev_out" when rendered.  The reference's
        "overlay" (Canny edges of both images, ``evaluation.make_overlay``) is added with ``config.eval_overlay``."""
        return evaluation.image_metrics_and_images(self, outputs, batch)

    @torch.no_grad()
    def render_camera(self, cameras, camera_index: int, camera_opt_to_camera: Optional[Tensor] = None) -> Dict[str, Tensor]:
        """Every pixel of one camera of ``cameras`` (``EdCameras``) rendered through ``get_outputs_for_camera_ray_bundle``:
        [H, W, C] outputs.  ``camera_opt_to_camera``: a pose correction as ``EdCameras.generate_rays`` takes it."""
        return evaluation.render_camera(self, cameras, camera_index, camera_opt_to_camera)

    def evaluate_set(self, eval_set, events_only: bool = False, on_image=None, panels=None):
        """``(average, per_image)`` metrics over a device-resident ``eval_set.EvalSet`` -- the reference pipeline's
        ``get_average_eval_image_metrics`` without host work or a wait per image; ``events_only``: its ``update_evs_only_metric``
        (grey, scale-corrected psnr / ssim); ``panels``: an ``eval_set.PanelSet`` that receives every image's uint8 panel grid.  See
        ``lsenerf_amd.eval_set.evaluate_set``."""
        from . import eval_set as _eval_set
        return _eval_set.evaluate_set(self, eval_set, events_only=events_only, on_image=on_image, panels=panels)

    def extract_mesh(self, **kwargs):
        """Triangle mesh of the field's density isosurface with analytic normals (``lsenerf_amd.mesh.extract_mesh``: resolution,
        level, bounds, normals, colors, chunk).  Runs without gradients in eval mode and restores the model's mode."""
        from . import mesh as _mesh
        return _mesh.extract_mesh(self, **kwargs)

    def export_tsdf_mesh(self, views, **kwargs):
        """Triangle mesh of the surface ``views`` (an ``eval_set.EvalSet`` or ``(EdCameras, poses)``) see of the field: eval depth
        renders fused into a truncated signed distance volume, meshed without a surface against unobserved space
        (``lsenerf_amd.tsdf.export_tsdf_mesh``: image_indices, resolution, bounds, truncation, min_accumulation, carve, min_weight,
        colors, normals, views_per_launch, depth, max_depth_spread).  ``depth="median"`` fuses the depth at which the accumulated
        weight crosses one half instead of the expected depth.  Runs without gradients in eval mode and restores the model's mode and eval settings."""
        from . import tsdf as _tsdf
        return _tsdf.export_tsdf_mesh(self, views, **kwargs)

    def export_point_cloud(self, views, **kwargs):
        """Point cloud of what ``views`` (an ``eval_set.EvalSet`` or ray bundles) see of the field: unprojected eval renders, merged
        per voxel and filtered by neighbour support on request (``lsenerf_amd.pointcloud.export_point_cloud``: image_indices,
        min_accumulation, bounds, voxel_size, min_support, normals, colors, max_points, depth, max_depth_spread).
        ``depth="median"`` unprojects the depth at which the accumulated weight crosses one half.  Runs without gradients in eval mode and
        restores the model's mode and eval settings."""
        from . import pointcloud as _pointcloud
        return _pointcloud.export_point_cloud(self, views, **kwargs)

    def simulate_events(self, cameras, poses, times, threshold: float, **kwargs):
        """Events an ideal sensor sees of the field along ``poses`` at ``times``: ``(EventStream, ref_out, counts_total)``
        (``lsenerf_amd.events.simulate_events``: threshold_neg, window, cap_step, max_events, ref, sort, appearance_id,
        camera_index).  Runs without gradients in eval mode and restores the model's mode and eval settings."""
        from . import events as _events
        return _events.simulate_events(self, cameras, poses, times, threshold, **kwargs)

    def predict_event_frames(self, cameras, poses, threshold: float, **kwargs):
        """Signed event counts per frame of ``poses`` [F, S + 1, 3, 4], int32 [F, H, W] -- the quantity the recorded event frames
        hold (``lsenerf_amd.events.predict_event_frames``: threshold_neg, cap_step, times, appearance_id, camera_index)."""
        from . import events as _events
        return _events.predict_event_frames(self, cameras, poses, threshold, **kwargs)

    def _ngp_metrics_dict(self, outputs: Dict[str, Tensor], batch: Dict[str, Tensor]) -> Dict[str, Tensor]:
        image = batch["image"].to(outputs["rgb"].device)
        return {"psnr": self.psnr(outputs["rgb"], image), "num_samples_per_batch": outputs["num_samples_per_ray"].sum()}

    def get_metrics_dict(self, outputs, batch) -> Dict[str, object]:
        """{"psnr", "num_samples_per_batch"} for a plain rgb batch; for the multi-bundle step {"col": that dict of the colour
        bundle} (nothing is logged for the event bundles)."""
        if outputs.get("col_out") is None and outputs.get("prev_out") is None:
            return self._ngp_metrics_dict(outputs, batch)
        metrics = {}
        if outputs["col_out"] is not None:
            metrics["col"] = self._ngp_metrics_dict(outputs["col_out"], batch["col_batch"])
        return metrics

    def correct_evs_dim(self, inp):
        return self._run_module(self.rgb_to_one, inp) if self.config.ev_one_dim else inp

    def use_deferred_counts(self, num_rays: int) -> bool:
        """Whether a batch of ``num_rays`` rays takes the count-free sampler path (``deferred_counts`` and the slot budget)."""
        cfg = self.config
        return bool(self.deferred_counts and cfg.render_step_size and cfg.render_step_size > 0 and
                    num_rays * self.occupancy_grid._cap_per_ray(cfg.near_plane, cfg.far_plane, cfg.render_step_size,
                                                                cfg.cone_angle) <= self.deferred_max_slots)

    # -- R:lse_nerf/lsenerf.py:265-326 ----------------------------------------------------------------
    def forward(self, ray_bundle: RayBundle, **kwargs):
        if self.collider is not None:
            ray_bundle = self.collider(ray_bundle)
        return self.get_outputs(ray_bundle, **kwargs)

    def exec_get_outputs(self, ray_bundle: RayBundle, jitter: Optional[Tensor] = None, premarched=None):
        assert self.field is not None
        num_rays = len(ray_bundle)
        cfg = self.config
        if self.training and self.sampler._packed_field is self.field and self.use_deferred_counts(num_rays):
            # no sample count visits the host: capacity-extent arrays + a device-side count handed to every per-sample kernel
            ri, ts, te, packed, n_dev = self.sampler.sample_packed(
                ray_bundle, near_plane=cfg.near_plane, far_plane=cfg.far_plane, render_step_size=cfg.render_step_size,
                alpha_thre=cfg.alpha_thre, cone_angle=cfg.cone_angle, jitter=jitter, premarched=premarched)
            return self.render_packed(ray_bundle, ri, ts, te, packed, n_dev=n_dev)
        if premarched is not None:
            raise ValueError("premarched samples need the count-free packed path (training, LSEField, use_deferred_counts)")
        ray_samples, ray_indices = self.sampler(ray_bundle=ray_bundle, near_plane=cfg.near_plane,
                                                far_plane=cfg.far_plane, render_step_size=cfg.render_step_size,
                                                alpha_thre=cfg.alpha_thre, cone_angle=cfg.cone_angle, jitter=jitter)
        # the per-sample metadata gathers of R:lse_nerf/lsenerf.py:292-296 are skipped: appearance ids stay per ray
        return self.render_packed(ray_bundle, ray_samples.ray_indices, ray_samples.frustums.starts[..., 0],
                                  ray_samples.frustums.ends[..., 0], ray_samples.packed_info)

    def render_packed(self, ray_bundle: RayBundle, ray_idx: Tensor, t_starts: Tensor, t_ends: Tensor,
                      packed_info: Tensor, n_dev: Optional[Tensor] = None) -> Dict[str, Tensor]:
        """R:lse_nerf/lsenerf.py:297-326 on packed samples: field -> weights -> rgb / depth / accumulation.
        ``n_dev``: device-side sample count when the packed arrays have capacity extent (deferred sampling)."""
        num_rays = len(ray_bundle)
        fld = self.field
        rays_o, rays_d = ray_bundle.origins.contiguous(), ray_bundle.directions.contiguous()
        grid = getattr(fld, "mlp_base_grid", None)
        if grid is not None and hasattr(grid, "dense_steps"):      # regime hint for the hash backward's path thresholds
            grid.dense_steps = not (self.config.cone_angle and self.config.cone_angle > 0)
        table, eidx = fld._ray_emb(ray_bundle.metadata, ray_bundle.camera_indices, num_rays, rays_o.device)
        # density_packed -> rgb_packed on the same samples (the two MLP forwards are one launch where the shapes allow)
        feats = {} if self.eval_normals_on() else None
        sigma, _, _, rgb16 = fld.density_rgb_packed(rays_o, rays_d, ray_idx, t_starts, t_ends, packed_info, eidx, table, n_dev,
                                                    features_out=feats)
        linear = isinstance(self.renderer_rgb, LinearRenderer)
        if not (self.training or linear):
            rgb16 = torch.nan_to_num(rgb16)
        rgb, acc, depth, weights = ops.volume_render_depth(t_starts, t_ends, sigma, rgb16, packed_info)
        bg = self.config.background_color
        if bg not in ("random", "last_sample"):
            rgb = rgb + {"black": 0.0, "white": 1.0}[bg] * (1.0 - acc[:, None])
        if not (self.training or linear):
            rgb = torch.clamp(rgb, 0.0, 1.0)
        out = {"rgb": rgb, "accumulation": acc[:, None], "depth": depth[:, None], "num_samples_per_ray": packed_info[:, 1]}
        if self.distortion_on():
            out["distortion"] = ops.distortion_loss(t_starts, t_ends, sigma, weights, packed_info, self.config.distortion_t_scale)[:, None]
        if feats is not None:
            out["normals"] = torch.empty((num_rays, 3), dtype=torch.float32, device=rays_o.device)
            self.composite_normals(feats["x01"], feats["y"], t_starts, t_ends, sigma, packed_info, rays_o, rays_d, out["normals"], n_dev)
        return out

    def distortion_on(self) -> bool:
        """Whether this render carries "distortion": ``config.distortion_loss_mult`` > 0, training mode, and the field not frozen."""
        return self.config.distortion_loss_mult > 0 and self.training and self.__dict__.get("_frozen_flags") is None

    def eval_normals_on(self) -> bool:
        """Whether this render carries "normals": ``config.eval_normals`` is on and the model is in eval mode."""
        return self.config.eval_normals != "off" and not self.training

    @torch.no_grad()
    def composite_normals(self, x01: Tensor, y: Tensor, t_starts: Tensor, t_ends: Tensor, sigma: Tensor, packed_info: Tensor,
                          rays_o: Tensor, rays_d: Tensor, out: Tensor, n_dev: Optional[Tensor] = None) -> None:
        """The normals pass of one chunk, shared by ``render_packed`` and the count-free eval route: ``LSEField.normals_packed`` on
        the chunk's samples, then ``lse_eval_composite_normals`` with the rendered ``sigma`` into ``out [n,3]``."""
        fld = self.field
        d_x01 = fld.normals_packed(x01, y, n_dev)
        contraction = fld._contraction == "inf"
        ops.eval_composite_normals(t_starts, t_ends, sigma.detach(), d_x01, packed_info, out,
                                   world=self.config.eval_normals == "world", renormalize=True, rays_o=rays_o, rays_d=rays_d,
                                   contraction=contraction, aabb6=None if contraction else fld._aabb_list())

    # -- output routing and losses (what R:lse_nerf/lsenerf.py:329-439 computes) ---------------------------------
    # One description of the routing (``_plan``) drives both implementations: ``route_outputs`` / ``get_loss_dict`` build
    # the reference's output dictionaries with torch ops (evaluation, logging, any mapper module), ``fused_loss_dict``
    # hands the same plan to the O(R) epilogue kernel pair (lse_loss_epilogue_fwd / _bwd) for the training step.
    def _plan(self) -> Dict[str, object]:
        cfg = self.config
        mode = cfg.map_mode if (cfg.use_mapping or cfg.map_mode == "rgb_evs") else None
        # a map_mode that names none of the three routes -- the reference's own default spelling "ev_rgb" is one
        # (R:lse_nerf/lsenerf.py:80) -- falls through every branch of the reference's get_outputs (:335-363): no mapper runs and
        # no "ev_out" exists, so an rgb-only batch trains and an event batch fails with the reference's KeyError('ev_out') in
        # get_loss_dict (:432-433).  Same here: such a plan takes the torch route (``unrouted``), never the fused epilogue.
        unrouted = mode is not None and mode not in ("co_map", "evs_rgb", "rgb_evs")
        if unrouted:
            mode = None
        one_dim = getattr(self, "rgb_to_one", None) if cfg.ev_one_dim else None
        if cfg.use_mapping:        # the event loss reads "ev_out"
            ev_mapper = {"co_map": self.evs_mapper, "evs_rgb": None, "rgb_evs": getattr(self, "rgb_mapper", None)}.get(cfg.map_mode)
            ev_one_dim = one_dim
        else:                      # ... otherwise the routed "rgb"
            ev_mapper, ev_one_dim = None, None
        return {"mode": mode, "rgb_mapper": getattr(self, "rgb_mapper", None) if mode in ("evs_rgb", "co_map") else None,
                "ev_key": "ev_out" if cfg.use_mapping else "rgb", "ev_mapper": ev_mapper, "ev_one_dim": ev_one_dim,
                "deblur_group": 4 if cfg.rgb_loss_type == "deblur" else 1, "unrouted": unrouted}

    def get_outputs(self, ray_bundle: RayBundle, ev_out=False, jitter: Optional[Tensor] = None, **kwargs):
        return self.route_outputs(self.exec_get_outputs(ray_bundle, jitter=jitter), ray_bundle, ev_out=ev_out, **kwargs)

    @staticmethod
    def _run_module(module, *args, **kwargs):
        """``module(*args)`` with its parameters' gradients accumulated straight into their preallocated buffers
        (ops.direct_grad_params): on the torch route of the loss too, no AccumulateGrad node of a model parameter receives a
        gradient -- which is what keeps a captured step indifferent to autograd graphs of earlier eager steps (graph.py)."""
        direct = ops.direct_grad_params(module) if isinstance(module, nn.Module) else None
        if direct is None:
            return module(*args, **kwargs)
        return torch.func.functional_call(module, direct, args, kwargs)

    def route_outputs(self, out_dict: Dict[str, Tensor], ray_bundle: RayBundle, ev_out=False, **kwargs):
        """Rendered radiance -> the reference's output keys: "rgb" in display space, "linear" / "ev_linear" / "ev_out" on
        the event side, by map_mode ("rgb_evs": render -> rgb -> events; "evs_rgb": render -> events -> rgb; "co_map":
        one linear render feeding an rgb mapper and an event mapper)."""
        plan, training = self._plan(), self.training
        radiance = out_dict["rgb"]
        linear = radiance.clamp_min(1e-5)
        events_wanted = ev_out or not training
        routed = dict(out_dict)
        rgb_mapper = lambda *a, **k: self._run_module(self.rgb_mapper, *a, **k)
        evs_mapper = lambda *a, **k: self._run_module(self.evs_mapper, *a, **k)
        correct_evs_dim = self.correct_evs_dim
        if plan["mode"] == "rgb_evs":
            if events_wanted:
                routed["ev_out"] = rgb_mapper(correct_evs_dim(linear))
                routed["linear"] = format_linear(routed["ev_out"])
        elif plan["mode"] == "evs_rgb":
            routed.update(ev_out=correct_evs_dim(linear), linear=linear, rgb=rgb_mapper(linear).to(linear))
        elif plan["mode"] == "co_map":
            routed["rgb"] = rgb_mapper(linear)
            if events_wanted:
                ev_linear = correct_evs_dim(linear)
                routed.update(linear=linear, ev_linear=ev_linear,
                              ev_out=evs_mapper(ev_linear, raybd1=ray_bundle, **kwargs))
        rgb = routed["rgb"]
        if training and plan["deblur_group"] > 1 and rgb.shape[-1] == 3 and rgb.shape[0] % plan["deblur_group"] == 0:
            rgb = rgb.reshape(-1, plan["deblur_group"], 3).mean(dim=1)          # the virtual cameras of one pixel
        routed["rgb"] = rgb.clamp_min(1e-5) if training else rgb.clamp(0, 1)
        return routed

    # -- losses ------------------------------------------------------------------------------------------
    @staticmethod
    def _log_intensity_change(prev_rad: Tensor, next_rad: Tensor) -> Tensor:
        if prev_rad.shape[-1] != 1:
            prev_rad, next_rad = to_gray(prev_rad), to_gray(next_rad)
        return torch.log(next_rad + EPS) - torch.log(prev_rad + EPS)

    def log_loss(self, evs, prev_rad, next_rad, evs_batch: dict):
        return self.rgb_loss(self._log_intensity_change(prev_rad, next_rad), evs)

    def mse_loss(self, rgb_gt, rgb_pred, rgb_out_dic=None):
        return self.rgb_loss(rgb_gt, rgb_pred)

    def enerf_norm_loss(self, evs, prev_rad, next_rad, evs_batch: dict):
        delta = self._log_intensity_change(prev_rad, next_rad)
        delta = delta / (torch.linalg.norm(delta, dim=0, keepdim=True) + EPS)
        with torch.no_grad():
            evs = evs / evs_batch["e_thresh"]
            evs = evs / (torch.linalg.norm(evs, dim=0, keepdim=True) + EPS)
        return self.rgb_loss(delta, evs)

    def get_loss_dict(self, outputs, batch, metrics_dict=None):
        """``outputs``: {"col_out", "prev_out", "next_out"} routed dictionaries (or a plain {"rgb"} for an rgb-only batch)."""
        if batch.get("col_batch") is None and batch.get("evs_batch") is None:
            return {"rgb_loss": self.rgb_loss(batch["image"], outputs["rgb"])}
        losses = {}
        if outputs["col_out"] is not None:
            losses["rgb_loss"] = self.rgb_loss_fn(batch["col_batch"]["image"], outputs["col_out"]["rgb"], outputs["col_out"])
        if outputs["prev_out"] is not None:
            key = self._plan()["ev_key"]
            prev_in, next_in = outputs["prev_out"][key], outputs["next_out"][key]
            evs = batch["evs_batch"]["image"]
            if prev_in.shape[-1] != 1:
                evs = torch.cat([evs] * 3, dim=-1)
            losses["event_loss"] = self.config.evs_loss_weight * self.event_loss(evs, prev_in, next_in, batch["evs_batch"])
        return losses

    # -- the reference's training step (R:lse_nerf/lse_pipeline.py:110-145) as ONE packed pass ----------------------------
    def train_step_bundles(self, col_bundle: Optional[RayBundle], prev_bundle: Optional[RayBundle],
                           next_bundle: Optional[RayBundle], batch: Dict[str, object], jitter: Optional[Tensor] = None,
                           with_metrics: bool = False, premarched=None, alias_blocks: bool = False):
        """``LSENeRFPipeline.get_train_loss_dict`` for bundles the data manager has already produced: returns
        ``(out_dict, loss_dict, metrics_dict)`` with ``out_dict = {"col_out", "prev_out", "next_out"}``.

        The reference runs up to three model forwards per step -- colour bundle, previous-event bundle, next-event bundle
        (2316 / 597 / 597 rays at its default batch, R:lse_nerf/lse_datamanager.py:135-144) -- each with its own sampler call,
        host synchronisations, field pass, renderer and, in backward, its own hash-table scatter.  Rays are independent, so the
        three bundles are rendered here as ONE packed batch: one marcher launch, one visibility pre-pass, one field pass, one
        volume-rendering kernel, one loss epilogue, ONE hash backward; per-bundle outputs are row slices of the packed
        result.  Every ray gets exactly the samples and values it gets in a pass of its own (``jitter``: one stratified
        offset per ray, colour rays first, for callers that need the draw reproduced); only the order in which gradient
        contributions are summed differs.  ``premarched``: the result of ``premarch_bundles`` for these bundles (the ray marcher
        run ahead of the step; ``jitter`` was applied there).  ``with_metrics``: also route the colour render and report NGPModel's psnr /
        num_samples_per_batch (R:lse_nerf/lsenerf.py:378-388) -- a handful of O(R) torch ops outside the fused epilogue.
        ``alias_blocks``: the bundles are the caller's own row blocks of one buffer per field and may be joined without a copy
        (``RayBundle.cat``; lsenerf_amd.graph's static inputs)."""
        assert self.training, "train_step_bundles is the training step; use forward() / get_outputs() for evaluation"
        names = ("col_out", "prev_out", "next_out")
        given = [(k, b) for k, b in zip(names, (col_bundle, prev_bundle, next_bundle)) if b is not None and len(b) > 0]
        assert given, "no rays in this step"
        if (prev_bundle is not None and len(prev_bundle) > 0) != (next_bundle is not None and len(next_bundle) > 0):
            raise ValueError("previous and next event bundles come in pairs")
        rb = RayBundle.cat([b for _, b in given], alias_blocks=alias_blocks)
        if self.collider is not None:
            rb = self.collider(rb)
        raw = self.exec_get_outputs(rb, jitter=jitter, premarched=premarched)
        out_dict: Dict[str, Optional[Dict[str, Tensor]]] = {k: None for k in names}
        lo = 0
        for k, b in given:
            hi = lo + len(b)
            out_dict[k] = {key: val[lo:hi] for key, val in raw.items()}
            lo = hi
        loss_dict = self.fused_loss_dict(out_dict, batch, packed_rgb=raw["rgb"])
        if "distortion" in raw:        # (distortion_on: one term over all rays of the packed pass, whichever route the other two took)
            # mult * mean, as a sum: its backward hands lse_distortion_bwd ONE broadcast scalar (g_stride 0), no [R] gradient is formed
            loss_dict["distortion_loss"] = raw["distortion"].sum() * (self.config.distortion_loss_mult / raw["distortion"].shape[0])
        metrics_dict: Dict[str, object] = {}
        if with_metrics and out_dict["col_out"] is not None:
            with torch.no_grad():
                routed = self.route_outputs({k: v.detach() for k, v in out_dict["col_out"].items()}, col_bundle)
                md = self.get_metrics_dict({"col_out": routed, "prev_out": out_dict["prev_out"], "next_out": out_dict["next_out"]},
                                           batch)
            metrics_dict = {f"{k1}_{k2}": v for k1, d in md.items() for k2, v in d.items()}   # flatten_metrics_dict (:100-107)
        return out_dict, loss_dict, metrics_dict

    def premarch_bundles(self, col_bundle: Optional[RayBundle], prev_bundle: Optional[RayBundle],
                         next_bundle: Optional[RayBundle], jitter: Optional[Tensor] = None, out=None,
                         alias_blocks: bool = False):
        """The ray marcher of ``train_step_bundles`` for these bundles, launched now (on torch's current stream): it reads the rays
        and the occupancy grid only, so the NEXT step's marcher can run behind the current step's backward pass.  The result is
        valid while ``occupancy_grid.grid_version`` equals its ``grid_version``."""
        cfg = self.config
        given = [b for b in (col_bundle, prev_bundle, next_bundle) if b is not None and len(b) > 0]
        rb = RayBundle.cat(given, alias_blocks=alias_blocks)
        if self.collider is not None:
            rb = self.collider(rb)
        return self.sampler.premarch(rb, near_plane=cfg.near_plane, far_plane=cfg.far_plane, render_step_size=cfg.render_step_size,
                                     cone_angle=cfg.cone_angle, jitter=jitter, out=out)

    # -- fused training epilogue -----------------------------------------------------------------------------
    def _epilogue_desc(self) -> Optional[Tuple[tuple, Optional[Tensor], Optional[Tensor], Optional[Tensor], tuple, tuple]]:
        """(descriptor fields, pow_rgb, pow_evs, w31, mlp_rgb, mlp_evs) for ops.loss_epilogue, or None when the configuration needs
        the torch route (an unrouted map_mode, the event loss reading a deblur-averaged "rgb", or an MLP mapper on a channel count
        its first nn.Linear does not take -- the reference raises there, and so does the torch route).  ``mlp_*``: the
        eight parameters of an MLP mapper on that side in module order (R:lse_nerf/intensity_mappers.py:28-62), () otherwise."""
        from . import _lib
        cfg, plan = self.config, self._plan()
        kinds = {IdentityMapper: _lib.LSE_MAP_IDENTITY, GT_Mapper: _lib.LSE_MAP_GT, Powpow: _lib.LSE_MAP_POWPOW,
                 MLP_Mapper: _lib.LSE_MAP_MLP, RGB_MLP_Mapper: _lib.LSE_MAP_RGB_MLP, type(None): _lib.LSE_MAP_IDENTITY}
        ev_loss = {"log_loss": _lib.LSE_EVLOSS_LOG, "enerf_norm_loss": _lib.LSE_EVLOSS_ENERF_NORM}.get(cfg.event_loss_type.lower())
        if plan["unrouted"] or ev_loss is None or type(plan["rgb_mapper"]) not in kinds \
                or type(plan["ev_mapper"]) not in kinds or (plan["ev_key"] == "rgb" and plan["deblur_group"] > 1):
            return None
        od = plan["ev_one_dim"]
        one_dim = _lib.LSE_ONE_DIM_NONE if od is None else (_lib.LSE_ONE_DIM_LEARNED if isinstance(od, ThreeToOne) else _lib.LSE_ONE_DIM_GRAY)
        rgb_kind, evs_kind = kinds[type(plan["rgb_mapper"])], kinds[type(plan["ev_mapper"])]
        one_channel = one_dim != _lib.LSE_ONE_DIM_NONE
        if rgb_kind == _lib.LSE_MAP_MLP or (evs_kind == _lib.LSE_MAP_MLP and not one_channel) \
                or (evs_kind == _lib.LSE_MAP_RGB_MLP and one_channel):
            return None           # nn.Linear(1, 16) on three channels / nn.Linear(3, 16) on one
        fields = (int(plan["rgb_mapper"] is not None), rgb_kind, evs_kind, one_dim, plan["deblur_group"], float(cfg.evs_loss_weight),
                  ev_loss)
        coeff = lambda m: m.pow_coeff if isinstance(m, Powpow) else None
        layers = lambda m: tuple(p for layer in m.mlp.layers for p in (layer.weight, layer.bias)) \
            if isinstance(m, (MLP_Mapper, RGB_MLP_Mapper)) else ()
        return (fields, coeff(plan["rgb_mapper"]), coeff(plan["ev_mapper"]), (od.weights if isinstance(od, ThreeToOne) else None),
                layers(plan["rgb_mapper"]), layers(plan["ev_mapper"]))

    @staticmethod
    def _e_thresh(batch, fields):
        """evs_batch["e_thresh"] when the event loss divides by it (enerf_norm_loss, R:lse_nerf/lsenerf.py:416: a KeyError when the
        batch does not carry it, like the reference's)."""
        from . import _lib
        return batch["evs_batch"]["e_thresh"] if fields[6] == _lib.LSE_EVLOSS_ENERF_NORM else None

    def fused_loss_dict(self, raw_outputs: Dict[str, Optional[Dict[str, Tensor]]], batch,
                        packed_rgb: Optional[Tensor] = None) -> Dict[str, Tensor]:
        """Training losses straight from the three bundles' ``exec_get_outputs`` results ({"col_out", "prev_out", "next_out"},
        each the raw render or None): routing, mappers, deblur mean and both MSEs run in one forward and one backward launch.
        Same values as ``get_loss_dict`` over ``route_outputs`` (tests/test_gpu_configs.py).
        ``packed_rgb``: the render of ONE packed pass whose row blocks [colour | previous | next] the three entries of
        ``raw_outputs`` are (train_step_bundles): the epilogue then works on that buffer directly and its backward returns one
        gradient buffer instead of three slices to be scattered back."""
        assert self.training, "the fused epilogue is the training-mode routing"
        desc = self._epilogue_desc()
        col, prev, nxt = (raw_outputs.get(k) for k in ("col_out", "prev_out", "next_out"))
        if desc is not None and packed_rgb is not None:
            fields, pow_rgb, pow_evs, w31, mlp_rgb, mlp_evs = desc
            n_col = col["rgb"].shape[0] if col is not None else 0
            n_ev = prev["rgb"].shape[0] if prev is not None else 0
            rgb_loss, event_loss = ops.loss_epilogue_packed(
                fields, packed_rgb, n_col, n_ev, batch["col_batch"]["image"] if col is not None else None,
                batch["evs_batch"]["image"] if prev is not None else None, pow_rgb, pow_evs, w31, mlp_rgb, mlp_evs,
                e_thresh=self._e_thresh(batch, fields) if prev is not None else None)
            losses = {}
            if col is not None:
                losses["rgb_loss"] = rgb_loss
            if prev is not None:
                losses["event_loss"] = event_loss
            return losses
        if desc is None:
            routed = {k: (self.route_outputs(v, None, ev_out=(k != "col_out")) if v is not None else None)
                      for k, v in (("col_out", col), ("prev_out", prev), ("next_out", nxt))}
            return self.get_loss_dict(routed, batch)
        fields, pow_rgb, pow_evs, w31, mlp_rgb, mlp_evs = desc
        rgb_loss, event_loss = ops.loss_epilogue(
            fields, col["rgb"] if col is not None else None, batch["col_batch"]["image"] if col is not None else None,
            prev["rgb"] if prev is not None else None, nxt["rgb"] if nxt is not None else None,
            batch["evs_batch"]["image"] if prev is not None else None, pow_rgb, pow_evs, w31, mlp_rgb, mlp_evs,
            e_thresh=self._e_thresh(batch, fields) if prev is not None else None)
        losses = {}
        if col is not None:
            losses["rgb_loss"] = rgb_loss
        if prev is not None:
            losses["event_loss"] = event_loss
        return losses
