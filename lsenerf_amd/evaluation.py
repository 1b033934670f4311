"""Whole-image evaluation: the ``Model`` surface the reference's pipeline calls at eval time.

* ``render_ray_bundle`` -- nerfstudio 0.3.2 ``Model.get_outputs_for_camera_ray_bundle`` (chunks of ``eval_num_rays_per_chunk`` rays
  through ``forward``, outputs concatenated and viewed as ``[*leading shape, C]``).  In eval mode with ``LSEField`` every chunk takes
  the count-free route instead: deferred sampling (no sample count read back), ``density_rgb_packed`` with the
  device-side count, and ``lse_eval_composite`` writing the chunk's rows of the image buffers directly -- no host synchronisation
  inside the loop, no per-sample ``RaySamples`` gathers, no autograd Functions.  Its values are those of the ``forward`` loop bit for
  bit (the mapper keys, formed once over the whole image, to GEMM rounding).  With ``config.eval_early_stop_eps > 0`` the count-free
  route composites each chunk in segments of the ray and stops evaluating the field on rays that have become opaque
  (``_render_early_stop``; opt-in, still without a host synchronisation inside the loops).
* ``image_metrics_and_images`` -- R:lse_nerf/lsenerf.py:477-530 restated: psnr / ssim from one ``lse_image_metrics`` launch, lpips
  when torchmetrics is importable, and the image dictionary ("overlay" with ``config.eval_overlay``: Canny edges on the device).
* ``make_overlay`` -- R:lse_nerf/lsenerf.py:462-475: where the rendered edges lie against the true ones (``ops.canny_edges``).
* ``make_lpips`` -- torchmetrics' ``LearnedPerceptualImagePatchSimilarity(normalize=True)``, or a callable that names what is missing.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor

from . import ops
from .field import LSEField
from .rays import RayBundle
from .renderer import LinearRenderer

_BUNDLE_FIELDS = ("origins", "directions", "pixel_area", "camera_indices", "nears", "fars", "times")


def _flatten_bundle(bundle, device=None) -> RayBundle:
    """This package's ``RayBundle`` with every tensor of ``bundle`` (any object with nerfstudio's attribute names) as ``[R, ...]``
    rows, row-major over its leading shape (nerfstudio's ``get_row_major_sliced_ray_bundle`` order)."""
    lead = tuple(bundle.origins.shape[:-1])
    n = 1
    for s in lead:
        n *= int(s)

    def flat(t):
        if t is None:
            return None
        t = t.reshape(n, *t.shape[len(lead):])
        return t.to(device) if device is not None else t     # (a bundle built on the host goes to the model's device)
    meta = getattr(bundle, "metadata", None) or {}
    return RayBundle(**{k: flat(getattr(bundle, k, None)) for k in _BUNDLE_FIELDS},
                     metadata={k: flat(v) for k, v in meta.items() if torch.is_tensor(v)})


def _slice(rb: RayBundle, lo: int, hi: int) -> RayBundle:
    part = lambda t: t[lo:hi] if t is not None else None
    return RayBundle(**{k: part(getattr(rb, k)) for k in _BUNDLE_FIELDS}, metadata={k: v[lo:hi] for k, v in rb.metadata.items()})


def uses_count_free_route(model, num_rays: int) -> bool:
    """Whether ``render_ray_bundle`` takes the count-free route for an image of ``num_rays`` rays (else the ``forward`` loop)."""
    fld = model.field
    if model.training or not isinstance(fld, LSEField) or model.sampler._packed_field is not fld or model.collider is not None:
        return False
    base = fld.mlp_base_mlp
    if base.in_pad != base.in_dim:          # the small-grid base MLP has no device-side count (LSEField._base_mlp)
        return False
    return model.use_deferred_counts(min(int(model.config.eval_num_rays_per_chunk), max(num_rays, 1)))


def _render_loop(model, rb: RayBundle, chunk: int) -> Dict[str, Tensor]:
    """nerfstudio's loop: ``forward`` per chunk, tensor outputs concatenated."""
    lists: Dict[str, list] = {}
    for lo in range(0, len(rb), chunk):
        out = model.forward(ray_bundle=_slice(rb, lo, min(len(rb), lo + chunk)))
        for k, v in out.items():
            if torch.is_tensor(v):
                lists.setdefault(k, []).append(v)
    return {k: torch.cat(v) for k, v in lists.items()}


def depth_quantile_settings(config) -> Tuple[Tuple[float, ...], bool]:
    """(quantiles, interpolate) of ``config``, validated: ValueError unless the quantiles are at most 4 values strictly inside
    (0, 1) in ascending order and -- with ``eval_early_stop_eps > 0`` -- every ``1 - q >= eps`` (a ray may be stopped once its
    transmittance is below eps: a quantile beyond that could lie behind the stop).  Pure host code: nothing touches a device."""
    raw = config.eval_depth_quantiles
    try:
        qs = tuple(float(q) for q in raw)
    except TypeError:
        raise ValueError(f"eval_depth_quantiles must be a tuple of floats, got {raw!r}") from None
    if len(qs) > 4:
        raise ValueError(f"eval_depth_quantiles takes at most 4 values, got {len(qs)}")
    if any(not (0.0 < q < 1.0) for q in qs):          # (a NaN fails this too)
        raise ValueError(f"eval_depth_quantiles must lie strictly inside (0, 1), got {qs}")
    if any(b <= a for a, b in zip(qs[:-1], qs[1:])):
        raise ValueError(f"eval_depth_quantiles must be ascending, got {qs}")
    eps = float(config.eval_early_stop_eps)
    if qs and eps > 0.0 and not (1.0 - qs[-1] >= eps):
        raise ValueError(f"eval_depth_quantiles {qs} with eval_early_stop_eps = {eps}: every quantile needs 1 - q >= eps, or a ray "
                         f"may be stopped before the crossing")
    return qs, bool(config.eval_depth_interpolate)


class _DepthQuantiles:
    """The quantile-depth outputs of one image on the count-free routes: the buffers, and the one extra launch per chunk
    (``full``) or per segment (``segment``, after ``begin`` has reset the chunk's state).  ``select`` = (column,
    max_spread or None) adds "depth_selected" (``ops.eval_depth_quantiles``' ``depth_sel``) for the exporters."""

    def __init__(self, qs, interpolate: bool, select, R: int, n: int, dev, segmented: bool):
        self.taus = [ops.depth_tau(q) for q in qs]
        self.interpolate = interpolate
        self.sel, self.max_spread = (0, None) if select is None else (int(select[0]), select[1])
        if select is not None and not 0 <= self.sel < len(qs):
            raise ValueError(f"depth_select: column {self.sel} of {len(qs)} quantiles")
        # the segment kernel leaves a ray without samples alone: there the image starts as what such a ray gets (0 / 0 / NaN), filled
        # once per image; the one-launch kernel writes every ray
        new = (lambda shape, dtype, fill: torch.full(shape, fill, dtype=dtype, device=dev)) if segmented else \
            (lambda shape, dtype, fill: torch.empty(shape, dtype=dtype, device=dev))
        self.depth_q = new((R, len(qs)), torch.float32, 0.0)
        self.reached = new((R,), torch.uint8, 0)
        self.selected = new((R,), torch.float32, float("nan")) if select is not None else None
        self.state = torch.empty((n, 2), dtype=torch.float32, device=dev) if segmented else None      # carry and found mask

    def _rows(self, lo: int, hi: int):
        return self.depth_q[lo:hi], self.reached[lo:hi], None if self.selected is None else self.selected[lo:hi]

    def _kw(self):
        return dict(interpolate=self.interpolate, sel=self.sel, max_spread=self.max_spread)

    def full(self, ts, te, sigma, packed, lo: int, hi: int) -> None:
        ops.eval_depth_quantiles(ts, te, sigma, packed, self.taus, *self._rows(lo, hi), **self._kw())

    def begin(self, lo: int, hi: int) -> None:
        self.state[:hi - lo].zero_()

    def segment(self, ts, te, sigma, packed, lo: int, hi: int) -> None:
        ops.eval_depth_quantiles_segment(ts, te, sigma, packed, self.taus, self.state[:hi - lo], *self._rows(lo, hi), **self._kw())

    def outputs(self) -> Dict[str, Tensor]:
        out = {"depth_quantiles": self.depth_q, "depth_reached": self.reached[:, None]}
        if self.selected is not None:
            out["depth_selected"] = self.selected[:, None]
        return out


def _depth_quantiles_of(model, depth_select, R: int, n: int, dev, segmented: bool) -> Optional[_DepthQuantiles]:
    qs, interpolate = depth_quantile_settings(model.config)
    if not qs or model.training:
        if depth_select is not None:
            raise ValueError("depth_select needs eval_depth_quantiles and eval mode")
        return None
    return _DepthQuantiles(qs, interpolate, depth_select, R, n, dev, segmented)


def _render_count_free(model, rb: RayBundle, chunk: int, check_overflow: bool = True, depth_select=None) -> Dict[str, Tensor]:
    cfg, fld = model.config, model.field
    R = len(rb)
    dev = rb.origins.device
    quant = _depth_quantiles_of(model, depth_select, R, min(chunk, R), dev, segmented=False)
    rgb = torch.empty((R, 3), dtype=torch.float32, device=dev)
    acc = torch.empty(R, dtype=torch.float32, device=dev)
    depth = torch.empty(R, dtype=torch.float32, device=dev)
    nsamples = torch.empty(R, dtype=torch.int64, device=dev)
    ws = torch.empty(3 * min(chunk, R), dtype=torch.float32, device=dev)
    normals = torch.empty((R, 3), dtype=torch.float32, device=dev) if model.eval_normals_on() else None
    feats = {} if normals is not None else None
    linear = isinstance(model.renderer_rgb, LinearRenderer)
    bg = cfg.background_color
    background = None if bg in ("random", "last_sample") else {"black": 0.0, "white": 1.0}[bg]
    fld._prepass = None                   # pre-pass features belong to a training step, never to these samples
    for lo in range(0, R, chunk):
        hi = min(R, lo + chunk)
        part = _slice(rb, lo, hi)
        ri, ts, te, packed, n_dev = model.sampler.sample_packed(
            part, near_plane=cfg.near_plane, far_plane=cfg.far_plane, render_step_size=cfg.render_step_size,
            alpha_thre=cfg.alpha_thre, cone_angle=cfg.cone_angle)
        rays_o, rays_d = part.origins.contiguous(), part.directions.contiguous()
        table, eidx = fld._eval_emb(hi - lo, dev) if fld.embedding_appearance is not None else (None, None)
        sigma, _, _, head = fld.density_rgb_packed(rays_o, rays_d, ri, ts, te, packed, eidx, table, n_dev, features_out=feats)
        ops.eval_composite(ts, te, sigma, head, packed, rgb[lo:hi], acc[lo:hi], depth[lo:hi], nsamples[lo:hi],
                           nan_to_num=not linear, background=background, clamp=not linear, workspace=ws)
        if quant is not None:
            quant.full(ts, te, sigma, packed, lo, hi)
        if normals is not None:
            model.composite_normals(feats["x01"], feats["y"], ts, te, sigma, packed, rays_o, rays_d, normals[lo:hi], n_dev)
    if check_overflow:
        model.occupancy_grid.check_deferred_overflow()      # the one read-back: a truncated ray raises here
    raw = {"rgb": rgb, "accumulation": acc[:, None], "depth": depth[:, None], "num_samples_per_ray": nsamples}
    if normals is not None:
        raw["normals"] = normals
    if quant is not None:
        raw.update(quant.outputs())
    return {k: v for k, v in model.route_outputs(raw, rb).items() if torch.is_tensor(v)}


def segment_schedule(cap: int, base: int) -> List[Tuple[int, int]]:
    """The segments ``[(offset, length), ...]`` the early-stop route cuts a ray of at most ``cap`` samples into: lengths ``base``,
    ``base``, ``2 base``, ``4 base``, ... with the last one cut so that they sum to ``cap``.  ``base`` is a positive multiple of 64,
    so every offset is one too: sample k of a ray meets lane k mod 64 of the compositing kernels whichever segment it falls into.
    Short segments first (most rays of a trained scene are opaque within a few dozen samples), doubling ones behind them (the
    number of segments, each a fixed set of launches, grows with log cap)."""
    cap, base = int(cap), int(base)
    if cap < 1:
        raise ValueError(f"segment_schedule: cap must be positive, got {cap}")
    if base <= 0 or base % 64 != 0:
        raise ValueError(f"segment_schedule: the base segment length must be a positive multiple of 64, got {base}")
    out, off, length = [], 0, base
    while off < cap:
        out.append((off, min(length, cap - off)))
        off += out[-1][1]
        if len(out) >= 2:
            length *= 2
    return out


def early_stop_settings(config) -> Tuple[float, int]:
    """(eps, base segment length) of ``config``, validated: ValueError unless 0 <= eps < 1 and the length is a positive multiple of
    64.  Pure host code: nothing touches a device."""
    eps, base = float(config.eval_early_stop_eps), config.eval_segment_samples
    if not (0.0 <= eps < 1.0):          # (a NaN fails this too)
        raise ValueError(f"eval_early_stop_eps must satisfy 0 <= eps < 1, got {config.eval_early_stop_eps}")
    if isinstance(base, bool) or int(base) != base or int(base) <= 0 or int(base) % 64 != 0:
        raise ValueError(f"eval_segment_samples must be a positive multiple of 64, got {config.eval_segment_samples}")
    return eps, int(base)


def _render_early_stop(model, rb: RayBundle, chunk: int, check_overflow: bool = True, depth_select=None) -> Dict[str, Tensor]:
    """The count-free route with early ray termination: a chunk is marched as in ``_render_count_free`` but its samples stay in the
    marcher's per-ray slots; per segment of ``segment_schedule`` the live rays' samples are packed, the field evaluates them and
    ``lse_eval_composite_segment`` continues every ray from its saved state, finishing those whose optical depth has reached
    -ln(eps).  The segment count is known on the host (from the capacity); which rays are alive never is: a segment without a live
    ray is the same launches over a device-side count of 0."""
    cfg, fld = model.config, model.field
    eps, base = early_stop_settings(cfg)
    tau_stop = ops.eval_tau_stop(eps)
    R = len(rb)
    n = min(chunk, R)
    dev = rb.origins.device
    quant = _depth_quantiles_of(model, depth_select, R, n, dev, segmented=True)
    cap = model.occupancy_grid._cap_per_ray(cfg.near_plane, cfg.far_plane, cfg.render_step_size, cfg.cone_angle)
    sched = segment_schedule(cap, base)
    longest = max(length for _, length in sched)
    rgb = torch.empty((R, 3), dtype=torch.float32, device=dev)
    acc = torch.empty(R, dtype=torch.float32, device=dev)
    depth = torch.empty(R, dtype=torch.float32, device=dev)
    nsamples = torch.empty(R, dtype=torch.int64, device=dev)
    ws = torch.empty(3 * n, dtype=torch.float32, device=dev)
    # per image, sized by the longest segment: the packed sample arrays, the per-ray state and the segment bookkeeping
    state = torch.empty(ops.eval_segment_state_bytes(n), dtype=torch.uint8, device=dev)
    seg_cnts = torch.empty(n, dtype=torch.int64, device=dev)
    seg_packed = torch.empty((n, 2), dtype=torch.int64, device=dev)
    n_dev = torch.empty(1, dtype=torch.int64, device=dev)
    ri_buf = torch.empty(n * longest, dtype=torch.int32, device=dev)
    ts_buf = torch.empty(n * longest, dtype=torch.float32, device=dev)
    te_buf = torch.empty(n * longest, dtype=torch.float32, device=dev)
    linear = isinstance(model.renderer_rgb, LinearRenderer)
    bg = cfg.background_color
    background = None if bg in ("random", "last_sample") else {"black": 0.0, "white": 1.0}[bg]
    fld._prepass = None
    for lo in range(0, R, chunk):
        hi = min(R, lo + chunk)
        m = hi - lo
        part = _slice(rb, lo, hi)
        cnts, ts_slots, te_slots, cap_marched = model.sampler.march_slots(
            part, near_plane=cfg.near_plane, far_plane=cfg.far_plane, render_step_size=cfg.render_step_size,
            cone_angle=cfg.cone_angle)
        assert cap_marched == cap
        rays_o, rays_d = part.origins.contiguous(), part.directions.contiguous()
        table, eidx = fld._eval_emb(m, dev) if fld.embedding_appearance is not None else (None, None)
        packed = seg_packed[:m]
        ops.eval_segment_begin(cnts, sched[0][1], state, seg_cnts[:m])
        if quant is not None:
            quant.begin(lo, hi)
        for k, (off, length) in enumerate(sched):
            ops.pack_info_from_counts(seg_cnts[:m], out=(packed, n_dev))
            C = m * length
            ri, ts, te = ri_buf[:C], ts_buf[:C], te_buf[:C]
            ops.compact_ray_slots(ts_slots, te_slots, cap, packed, ri, ts, te, slot_offset=off)
            if k == 0:           # nerfstudio's fake sample belongs to the chunk: a chunk without any sample gets it here
                ops.fake_sample_if_empty(packed, n_dev, ri, ts, te)
            sigma, _, _, head = fld.density_rgb_packed(rays_o, rays_d, ri, ts, te, packed, eidx, table, n_dev)
            if quant is not None:      # its own state and launch: the compositor's state is not read
                quant.segment(ts, te, sigma, packed, lo, hi)
            next_len = sched[k + 1][1] if k + 1 < len(sched) else 0
            ops.eval_composite_segment(ts, te, sigma, head, packed, cnts, off + length, next_len, tau_stop, state,
                                       seg_cnts[:m] if next_len else None, nan_to_num=not linear)
        ops.eval_composite_finish(state, rgb[lo:hi], acc[lo:hi], depth[lo:hi], nsamples[lo:hi], background=background,
                                  clamp=not linear, workspace=ws)
    if check_overflow:
        model.occupancy_grid.check_deferred_overflow()      # the one read-back, as on the full route
    raw = {"rgb": rgb, "accumulation": acc[:, None], "depth": depth[:, None], "num_samples_per_ray": nsamples}
    if quant is not None:
        raw.update(quant.outputs())
    return {k: v for k, v in model.route_outputs(raw, rb).items() if torch.is_tensor(v)}


@torch.no_grad()
def render_flat(model, rb: RayBundle, check_overflow: bool = True, depth_select=None) -> Dict[str, Tensor]:
    """Outputs ``[R, ...]`` for the ``[R, ...]`` bundle ``rb``, chunked by ``config.eval_num_rays_per_chunk`` on every route (the
    chunking is observable: nerfstudio's fake sample is inserted per chunk).  ``check_overflow=False`` leaves out the count-free
    routes' ``check_deferred_overflow()`` behind the last chunk: the accumulator is sticky, so a caller that renders many images
    (``eval_set.evaluate_set``) reads it once behind the last of them -- and MUST do so.  With ``config.eval_depth_quantiles`` the
    count-free routes add "depth_quantiles" [R, n_q] and "depth_reached" [R, 1] (uint8, bit j: quantile j was reached), and with
    ``depth_select = (column, max_spread or None)`` also "depth_selected" [R, 1]: that column, NaN where it was not reached or the
    last column lies more than ``max_spread`` behind the first (what the exporters unproject and fuse).  The ``forward`` loop has no
    quantile depths: with the setting on it is a ValueError."""
    chunk = int(model.config.eval_num_rays_per_chunk)
    if chunk <= 0:
        raise ValueError("eval_num_rays_per_chunk must be positive")
    eps, _ = early_stop_settings(model.config)
    qs, _ = depth_quantile_settings(model.config)
    if len(rb) == 0:
        raise ValueError("empty ray bundle")
    more = {} if depth_select is None else {"depth_select": depth_select}
    if uses_count_free_route(model, len(rb)):
        if eps > 0.0:
            if model.eval_normals_on():
                raise ValueError("eval_normals is not built for the early-stop segment route: set eval_early_stop_eps = 0")
            return _render_early_stop(model, rb, chunk, check_overflow, **more)
        return _render_count_free(model, rb, chunk, check_overflow, **more)
    if qs or depth_select is not None:
        raise ValueError("eval_depth_quantiles is built for the count-free eval routes only (eval mode, LSEField with the full-size "
                         "base MLP, a chunk within deferred_max_slots): this render falls back to the forward loop -- set "
                         "eval_depth_quantiles = ()")
    return _render_loop(model, rb, chunk)


@torch.no_grad()
def render_ray_bundle(model, camera_ray_bundle) -> Dict[str, Tensor]:
    lead = tuple(camera_ray_bundle.origins.shape[:-1])
    out = render_flat(model, _flatten_bundle(camera_ray_bundle, device=model.scene_aabb.device))
    return {k: v.reshape(*lead, -1) for k, v in out.items()}


@torch.no_grad()
def render_camera(model, cameras, camera_index: int, camera_opt_to_camera: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """Every pixel of camera ``camera_index`` of ``cameras`` (``EdCameras``): ``generate_rays`` over ``get_image_coords()``, then
    ``render_ray_bundle``; outputs ``[H, W, C]``."""
    coords = cameras.get_image_coords()
    H, W = coords.shape[:2]
    idx = torch.full((H * W,), int(camera_index), dtype=torch.long)
    rb = cameras.generate_rays(idx, coords.reshape(-1, 2), camera_opt_to_camera=camera_opt_to_camera)
    dev = model.scene_aabb.device
    out = render_flat(model, _flatten_bundle(rb, device=dev))
    return {k: v.reshape(H, W, -1) for k, v in out.items()}


# ----------------------------------------------------------------------------------------------------
# metrics and images
# ----------------------------------------------------------------------------------------------------
class _MissingLPIPS:
    """Stands in for LPIPS where torchmetrics is absent: calling it raises ModuleNotFoundError naming what is missing."""
    available = False

    def __init__(self, missing: str):
        self.missing = missing

    def __call__(self, *args, **kwargs):
        raise ModuleNotFoundError(
            f"lpips needs torchmetrics' LearnedPerceptualImagePatchSimilarity(normalize=True), and '{self.missing}' is not "
            f"installed (its network weights are not part of this package either)", name=self.missing)


class _LPIPS:
    """torchmetrics LPIPS, moved to the device of its first input."""
    available = True

    def __init__(self, metric):
        self.metric = metric

    def __call__(self, preds: Tensor, target: Tensor) -> Tensor:
        if next(self.metric.parameters(), preds).device != preds.device:
            self.metric = self.metric.to(preds.device)
        return self.metric(preds, target)


def make_lpips():
    try:
        from torchmetrics.image.lpip import LearnedPerceptualImagePatchSimilarity
    except ModuleNotFoundError as e:
        return _MissingLPIPS((e.name or "torchmetrics").split(".")[0])
    return _LPIPS(LearnedPerceptualImagePatchSimilarity(normalize=True))


def make_error_map(image: Tensor, pred: Tensor, norm_cnst: float = 6.0) -> Tensor:
    """R:lse_nerf/lsenerf.py:442-460 restated: white where the grey levels agree; where the ground truth is brighter the green and
    blue channels drop by ``6 * difference`` (red remains), where it is darker red and green drop (blue remains)."""
    gray = lambda x: (x * x.new_tensor([0.2989, 0.5870, 0.1140])).sum(-1)
    err = (gray(image) - gray(pred)) * norm_cnst
    one = torch.ones_like(err)
    pos, neg = err > 0, err < 0
    r = torch.where(neg, 1 - err.abs(), one)
    g = torch.where(pos, 1 - err, torch.where(neg, 1 - err.abs(), one))
    b = torch.where(pos, 1 - err, one)
    return torch.stack([r, g, b], dim=-1)


def gray_colormap(image: Tensor, invert: bool = False) -> Tensor:
    """nerfstudio 0.3.2 ``apply_colormap`` of a one-channel float image with ``colormap="gray"``: clip to [0, 1], optionally
    ``1 - x``, three channels."""
    out = torch.clip(image, 0, 1)
    if invert:
        out = 1 - out
    return out.repeat(*([1] * (out.dim() - 1)), 3)


def normals_colormap(normals: Tensor, accumulation: Tensor) -> Tensor:
    """The picture of rendered normals as nerfstudio's viewer shows it: ``(n + 1) / 2`` blended with the accumulation onto white."""
    return (normals + 1) / 2 * accumulation + (1 - accumulation)


def depth_gray_map(depth: Tensor, accumulation: Tensor) -> Tensor:
    """nerfstudio 0.3.2 ``apply_depth_colormap(depth, accumulation, ColormapOptions(colormap="gray", invert=True))``: depth
    normalised by its own min / max, grey map inverted (near = white), blended with the accumulation onto white.  Restated, parity
    unpinned."""
    near, far = torch.min(depth), torch.max(depth)
    d = torch.clip((depth - near) / (far - near + 1e-10), 0, 1)
    return gray_colormap(d, invert=True) * accumulation + (1 - accumulation)


@torch.no_grad()
def make_overlay(image_planes: Tensor, pred_planes: Tensor) -> Tensor:
    """R:lse_nerf/lsenerf.py:462-475 on the device: float32 [H, W, 3] with values in {0, 1} -- white; black where the Canny edges
    (50, 200) of the 8-bit grey ground truth or prediction lie; then red = 1 on the ground truth's edges and blue = 1 on the
    prediction's (both: magenta).  ``image_planes`` / ``pred_planes``: float32 [3, H, W] or [1, 3, H, W], the masked images as
    ``ops.eval_image_prep`` writes them.  The reference returns ``overlay / 255`` in float64; its values are 0 and 1 as well, so
    these are the same numbers in float32.  The edges are ``ops.canny_edges``: OpenCV's published algorithm restated, parity
    unpinned (OpenCV is no dependency); the grey is ``lse_eval_image_prep``'s, as the reference's matmul order is not knowable."""
    H, W = int(image_planes.shape[-2]), int(image_planes.shape[-1])
    edges = ops.canny_edges(ops.gray8_planes(image_planes, pred_planes))
    grid = ops.eval_panels(("overlay",), H, W, edges=edges)
    return grid.to(torch.float32) / 255.0


@torch.no_grad()
def image_metrics_and_images(model, outputs: Dict[str, Tensor], batch: Dict[str, Tensor]):
    dev = outputs["rgb"].device
    image = batch["image"].to(dev)
    rgb = ori_rgb = outputs["rgb"]
    if batch.get("msk") is not None:
        msk = batch["msk"].to(dev)[..., None]
        image, rgb = image * msk, rgb * msk
    images = {"img": torch.cat([image, ori_rgb], dim=1),      # the unmasked prediction beside the (masked) ground truth
              "accumulation": gray_colormap(outputs["accumulation"]),
              "depth": depth_gray_map(outputs["depth"], outputs["accumulation"]),
              "err_map": make_error_map(image, rgb)}
    img_b = torch.moveaxis(image, -1, 0)[None].float().contiguous()     # [H, W, C] -> [1, C, H, W]
    rgb_b = torch.moveaxis(rgb, -1, 0)[None].float().contiguous()
    if getattr(getattr(model, "config", None), "eval_overlay", False):
        images["overlay"] = make_overlay(img_b, rgb_b)
    if outputs.get("ev_out") is not None:
        images["ev_out"] = outputs["ev_out"]
    if outputs.get("normals") is not None:
        images["normals"] = normals_colormap(outputs["normals"], outputs["accumulation"])
    ssim, mse = ops.image_metrics(img_b, rgb_b)
    psnr = 10.0 * torch.log10(1.0 / mse)
    values = torch.stack([psnr, ssim]).tolist()
    metrics = {"psnr": float(values[0]), "ssim": float(values[1])}
    lpips = model.lpips
    if getattr(lpips, "available", True):
        metrics["lpips"] = float(lpips(img_b, rgb_b))
    return metrics, images
