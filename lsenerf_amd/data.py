"""Device-resident training data and the in-graph batch composer: the hot loop of the reference's data manager
(``MultiCamManager.next_train``, R:lse_nerf/lse_datamanager.py:337-372 -- pixel sampler, pixel gather, ray generators,
``add_metadata``, ``CameraIdxFixer``) as ONE HIP launch that writes the three bundles and the batch of a step into static buffers.

    scene = DeviceScene.from_datasets(ColorDataset(...), EventFrameDataset(...), "cuda", rgb_times=...)
    n_col, n_evs = batch_split(3512, 0.66, "deblur")
    composer = BatchComposer(scene, n_col, n_evs, deblur=True, seed=0, num_embd=...)
    composer.set_poses(col=spline_tables(spline, scene.col.cameras, "deblur"), prev=spline_tables(spline, scene.evs.cameras, "evs"))
    (col, prev, nxt), batch = composer.compose()                # eager: the device step counter advances
    step = GraphedTrainStep(model, opt, composer=composer)      # or inside the captured step (lsenerf_amd.graph)

Sampling convention (this package's own; the docs say so): pixel ``i`` of a stream at step ``s`` is drawn with Philox4x32-10, key
``(seed & 0xffffffff, seed >> 32)``, counter ``(s & 0xffffffff, i, stream id (0 colour / 1 events), 0)``, and
``c = mulhi32(w0, n_images)``, ``y = mulhi32(w1, H)``, ``x = mulhi32(w2, W)`` -- uniform i.i.d. over images x pixels like
nerfstudio's ``floor(rand * [n, h, w])`` that ``EvPixelSampler`` inherits, with no bit parity to ``torch.rand``.
``draw_indices_host`` is the same integer arithmetic in numpy (exact), the twin the tests compare the device draw with.
With ``sampling=PixelSampling(...)`` pixels are drawn by integer weight instead -- masked pixels never, event pixels by whether
their frame value is non-zero -- by ``lse_pixel_draw`` in front of the compose launch (``PixelSampling``; opt-in).

The composer reads poses from POSE TABLES in device memory (``pose_tables``), never from an optimiser: the helpers at the end of
this module build the tables from what ``cameras.py`` has (plain ``camera_to_worlds``, ``CameraOptimizer``, the spline) as
differentiable torch expressions over O(cameras) rows, and ``lse_compose_rays_bwd`` returns the gradient w.r.t. the tables.

The outputs of ``compose`` ARE the composer's static buffers (row blocks of one buffer per field, the layout
``graph._static_bundles`` uses): the next ``compose`` overwrites them.  All images are resident (the reference's
``num_images_to_sample_from = -1``); an image-subset cache and patch sampling are out of scope.  Whole eval images are
``lsenerf_amd.eval_set``'s: an ``EvalSet`` is a ``CameraSetData`` with a pose table of its own.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .cameras import EdCameras
from .rays import RayBundle


# ---------------------------------------------------------------------------------------------------- host-side arithmetic
def batch_split(train_num_rays_per_batch: int, rgb_frac: float, rgb_loss_mode: str = "mse") -> Tuple[int, int]:
    """``(n_col_pixels, n_evs_pixels)`` of a step (R:lse_nerf/lse_datamanager.py:135-144): the event pixels take half of the
    non-colour share (each gives two rays); a deblur colour pixel gives four rays."""
    n_evs = int((1 - rgb_frac) * train_num_rays_per_batch * 0.5)
    n_col = train_num_rays_per_batch - n_evs * 2
    if rgb_loss_mode.lower() == "deblur":
        n_col = int(n_col * (1 / 4))
    return n_col, n_evs


_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter: np.ndarray, key: Sequence[int]) -> np.ndarray:
    """Philox4x32-10 (Salmon et al., SC'11): ``counter`` uint32 [..., 4], ``key`` two uint32 words -> uint32 [..., 4]."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c[0], _PHILOX_M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK32]
        k0, k1 = (k0 + _PHILOX_W0) & 0xFFFFFFFF, (k1 + _PHILOX_W1) & 0xFFFFFFFF
    return np.stack(c, -1).astype(np.uint32)


def draw_indices_host(seed: int, step: int, stream_id: int, n_pixels: int, n_images: int, height: int, width: int) -> np.ndarray:
    """The composer's draw on the host: int64 [n_pixels, 3] = (c, y, x) (module docstring).  Integers only, so exact."""
    ctr = np.zeros((n_pixels, 4), dtype=np.uint32)
    ctr[:, 0] = int(step) & 0xFFFFFFFF
    ctr[:, 1] = np.arange(n_pixels, dtype=np.uint32)
    ctr[:, 2] = stream_id
    w = philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)).astype(np.uint64)
    lim = np.array([n_images, height, width], dtype=np.uint64)
    return ((w[:, :3] * lim[None]) >> np.uint64(32)).astype(np.int64)


@dataclass
class PixelSampling:
    """Weighted pixel sampling of a ``BatchComposer`` (``sampling=``; None, the default, is the uniform draw above).

    Every pixel of a stream has an integer weight and is drawn with a probability proportional to it:
      colour pixel   1, or 0 where ``respect_mask`` and the set's ``msk`` is 0
      event pixel    ``evs_active_weight`` where the frame's value is != 0, ``evs_idle_weight`` where it is == 0, or 0 where
                     ``respect_mask`` and the set's ``msk`` is 0
    "Active" compares the STORED frame value, converted to float32 the way the gather converts it, with zero: ``-0.0`` is idle, a
    pixel whose events cancelled to a net 0 is idle, NaN is active.  ``respect_mask`` does nothing for a set without ``msk``.  The
    weights are integers in [0, 255], not both zero; a weight of 0 means such pixels are never drawn.

    Unequal event weights CHANGE THE OBJECTIVE -- the loss becomes a weighted mean over the pixels, as with the negative sampling
    of EventNeRF -- and so does a mask.  ``BatchComposer.draw_weights`` holds the weight of every drawn pixel: a caller who wants the
    uniform objective back reweights each ray's loss by ``1 / weight`` (times ``sampling_totals / pixels`` for the same scale).

    The draw (include/lse_hip.h, "weighted pixel draw"; integers only, ``BatchComposer.indices_host`` is its host twin): with
    ``row_off`` the exclusive prefix sums of the image rows' summed weights, the Philox call of the uniform draw gives
    ``t = mulhi64((w0 << 32) | w1, total)``, the row is the last ``r`` with ``row_off[r] <= t``, the pixel the last ``x`` of that row
    whose exclusive prefix sum is ``<= t - row_off[r]``.  A stream takes this route whenever ``sampling`` is set, also where its
    weights end up all equal: which pixels a step draws depends on the setting, never on the data."""
    respect_mask: bool = True
    evs_active_weight: int = 1
    evs_idle_weight: int = 1

    def __post_init__(self):
        for name in ("evs_active_weight", "evs_idle_weight"):
            w = getattr(self, name)
            if isinstance(w, bool) or not isinstance(w, (int, np.integer)) or not 0 <= int(w) <= 255:
                raise ValueError(f"PixelSampling.{name} must be an integer in [0, 255], got {w!r}")
            setattr(self, name, int(w))
        if self.evs_active_weight == 0 and self.evs_idle_weight == 0:
            raise ValueError("PixelSampling: evs_active_weight and evs_idle_weight are both zero")
        self.respect_mask = bool(self.respect_mask)


class _WeightedStream:
    """One stream of a composer with ``sampling``: what ``ops.pixel_rows_build`` / ``ops.pixel_draw`` take, the row table (8 bytes
    per image row -- the whole state of the feature) and the static outputs of the draw."""

    def __init__(self, data: "CameraSetData", stream_id: int, n: int, images: Optional[Tensor], w_active: int, w_idle: int,
                 respect_mask: bool, device):
        self.data, self.stream_id, self.n = data, stream_id, n
        self.images, self.msk = images, (data.msk if respect_mask else None)
        self.shape = (data.n_images, data.H, data.W)
        self.w_active, self.w_idle = w_active, w_idle
        self.row_off = torch.zeros(data.n_images * data.H + 1, dtype=torch.int64, device=device)
        self.indices = torch.zeros(n, 3, dtype=torch.int32, device=device)
        self.weights = torch.zeros(n, dtype=torch.int32, device=device)
        self.total = 0

    def build(self) -> int:
        from . import ops
        ops.pixel_rows_build(self.images, self.msk, self.shape, self.w_active, self.w_idle, row_off=self.row_off)
        self.total = int(self.row_off[-1])          # the one host read, at set-up
        return self.total

    def draw(self, step: Optional[int], step_dev: Tensor, seed: int) -> None:
        from . import ops
        ops.pixel_draw(self.images, self.msk, self.shape, self.w_active, self.w_idle, self.row_off, seed, self.stream_id, self.n,
                       step=step, step_dev=step_dev if step is None else None, indices=self.indices, weights=self.weights)

    def row_weights(self, rows: np.ndarray) -> np.ndarray:
        """int64 [len(rows), W]: the weights of the given image rows, computed on the device from the resident data."""
        _, H, W = self.shape
        r = torch.as_tensor(rows, dtype=torch.int64, device=self.row_off.device)
        if self.images is None:
            w = torch.full((len(rows), W), self.w_idle, dtype=torch.int64, device=r.device)
        else:
            active = self.images.reshape(-1, W)[r].to(torch.float32) != 0
            w = torch.where(active, self.w_active, self.w_idle).to(torch.int64)
        if self.msk is not None:
            w = torch.where(self.msk.reshape(-1, W)[r].to(torch.float32) == 0, torch.zeros_like(w), w)
        return w.cpu().numpy()

    def draw_host(self, seed: int, step: int) -> Tuple[np.ndarray, np.ndarray]:
        """``(indices int64 [n, 3], weights int64 [n])``: the draw in Python integers and numpy (exact)."""
        _, H, W = self.shape
        ctr = np.zeros((self.n, 4), dtype=np.uint32)
        ctr[:, 0] = int(step) & 0xFFFFFFFF
        ctr[:, 1] = np.arange(self.n, dtype=np.uint32)
        ctr[:, 2] = self.stream_id
        p = philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
        row_off = self.row_off.cpu().numpy()
        total = int(row_off[-1])
        t = np.array([(((int(a) << 32) | int(b)) * total) >> 64 for a, b in p[:, :2]], dtype=np.int64)
        r = np.searchsorted(row_off[:-1], t, side="right") - 1
        v = t - row_off[r]
        uniq, inv = np.unique(r, return_inverse=True)
        w = self.row_weights(uniq)[inv] if self.n else np.zeros((0, W), np.int64)
        excl = np.cumsum(w, axis=1) - w
        x = (excl <= v[:, None]).sum(1) - 1
        idx = np.stack([r // H, r % H, x], axis=1).astype(np.int64)
        return idx, (w[np.arange(self.n), x] if self.n else np.zeros(0, np.int64))


def find_closest_idxs(ref: Tensor, srch: Tensor) -> Tensor:
    """Index of the element of the ascending ``ref`` closest to every element of ``srch``; of two equally close ones the later
    (R:lse_nerf/data_components.py:5-29)."""
    ins = torch.searchsorted(ref.contiguous(), srch.contiguous()).clamp(max=len(ref) - 1)
    prev = (ins - 1).clamp(min=0)
    return torch.where((ref[prev] - srch).abs() < (ref[ins] - srch).abs(), prev, ins)


# ---------------------------------------------------------------------------------------------------- the resident scene
_PIX_OF = {torch.int8: _lib.LSE_PIX_I8, torch.uint8: _lib.LSE_PIX_U8, torch.int16: _lib.LSE_PIX_I16, torch.int32: _lib.LSE_PIX_I32,
           torch.float32: _lib.LSE_PIX_F32}


def _as_tensor(a) -> Tensor:
    return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))


class CameraSetData:
    """One camera set on the device: images, optional masks, per-image appearance id and camera index, per-camera times, and the
    host ``EdCameras`` (intrinsics, distortion, the poses the default tables start from)."""

    def __init__(self, device, images: Tensor, cameras: EdCameras, appearance_ids, msk=None, image_idx=None, channels: int = 1):
        images = _as_tensor(images)
        if channels == 1 and images.dim() == 4:
            assert images.shape[-1] == 1, f"event frames are [n, H, W] or [n, H, W, 1], got {tuple(images.shape)}"
            images = images[..., 0]
        n, H, W = images.shape[:3]
        if (H, W) != (cameras.height, cameras.width):
            raise ValueError(f"images are {H} x {W}, the cameras {cameras.height} x {cameras.width}")
        if images.dtype not in _PIX_OF:        # int64 that fits -> int32; anything else (float64, float16, ...) -> float32
            fits = images.dtype == torch.int64 and (images.numel() == 0 or int(images.abs().max()) < 2 ** 31)
            images = images.to(torch.int32 if fits else torch.float32)
        self.pix_type = _PIX_OF[images.dtype]
        self.images = images.contiguous().to(device)
        self.n_images, self.H, self.W = int(n), int(H), int(W)
        self.cameras = cameras
        self.n_cameras = len(cameras)
        self.msk, self.msk_type = None, _lib.LSE_PIX_NONE
        if msk is not None:
            msk = _as_tensor(msk)
            if msk.dim() == 4:
                msk = msk[..., 0]
            assert tuple(msk.shape) == (n, H, W), f"masks are {tuple(msk.shape)}, images {(n, H, W)}"
            msk = msk.to(torch.uint8) if msk.dtype in (torch.bool, torch.uint8) else msk.to(torch.float32)
            self.msk, self.msk_type = msk.contiguous().to(device), _PIX_OF[msk.dtype]
        app = torch.as_tensor(list(appearance_ids) if not torch.is_tensor(appearance_ids) else appearance_ids).reshape(-1)
        assert app.numel() == n, f"{app.numel()} appearance ids for {n} images"
        self.appearance_id = app.to(torch.int32).to(device)
        idx = torch.arange(n) if image_idx is None else torch.as_tensor(image_idx).reshape(-1)
        assert idx.numel() == n and int(idx.min()) >= 0 and int(idx.max()) < self.n_cameras, "image_idx must name cameras of the set"
        self.image_idx_host = idx.to(torch.int64)
        self.image_idx = idx.to(torch.int32).to(device)
        times = cameras.times.reshape(-1).float() if cameras.times is not None else torch.zeros(self.n_cameras)
        self.times = times.contiguous().to(device)
        dist = cameras.distortion_params
        if dist is not None and dist.dim() != 1:
            raise ValueError("the composer takes one set of distortion parameters per camera set")
        self.distort = bool(dist is not None and bool((dist != 0).any()))
        self.dist = [float(v) for v in dist] if self.distort else [0.0] * 6

    def stream_desc(self, n_pixels: int) -> "_lib.ComposeStream":
        cam = self.cameras
        return _lib.ComposeStream(fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy, dist=(ctypes.c_float * 6)(*self.dist), H=self.H, W=self.W,
                                  n_images=self.n_images, n_cameras=self.n_cameras, n_pixels=int(n_pixels), pix_type=self.pix_type,
                                  msk_type=self.msk_type, distort=int(self.distort))


class DeviceScene:
    """The training data of a scene in device memory, uploaded once: ``col`` / ``evs`` (``CameraSetData`` or None).  The event set
    also carries ``e_thresh`` (what every event ray's ``e_thresh`` reads), ``e_scale`` (target = float(frame) * e_scale), the
    previous / next camera sets of ``PrevNextRayGenerator`` when the scene has them, and for every event camera the index of the
    closest colour-camera time (``CameraIdxFixer``, R:lse_nerf/data_components.py:70-90; the identity without ``rgb_times``)."""

    def __init__(self, device, col: Optional[CameraSetData], evs: Optional[CameraSetData], e_thresh: float = 1.0, e_scale: float = 1.0,
                 prev_cameras: Optional[EdCameras] = None, next_cameras: Optional[EdCameras] = None, rgb_times: Optional[Tensor] = None):
        assert col is not None or evs is not None, "a scene needs a colour set or an event set"
        self.device = torch.device(device)
        self.col, self.evs = col, evs
        self.e_thresh, self.e_scale = float(e_thresh), float(e_scale)
        self.prev_cameras, self.next_cameras = prev_cameras, next_cameras
        self.rgb_times = None if rgb_times is None else torch.as_tensor(rgb_times).reshape(-1).float()
        if evs is not None:
            sets = {"consec": evs.cameras}
            if prev_cameras is not None:
                assert next_cameras is not None and len(prev_cameras) == len(next_cameras) == evs.n_cameras
                sets.update(prev=prev_cameras, next=next_cameras)
            self.evs_times: Dict[str, Tensor] = {}
            self.evs_closest: Dict[str, Tensor] = {}
            for k, cams in sets.items():
                t = cams.times.reshape(-1).float() if cams.times is not None else torch.zeros(len(cams))
                closest = find_closest_idxs(self.rgb_times, t) if self.rgb_times is not None else torch.arange(len(cams))
                self.evs_times[k] = t.contiguous().to(self.device)
                self.evs_closest[k] = closest.to(torch.int32).to(self.device)

    @classmethod
    def from_arrays(cls, device, col_images=None, col_cameras: Optional[EdCameras] = None, col_appearance_ids=None, col_msk=None,
                    col_image_idx=None, evs_frames=None, evs_cameras: Optional[EdCameras] = None, evs_appearance_ids=None,
                    evs_msk=None, evs_image_idx=None, e_thresh: float = 1.0, prev_cameras: Optional[EdCameras] = None,
                    next_cameras: Optional[EdCameras] = None, rgb_times=None) -> "DeviceScene":
        """In-memory arrays: ``col_images`` uint8 [Nc, H, W, 3]; ``evs_frames`` [Ne, H, W] (or [..., 1]) -- integer frames stay in their
        own type (one byte per pixel for int8 / uint8) and are scaled by ``e_thresh`` at the gather; anything non-integer is taken as
        the final float32 target."""
        col = evs = None
        if col_images is not None:
            img = _as_tensor(col_images)
            assert img.dtype == torch.uint8 and img.dim() == 4 and img.shape[-1] >= 3, "colour images are uint8 [N, H, W, 3]"
            col = CameraSetData(device, img[..., :3], col_cameras, col_appearance_ids, col_msk, col_image_idx, channels=3)
        e_scale = 1.0
        if evs_frames is not None:
            fr = _as_tensor(evs_frames)
            integer = not (fr.dtype.is_floating_point or fr.dtype.is_complex)
            e_scale = float(np.float32(e_thresh)) if integer else 1.0
            evs = CameraSetData(device, fr, evs_cameras, evs_appearance_ids, evs_msk, evs_image_idx, channels=1)
        return cls(device, col, evs, e_thresh=float(np.float32(e_thresh)), e_scale=e_scale, prev_cameras=prev_cameras,
                   next_cameras=next_cameras, rgb_times=rgb_times)

    @classmethod
    def from_datasets(cls, color_dataset, event_dataset, device, rgb_times=None) -> "DeviceScene":
        """``scene_io.ColorDataset`` / ``EventFrameDataset`` (either may be None) -> resident scene.  ``rgb_times``: the colour cameras'
        times for ``CameraIdxFixer`` (None: the event bundles keep their own camera indices, as the reference does without them)."""
        kw = {}
        if color_dataset is not None:
            imgs = np.stack([color_dataset.get_numpy_image(i)[:, :, :3] for i in range(len(color_dataset))])
            kw.update(col_images=imgs, col_cameras=color_dataset.cameras, col_appearance_ids=color_dataset.appearance_ids,
                      col_msk=color_dataset.msk)
        if event_dataset is not None:
            evs = event_dataset.evs
            e_thresh = float(event_dataset.e_thresh[0])
            if evs.dtype.is_floating_point:             # the float32 get_image values themselves, threshold already applied
                evs = torch.stack([event_dataset.get_image(i) for i in range(len(event_dataset))])
            out = event_dataset.out
            kw.update(evs_frames=evs, evs_cameras=event_dataset.cameras, evs_appearance_ids=event_dataset.appearance_ids[:len(evs)],
                      evs_msk=event_dataset.msk[:len(evs)] if event_dataset.msk is not None else None, e_thresh=e_thresh,
                      prev_cameras=out.prev_cameras, next_cameras=out.next_cameras)
        return cls.from_arrays(device, rgb_times=rgb_times, **kw)


# ---------------------------------------------------------------------------------------------------- the composer
def _ptr(t: Optional[Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _ComposeRays(torch.autograd.Function):
    """pose tables -> (origins, directions) of a composed step; backward = lse_compose_rays_bwd on the tables and pixels of THAT
    step (saved copies: O(cameras) + O(rays) integers)."""

    @staticmethod
    def forward(ctx, composer, step, indices, *tables):
        names = [n for n, t in zip(("col", "prev", "nxt"), composer.pose_tables) if t is not None]
        composer.set_poses(**dict(zip(names, tables)))
        composer._launch(step, indices)
        ctx.composer = composer
        ctx.saved = (composer._ray_px.clone(), [None if t is None else t.clone() for t in composer.pose_tables])
        return composer._buf["origins"].clone(), composer._buf["directions"].clone()

    @staticmethod
    def backward(ctx, g_o, g_d):
        ray_px, tables = ctx.saved
        grads = ctx.composer._rays_bwd(g_o.contiguous(), g_d.contiguous(), ray_px=ray_px, tables=tables, static=False)
        return (None, None, None) + tuple(g for g in grads if g is not None)


class BatchComposer:
    """One step's batch from a ``DeviceScene``: ``n_col_pixels`` colour pixels (``G`` = 4 rays each with ``deblur``, else 1) and
    ``n_evs_pixels`` event pixels (one ray in the previous and one in the next bundle).

    ``event_pairing``: "consec" (``ConsecRayGenerator``: ONE table over the event set's cameras, read at ``c`` and ``c + 1``;
    ``pose_tables[2]`` is None) or "prevnext" (``PrevNextRayGenerator``: two tables, both read at ``c``).
    ``num_embd``: the clip bound of the deblur appearance offsets (R:lse_nerf/utils.py:170-178); default: largest colour id + 1.
    ``sampling``: a ``PixelSampling`` -- pixels are drawn by integer weight (masked pixels never, event pixels by activity) by one
    ``lse_pixel_draw`` launch per stream in front of the compose launch, which then takes the drawn pixels as given indices.
    ``draw_weights`` = ``(col, evs)`` int32 [n] static tensors: the weight of every pixel of the last draw (a stream whose pixels
    came from ``compose(indices=...)`` keeps those of its last draw); ``sampling_totals`` = ``(col, evs)`` the streams' total
    weights, read once here, ValueError where one is 0; ``rebuild_sampling()`` after the resident images or masks were edited in
    place.  Both are None with ``sampling=None``, which launches and allocates exactly what it did without this argument."""

    def __init__(self, scene: DeviceScene, n_col_pixels: int, n_evs_pixels: int, deblur: bool = False, seed: int = 0,
                 event_pairing: str = "consec", num_embd: Optional[int] = None, sampling: Optional[PixelSampling] = None):
        assert event_pairing in ("consec", "prevnext"), event_pairing
        if not 0 <= int(seed) < 2 ** 64:
            raise ValueError("seed must fit 64 unsigned bits")
        if sampling is not None and not isinstance(sampling, PixelSampling):
            raise ValueError(f"sampling= takes a PixelSampling or None, got {type(sampling).__name__}")
        self.scene, self.seed = scene, int(seed)
        self.n_col = int(n_col_pixels) if scene.col is not None else 0
        self.n_evs = int(n_evs_pixels) if scene.evs is not None else 0
        if self.n_col != int(n_col_pixels) or self.n_evs != int(n_evs_pixels):
            raise ValueError("pixels were asked from a camera set the scene does not have")
        assert self.n_col + self.n_evs > 0, "no pixels in this step"
        self.G = 4 if deblur else 1
        self.consec = event_pairing == "consec"
        dev = scene.device
        col, evs = scene.col, scene.evs
        if self.n_col and num_embd is None:
            num_embd = int(col.appearance_id.max()) + 1
        self.num_embd = int(num_embd or 1)
        if self.n_evs:
            if self.consec:
                assert int(evs.image_idx_host.max()) + 1 < evs.n_cameras, \
                    "consecutive event cameras: every frame needs the camera after its own (n_frames + 1 <= n_cameras)"
            else:
                assert scene.prev_cameras is not None, "event_pairing='prevnext' needs the scene's prev / next camera sets"
        nc, ne, G = self.n_col, self.n_evs, self.G
        self.rows = {"col": (0, nc * G), "prev": (nc * G, nc * G + ne), "nxt": (nc * G + ne, nc * G + 2 * ne)}
        R = self.n_rays = nc * G + 2 * ne
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
        self._buf = {"origins": f32(R, 3), "directions": f32(R, 3), "pixel_area": f32(R, 1), "directions_norm": f32(R, 1),
                     "times": f32(R, 1), "camera_indices": torch.zeros(R, 1, dtype=torch.int64, device=dev),
                     "appearance_id": i32(R, 1), "cam_type": i32(R), "coords": i32(R, 3)}
        self._ray_px = i32(R, 3)
        self.col_batch = self.evs_batch = None
        if nc:
            self.col_batch = {"image": f32(nc, 3), "indices": i32(nc, 3), "appearance_id": i32(nc)}
            if col.msk is not None:
                self.col_batch["msk"] = f32(nc, 1)
        if ne:
            self.evs_batch = {"image": f32(ne, 1), "e_thresh": f32(ne, 1), "indices": i32(ne, 3), "appearance_id": i32(ne)}
            if evs.msk is not None:
                self.evs_batch["msk"] = f32(ne, 1)
        self.batch = {"col_batch": self.col_batch, "evs_batch": self.evs_batch}
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        # pose tables, started from the scene's own poses (every deblur slot of a camera: its one pose)
        t_col = t_prev = t_nxt = None
        if nc:
            t_col = col.cameras.camera_to_worlds[:, None].expand(-1, G, -1, -1).contiguous().to(dev)
        if ne:
            if self.consec:
                t_prev = evs.cameras.camera_to_worlds.contiguous().to(dev)
            else:
                t_prev = scene.prev_cameras.camera_to_worlds.contiguous().to(dev)
                t_nxt = scene.next_cameras.camera_to_worlds.contiguous().to(dev)
        self.pose_tables: Tuple[Optional[Tensor], Optional[Tensor], Optional[Tensor]] = (t_col, t_prev, t_nxt)
        self._pose_grads = tuple(None if t is None else torch.zeros_like(t) for t in self.pose_tables)
        self.spline = None                     # attach_spline(): a SplinePoses that fills (some of) the tables in front of every compose
        self.deltas = None                     # attach_camera_optimizers(): a DeltaPoses, the same for the per-camera optimisers
        self.bundles = self._make_bundles(self._buf["origins"], self._buf["directions"])
        # C-ABI descriptors (host structs; the pointers are those of the static tensors above)
        key = "consec" if self.consec else "prev"
        self._desc = _lib.ComposeDesc(
            col=col.stream_desc(nc) if nc else _lib.ComposeStream(), evs=evs.stream_desc(ne) if ne else _lib.ComposeStream(), G=G,
            num_embd=self.num_embd, consecutive=int(self.consec), e_scale=scene.e_scale, e_thresh=scene.e_thresh, seed=self.seed)
        s = _lib.ComposeScene()
        if nc:
            s.col_images, s.col_msk, s.col_appearance_id = _ptr(col.images), _ptr(col.msk), _ptr(col.appearance_id)
            s.col_image_idx, s.col_times, s.col_pose = _ptr(col.image_idx), _ptr(col.times), _ptr(t_col)
        if ne:
            s.evs_images, s.evs_msk, s.evs_appearance_id = _ptr(evs.images), _ptr(evs.msk), _ptr(evs.appearance_id)
            s.evs_image_idx = _ptr(evs.image_idx)
            s.prev_times, s.prev_closest, s.prev_pose = _ptr(scene.evs_times[key]), _ptr(scene.evs_closest[key]), _ptr(t_prev)
            if not self.consec:
                s.next_times, s.next_closest, s.next_pose = _ptr(scene.evs_times["next"]), _ptr(scene.evs_closest["next"]), _ptr(t_nxt)
        self._scene_desc = s
        o = _lib.ComposeOut(row_col=self.rows["col"][0], row_prev=self.rows["prev"][0], row_next=self.rows["nxt"][0], n_rows=R)
        for k, v in self._buf.items():
            setattr(o, k, _ptr(v))
        o.ray_px = _ptr(self._ray_px)
        if nc:
            b = self.col_batch
            o.col_image, o.col_msk, o.col_indices = _ptr(b["image"]), _ptr(b.get("msk")), _ptr(b["indices"])
            o.col_batch_appearance_id = _ptr(b["appearance_id"])
        if ne:
            b = self.evs_batch
            o.evs_image, o.evs_msk, o.evs_e_thresh = _ptr(b["image"]), _ptr(b.get("msk")), _ptr(b["e_thresh"])
            o.evs_indices, o.evs_batch_appearance_id = _ptr(b["indices"]), _ptr(b["appearance_id"])
        self._out_desc = o
        # weighted sampling: per stream a row table and the static outputs of the draw (nothing at all with sampling=None)
        self.sampling = sampling
        self._weighted: Tuple[Optional[_WeightedStream], Optional[_WeightedStream]] = (None, None)
        self.draw_weights = self.sampling_totals = None
        if sampling is not None:
            self._weighted = (
                _WeightedStream(col, 0, nc, None, 1, 1, sampling.respect_mask, dev) if nc else None,
                _WeightedStream(evs, 1, ne, evs.images, sampling.evs_active_weight, sampling.evs_idle_weight, sampling.respect_mask,
                                dev) if ne else None)
            self.draw_weights = tuple(None if w is None else w.weights for w in self._weighted)
            self.rebuild_sampling()

    # -- weighted sampling
    def rebuild_sampling(self) -> Tuple[Optional[int], Optional[int]]:
        """Build the row tables of the weighted draw again from the resident images and masks -- after a caller edited them in place
        -- and read the streams' total weights (one host read per stream; ValueError where a total is 0, as at construction).
        Returns ``sampling_totals``."""
        if self.sampling is None:
            raise ValueError("this composer draws uniformly (sampling=None): there are no tables to rebuild")
        totals = []
        for name, w in zip(("colour", "event"), self._weighted):
            totals.append(None if w is None else w.build())
            if totals[-1] == 0:
                raise ValueError(f"weighted sampling: the {name} stream has a total weight of 0 -- every pixel is masked out or has "
                                 f"a weight of 0, nothing can be drawn")
        self.sampling_totals = tuple(totals)
        return self.sampling_totals

    # -- buffers as bundles
    def _make_bundles(self, origins: Tensor, directions: Tensor) -> Tuple[Optional[RayBundle], ...]:
        """The three bundles as row blocks of one buffer per field (``origins`` / ``directions``: the static buffers, or the outputs
        of the autograd route)."""
        single = self.n_evs == 0                  # one bundle: it IS the buffer (graph._fresh_ray_leaves)
        out = []
        for name in ("col", "prev", "nxt"):
            lo, hi = self.rows[name]
            if hi == lo:
                out.append(None)
                continue
            cut = (lambda t: t) if single else (lambda t: t[lo:hi])
            with torch.no_grad():
                fixed = {k: cut(v) for k, v in self._buf.items()}
            o, d = (cut(origins), cut(directions)) if origins.requires_grad else (fixed["origins"], fixed["directions"])
            out.append(RayBundle(origins=o, directions=d, pixel_area=fixed["pixel_area"], camera_indices=fixed["camera_indices"],
                                 times=fixed["times"],
                                 metadata={k: fixed[k] for k in ("directions_norm", "appearance_id", "cam_type", "coords")}))
        return tuple(out)

    # -- the draw position
    @torch.no_grad()
    def set_step(self, step: int) -> None:
        """Set the draw position: the next ``compose()`` -- eager, or the replay of a step captured with ``composer=`` -- draws what
        ``indices_host(step)`` lists, the one after it ``step + 1``.  A fill of ``step_dev`` in stream order (no synchronisation,
        like ``FlatAdam.prepare_step``): replays queued earlier keep their positions.  A checkpoint does not carry the position;
        a run resumed from one written after step ``s`` continues with ``set_step(s + 1)``, before or after the step is captured
        (a capture puts back the position it found)."""
        step = int(step)
        if not 0 <= step < 2 ** 63:
            raise ValueError(f"the draw position is a step number, got {step}")
        self.step_dev.fill_(step)

    # -- poses
    @torch.no_grad()
    def set_poses(self, col: Optional[Tensor] = None, prev: Optional[Tensor] = None, nxt: Optional[Tensor] = None) -> None:
        """Copy new poses into the static tables, in place, in stream order (no synchronisation): ``col`` [C, G, 3, 4] (or [C, 3, 4]:
        every slot of a camera), ``prev`` / ``nxt`` [Ce, 3, 4] ("consec": ``prev`` is the one event table and ``nxt`` must be None)."""
        for i, (name, dst, src) in enumerate(zip(("col", "prev", "nxt"), self.pose_tables, (col, prev, nxt))):
            if src is None:
                continue
            if dst is None:
                raise ValueError(f"this composer has no '{name}' pose table")
            if self.spline is not None and self.spline.fed[i]:
                raise ValueError(f"the '{name}' pose table is fed by the attached spline: every compose() overwrites it")
            if self.deltas is not None and self.deltas.fed[i]:
                raise ValueError(f"the '{name}' pose table is fed by the attached camera optimiser: every compose() overwrites it")
            if name == "col" and src.dim() == 3:
                src = src[:, None].expand(-1, self.G, -1, -1)
            if tuple(src.shape) != tuple(dst.shape):
                raise ValueError(f"'{name}' pose table is {tuple(dst.shape)}, got {tuple(src.shape)}")
            dst.copy_(src, non_blocking=True)

    def attach_spline(self, spline, tables: Optional[Sequence[str]] = None):
        """From now on the pose tables come from ``spline`` (a ``SplineCameraOptimizer`` on the composer's device) by one launch in
        front of every ``compose()`` -- ``lse_spline_poses``, the device-side counterpart of ``spline_tables`` -- so they are always
        those of the spline's CURRENT parameters, which the kernel reads in place.  The colour table is fed as "deblur" when G == 4,
        else as "rgb" at the colour cameras' times; prev / nxt as "evs" at the event cameras' times of this composer's pairing.
        ``tables``: the names ("col", "prev", "nxt") to feed; default: every table the composer has.  ``set_poses`` on a fed table
        and ``compose(tables=...)`` then raise ValueError -- the latter also when only a subset is fed: the tables the spline does
        not feed are then set with ``set_poses`` only, there is no differentiable eager route to them while a spline is attached.  Indices, fractions and the backward's query lists are computed here,
        once; ``spline_grads`` / ``spline_pose_tables`` are the way back to the parameters.  A spline whose mode is "off" (frozen,
        or "delayed" before ``turn_on()``) is refused with ValueError: its tables are constant, ``set_poses`` once is the right
        call; attach after ``turn_on()`` and rebuild the captured step.  Returns the ``SplinePoses``."""
        from .spline_dev import SEGMENTS, SplinePoses
        names = [n for n, t in zip(SEGMENTS, self.pose_tables) if t is not None] if tables is None else list(tables)
        for n in names:
            if n not in SEGMENTS or self.pose_tables[SEGMENTS.index(n)] is None:
                raise ValueError(f"this composer has no '{n}' pose table")
        scene = self.scene
        key = "consec" if self.consec else "prev"
        times = {"col": None if not self.n_col else ("deblur" if self.G == 4 else "rgb", scene.col.times),
                 "prev": None if not self.n_evs else ("evs", scene.evs_times[key]),
                 "nxt": None if not self.n_evs or self.consec else ("evs", scene.evs_times["next"])}
        if self.G == 4 and "col" in names and int(spline.n_deblur_rays) != self.G:
            raise ValueError(f"the spline has {spline.n_deblur_rays} deblur cameras per exposure, the composer {self.G} rays per pixel")
        if self.deltas is not None and any(self.deltas.fed[SEGMENTS.index(n)] for n in names):
            raise ValueError("a pose table named here is already fed by an attached camera optimiser")
        segments = [times[n] if n in names else None for n in SEGMENTS]
        shapes = [None if t is None else tuple(t.shape) for t in self.pose_tables]
        self.spline = SplinePoses(spline, segments, shapes, scene.device)
        return self.spline

    def spline_grads(self, pose_grads, out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
        """``{"ctrl_tangents": [K, 6], "scale": [1]}``: the gradients of the attached spline's parameters from the gradients of the
        pose tables -- ``pose_grads`` as ``pose_grads()`` returns them or as ``GraphedTrainStep.pose_grads`` holds them (entries of
        tables the spline does not feed are ignored).  One launch of fixed-order sums (two calls are bit-equal, control points that
        no query brackets get exactly zero); the result lives in static tensors that the next call overwrites, or in ``out``."""
        if self.spline is None:
            raise ValueError("no spline attached (attach_spline)")
        if isinstance(pose_grads, dict):
            pose_grads = [pose_grads.get(k) for k in ("col", "prev", "next")]
        return self.spline.backward(list(pose_grads), out=out)

    def spline_pose_tables(self):
        """``(col, prev, nxt)`` of the attached spline as NEW tensors with autograd history back to ``ctrl_tangents`` / ``scale`` (None
        where the spline feeds none): the eager, differentiable twin of what ``compose()`` writes into ``pose_tables``."""
        if self.spline is None:
            raise ValueError("no spline attached (attach_spline)")
        return tuple(self.spline.tables())

    def attach_camera_optimizers(self, col=None, evs=None):
        """From now on the pose tables come from per-camera optimisers on the composer's device by one launch in front of every
        ``compose()`` -- ``lse_pose_delta_tables``, the device-side counterpart of ``camera_tables`` -- over static copies of the
        scene's own poses taken here, so they are always those of the CURRENT ``pose_adjustment``, which the kernel reads in place.
        ``col``: a ``CameraOptimizer`` over the colour cameras (not with deblur rays: the reference's exist only with the spline,
        R:lse_nerf/lse_ray_generator.py:103-147).  ``evs``: "consec" pairing -- a ``CameraOptimizer`` for the one event table, which
        both bundles read (R:lse_nerf/lse_datamanager.py:363-364 applies one optimiser to both); "prevnext" pairing -- a
        ``PrevNextCamOptimizer`` (``prev_optim`` feeds prev, ``next_optim`` nxt) or a plain ``CameraOptimizer`` (one parameter block
        feeds both tables, each over its own base poses; its gradient is row(prev) + row(nxt)).
        ``non_trainable_camera_indices`` becomes a device mask.  An optimiser whose mode is "off" (frozen, or "delayed" before
        ``turn_on()``) is refused like a spline that is off; so is a table an attached spline feeds already (a spline on "col" beside
        per-camera optimisers on the event tables is fine).  ``set_poses`` on a fed table and ``compose(tables=...)`` then raise
        ValueError; ``delta_grads`` / ``delta_pose_tables`` are the way back to the parameters.  Returns the ``DeltaPoses``."""
        from .cameras import CameraOptimizer, PrevNextCamOptimizer
        from .pose_delta_dev import DeltaPoses, check_trainable
        if col is None and evs is None:
            raise ValueError("attach_camera_optimizers: give col=, evs= or both")
        scene = self.scene
        feeds = [None, None, None]
        if col is not None:
            if not self.n_col:
                raise ValueError("this composer has no 'col' pose table")
            if not isinstance(col, CameraOptimizer):
                raise ValueError("col= takes a CameraOptimizer (a spline is attached with attach_spline)")
            if self.G == 4:
                raise ValueError("deblur rays (G == 4) come from the spline only: a per-camera optimiser has one pose per camera")
            check_trainable(col, "'col'")
            if int(col.num_cameras) != scene.col.n_cameras:
                raise ValueError(f"the 'col' optimiser has {col.num_cameras} cameras, the colour table {scene.col.n_cameras}")
            feeds[0] = (col, scene.col.cameras.camera_to_worlds)
        if evs is not None:
            if not self.n_evs:
                raise ValueError("this composer has no 'prev' pose table")
            if isinstance(evs, PrevNextCamOptimizer):
                if self.consec:
                    raise ValueError("a PrevNextCamOptimizer needs event_pairing='prevnext': 'consec' has ONE event table")
                pair = (evs.prev_optim, evs.next_optim)
            elif isinstance(evs, CameraOptimizer):
                pair = (evs, None if self.consec else evs)
            else:
                raise ValueError("evs= takes a CameraOptimizer or a PrevNextCamOptimizer (a spline is attached with attach_spline)")
            sets = (scene.evs.cameras, None) if self.consec else (scene.prev_cameras, scene.next_cameras)
            for i, (o, cams) in enumerate(zip(pair, sets)):
                if o is None:
                    continue
                name = ("prev", "nxt")[i]
                check_trainable(o, f"'{name}'")
                if int(o.num_cameras) != len(cams):
                    raise ValueError(f"the '{name}' optimiser has {o.num_cameras} cameras, the table {len(cams)}")
                feeds[1 + i] = (o, cams.camera_to_worlds)
        if self.spline is not None and any(f is not None and sp for f, sp in zip(feeds, self.spline.fed)):
            raise ValueError("a pose table named here is already fed by the attached spline")
        shapes = [None if t is None or f is None else tuple(t.shape) for t, f in zip(self.pose_tables, feeds)]
        self.deltas = DeltaPoses(feeds, shapes, scene.device)
        return self.deltas

    def delta_grads(self, pose_grads, out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
        """``{block: [C, 6]}``: the gradients of the attached ``pose_adjustment`` parameters ("col", "prev", "nxt": a block carries the
        name of the first table it feeds) from the gradients of the pose tables, as ``spline_grads`` does for the spline.  One launch,
        no sums across threads (two calls are bit-equal, non-trainable cameras get exactly zero); the result lives in static tensors
        that the next call overwrites, or in ``out``."""
        if self.deltas is None:
            raise ValueError("no camera optimiser attached (attach_camera_optimizers)")
        if isinstance(pose_grads, dict):
            pose_grads = [pose_grads.get(k) for k in ("col", "prev", "next")]
        return self.deltas.backward(list(pose_grads), out=out)

    def delta_pose_tables(self):
        """``(col, prev, nxt)`` of the attached camera optimisers as NEW tensors with autograd history back to the parameters (None
        where they feed none): the eager, differentiable twin of what ``compose()`` writes into ``pose_tables``."""
        if self.deltas is None:
            raise ValueError("no camera optimiser attached (attach_camera_optimizers)")
        return tuple(self.deltas.tables())

    # -- launches
    def _given(self, indices):
        if indices is None:
            return None, None
        col_i, evs_i = indices
        fix = lambda t, n: None if t is None else torch.as_tensor(t).to(self.scene.device, torch.int32).reshape(n, 3).contiguous()
        return fix(col_i, self.n_col) if self.n_col else None, fix(evs_i, self.n_evs) if self.n_evs else None

    def _launch(self, step: Optional[int], indices) -> None:
        col_i, evs_i = self._given(indices)
        own = step is None
        if self.sampling is not None:          # the weighted draw of every stream no pixels were given for, in front of the advance
            drawn = []
            for w, given in zip(self._weighted, (col_i, evs_i)):
                if w is not None and given is None:
                    w.draw(step, self.step_dev, self.seed)
                    given = w.indices
                drawn.append(given)
            col_i, evs_i = drawn
        _lib.call("lse_compose_batch", ctypes.byref(self._desc), ctypes.byref(self._scene_desc), ctypes.byref(self._out_desc),
                  _ptr(self.step_dev) if own else None, 0 if own else int(step), int(own), _ptr(col_i), _ptr(evs_i), _stream())

    def compose(self, step: Optional[int] = None, indices=None, tables: Optional[Sequence[Optional[Tensor]]] = None):
        """One step's ``(col, prev, nxt), {"col_batch": ..., "evs_batch": ...}`` in the static buffers.
        ``step=None`` draws with the device step counter and advances it (a device-side action behind the launch); an explicit
        ``step`` leaves the counter alone.  ``indices=(col [n_col, 3], evs [n_evs, 3])`` int (c, y, x), either may be None: given
        pixels instead of the draw (values outside the scene are clamped into it).
        ``tables=(col, prev, nxt)``: pose tables as (differentiable) torch expressions -- they are copied into the static tables and
        the returned origins / directions carry autograd history back to them (new tensors; backward = ``lse_compose_rays_bwd``)."""
        if tables is None:
            if self.spline is not None:        # the tables of the spline's current parameters, in stream order in front of the rays
                self.spline.forward(self.pose_tables)
            if self.deltas is not None:        # ... and those of the per-camera optimisers' current parameters
                self.deltas.forward(self.pose_tables)
            self._launch(step, indices)
            return self.bundles, self.batch
        if self.spline is not None:
            raise ValueError("compose(tables=...) with a spline attached: the attached spline feeds the pose tables "
                             "(spline_pose_tables() is their differentiable twin)")
        if self.deltas is not None:
            raise ValueError("compose(tables=...) with a camera optimiser attached: the attached optimisers feed the pose tables "
                             "(delta_pose_tables() is their differentiable twin)")
        given = [t for t, own in zip(tables, self.pose_tables) if own is not None]
        if len(given) != sum(t is not None for t in self.pose_tables) or any(t is None for t in given):
            raise ValueError("tables= takes one tensor per pose table of this composer")
        if self.n_col and given[0].dim() == 3:
            given[0] = given[0][:, None].expand(-1, self.G, -1, -1)
        o, d = _ComposeRays.apply(self, step, indices, *given)
        return self._make_bundles(o, d), self.batch

    def _rays_bwd(self, d_o: Tensor, d_d: Tensor, ray_px: Optional[Tensor] = None, tables=None, static: bool = True):
        assert tuple(d_o.shape) == tuple(d_d.shape) == (self.n_rays, 3) and d_o.dtype == d_d.dtype == torch.float32
        assert d_o.is_contiguous() and d_d.is_contiguous()
        out = self._pose_grads if static else tuple(None if t is None else torch.empty_like(t) for t in self.pose_tables)
        od, sd = self._out_desc, self._scene_desc
        if ray_px is not None:
            od = _lib.ComposeOut.from_buffer_copy(od)
            od.ray_px = _ptr(ray_px)
        if tables is not None:
            sd = _lib.ComposeScene.from_buffer_copy(sd)
            sd.col_pose, sd.prev_pose, sd.next_pose = _ptr(tables[0]), _ptr(tables[1]), _ptr(tables[2])
        _lib.call("lse_compose_rays_bwd", ctypes.byref(self._desc), ctypes.byref(sd), ctypes.byref(od), _ptr(d_o), _ptr(d_d),
                  _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _stream())
        return out

    def pose_grads(self, ray_grads):
        """Gradients of the three pose tables (same shapes; None where there is no table) from the gradients w.r.t. the rays of the
        LAST composed step: ``ray_grads`` = ``(d_origins, d_directions)`` [n_rays, 3] over all bundles, or the per-bundle dictionary
        ``GraphedTrainStep.ray_grads`` holds.  Fixed-order sums: two calls are bit-equal; rows no ray touched are zero.  The result
        lives in static tensors that the next call overwrites."""
        if isinstance(ray_grads, dict):
            parts = [ray_grads[k] for k in ("col", "prev", "next") if ray_grads.get(k) is not None]
            ray_grads = (torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])) if len(parts) > 1 else parts[0]
        d_o, d_d = ray_grads
        return self._rays_bwd(d_o.contiguous(), d_d.contiguous())

    def indices_host(self, step: int) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
        """``(col, evs)`` int64 [n, 3] = (c, y, x): what the device draws at ``step`` (``draw_indices_host``; with ``sampling`` the
        weighted draw in host integers, over the row tables and the image rows it needs copied from the device -- a test and resume
        helper, not for the training loop)."""
        col, evs = self.scene.col, self.scene.evs
        if self.sampling is not None:
            return tuple(None if w is None else w.draw_host(self.seed, step)[0] for w in self._weighted)
        return (draw_indices_host(self.seed, step, 0, self.n_col, col.n_images, col.H, col.W) if self.n_col else None,
                draw_indices_host(self.seed, step, 1, self.n_evs, evs.n_images, evs.H, evs.W) if self.n_evs else None)


# ---------------------------------------------------------------------------------------------------- pose tables from cameras.py
def camera_tables(cameras: EdCameras, optimizer=None) -> Tensor:
    """[C, 3, 4]: the cameras' poses, with a ``CameraOptimizer``'s per-camera correction applied the way ``apply_to_raybundle``
    applies it to a ray (``cameras.py``: origins += t_corr, directions = R_corr @ directions): ``[R_corr R | t + t_corr]``."""
    c2w = cameras.camera_to_worlds
    if optimizer is None or optimizer.config.mode == "off":
        return c2w
    corr = optimizer(torch.arange(len(cameras), device=optimizer.pose_adjustment.device))
    c2w = c2w.to(corr.device)
    return torch.cat([corr[:, :3, :3] @ c2w[:, :3, :3], c2w[:, :3, 3:] + corr[:, :3, 3:]], dim=-1)


def spline_tables(spline, cameras: EdCameras, kind: str = "rgb") -> Tensor:
    """Pose tables from a ``SplineCameraOptimizer`` evaluated at every camera's time: "rgb" / "evs" -> [C, 3, 4]
    (``get_rgb_cameras`` / ``get_evs_cameras``), "deblur" -> [C, 4, 3, 4] (slot k = the k-th virtual camera of the exposure,
    ``get_deblur_cameras``).  Differentiable w.r.t. the spline's parameters."""
    times = cameras.times.to(spline.ctrl_ts.device)
    if kind == "deblur":
        return spline.get_deblur_cameras(times.reshape(-1, 1)).reshape(len(cameras), spline.n_deblur_rays, 3, 4)
    fn = {"rgb": spline.get_rgb_cameras, "evs": spline.get_evs_cameras}[kind]
    return fn(times.reshape(-1))
