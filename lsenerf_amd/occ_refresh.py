"""Count-free occupancy-grid refresh: ``LSEOccGridEstimator._update`` with every size kept on the device.

The eager ``_update`` sizes tensors from device values (``torch.nonzero``, two boolean-mask gathers, a density pass over a row
count only the host knows), so every refresh blocks the host several times and cannot be captured.  ``DeviceGridRefresher`` runs
the same update rule through csrc/occ_refresh.hip: the occupied cells are listed by an ordered compaction, the cells of a level are
drawn into a DENSE slot layout whose length lives in ``n_dev``, the field evaluates them through its count-free entry points, the
EMA-max reads ``n_dev``, and the mean / threshold come from one deterministic reduction that also rewrites the estimator's
device-side ``occs.mean()`` in place.  Nothing synchronises, so the whole refresh captures into one HIP graph per branch:

    refresher = DeviceGridRefresher(model.occupancy_grid, model.field, render_step_size)
    refresher.capture()                      # optional: one graph for the warm-up branch, one for the sampled branch
    refresher.refresh(step)                  # between two replays of the training step, on the same stream

Sampling convention (this package's own, like the batch composer's): slot ``i`` of level ``l`` at step ``s`` takes ONE Philox4x32-10
call, key ``(update_seed & 0xffffffff, update_seed >> 32)``, counter ``(s & 0xffffffff, i, l, 0)``.  Word 0 picks the cell
(``mulhi32(w0, cnt)`` into the occupied list, ``mulhi32(w0, C)`` for a uniform cell), words 1..3 give the in-cell jitter
``u = (w >> 8) * 2^-24``.  Uniform with replacement like nerfacc's ``torch.randint``; no bit parity with ``torch.Generator``.
Slot layout of the sampled branch (``N = C // 4``, ``cnt`` occupied cells, ``m = min(cnt, N)``): ``[0, m)`` occupied cells (the
whole list when ``cnt <= N``), ``[m, m + N)`` uniform cells, ``n = m + N``.  Warm-up branch: slot ``i`` is cell ``i``, ``n = C``.
A cell whose ``occs < 0`` keeps its slot with id ``-1``: it is evaluated (at its own, in-bounds position) and the EMA skips it.
``draw_cells_host`` is this specification in numpy; the device draw is tested against it bit for bit.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib, ops
from .data import philox4x32_10


def draw_cells_host(seed: int, step: int, level: int, cells: int, res: Sequence[int], aabb: Sequence[float], warmup: bool,
                    occs_level: Optional[np.ndarray] = None, occupied: Optional[np.ndarray] = None
                    ) -> Tuple[np.ndarray, np.ndarray, int]:
    """The draw of one level on the host: ``(cell_ids int64 [n], positions float32 [n, 3], n)`` (module docstring).
    ``aabb``: the level's (lo, hi) box; ``occs_level``: float32 [cells] (cells with a negative value get id -1; None: none has);
    ``occupied``: ascending indices of the level's set cells (sampled branch).  Integer arithmetic is exact and every float32
    operation is rounded on its own, as in the kernel."""
    cells = int(cells)
    n_quarter = cells // 4
    if warmup:
        cnt = m = 0
        n = cells
    else:
        occupied = np.asarray(occupied if occupied is not None else [], dtype=np.int64)
        cnt = int(occupied.shape[0])
        m = min(cnt, n_quarter)
        n = m + n_quarter
    ctr = np.zeros((n, 4), dtype=np.uint32)
    ctr[:, 0] = int(step) & 0xFFFFFFFF
    ctr[:, 1] = np.arange(n, dtype=np.uint32)
    ctr[:, 2] = int(level)
    w = philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    w0 = w[:, 0].astype(np.uint64)
    if warmup:
        idx = np.arange(n, dtype=np.int64)
    else:
        idx = ((w0 * np.uint64(cells)) >> np.uint64(32)).astype(np.int64)
        if cnt <= n_quarter:
            idx[:m] = occupied
        else:
            idx[:m] = occupied[((w0[:m] * np.uint64(cnt)) >> np.uint64(32)).astype(np.int64)]
    rx, ry, rz = (int(r) for r in res)
    coord = np.stack([idx // (rz * ry), (idx // rz) % ry, idx % rz], -1).astype(np.float32)
    u = (w[:, 1:4] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    box = np.asarray(aabb, dtype=np.float32).reshape(6)
    lo, hi = box[:3], box[3:]
    x = (coord + u) / np.array([rx, ry, rz], dtype=np.float32)
    positions = (lo + x * (hi - lo)).astype(np.float32)
    ids = int(level) * cells + idx
    if occs_level is not None:
        ids = np.where(np.asarray(occs_level)[idx] < 0, np.int64(-1), ids)
    return ids.astype(np.int64), positions, n


def mean_and_threshold_host(occs: np.ndarray, occ_thre: float) -> Tuple[float, float]:
    """``(occs.mean(), min(occs[occs >= 0].mean(), occ_thre))`` in float64: what lse_occ_mean_threshold rounds to float32."""
    o = np.asarray(occs, dtype=np.float64).reshape(-1)
    pos = o[o >= 0]
    mean_pos = float(pos.sum() / pos.size) if pos.size else float("nan")
    return float(o.sum() / o.size), (mean_pos if not mean_pos > occ_thre else float(occ_thre))


class DeviceGridRefresher:
    """``estimator._update(step, lambda x: density(x) * render_step_size, occ_thre, ema_decay, warmup_steps)`` without a host
    synchronisation (module docstring).

    ``density``: an ``LSEField`` -- evaluated count-free through ``density_packed(p, None, ..., n_dev)`` -- or any callable
    ``positions [cap, 3] -> density [cap] / [cap, 1]``, evaluated over the whole capacity (rows beyond ``n_dev`` are ignored).
    Levels are processed one after another into buffers allocated here, once: ``C`` rows when there is a warm-up branch, else
    ``2 * (C // 4)`` (the eager route holds int64 coordinates, jitter and positions of a whole level on top of that)."""

    def __init__(self, estimator, density: Union[Callable[[Tensor], Tensor], object], render_step_size: float,
                 occ_thre: float = 1e-2, ema_decay: float = 0.95, warmup_steps: int = 256) -> None:
        from .field import LSEField
        self.estimator = estimator
        self.density = density
        self._field = density if isinstance(density, LSEField) else None
        self.render_step_size, self.occ_thre = float(render_step_size), float(occ_thre)
        self.ema_decay, self.warmup_steps = float(ema_decay), int(warmup_steps)
        dev = estimator.occs.device
        if dev.type != "cuda":
            raise _lib.LseHipError(f"DeviceGridRefresher needs the grid on the GPU (got {dev}); the HIP path has no CPU fallback")
        L, C = estimator.levels, estimator.cells_per_lvl
        if L > _lib.LSE_MAX_OCC_LEVELS or not 4 <= C < 1 << 31:
            raise ValueError(f"DeviceGridRefresher: {L} levels of {C} cells are outside the kernels' limits")
        self._res = tuple(int(v) for v in estimator.resolution.tolist())       # (one read-back, at construction)
        if self._field is not None and self._field._contraction != "inf":
            self._field._aabb_list()                                           # (cached host copy: read now, not in refresh())
        self._cap = {True: C, False: 2 * (C // 4)}
        cap = C if self.warmup_steps > 0 else self._cap[False]
        i32, i64, f32 = torch.int32, torch.int64, torch.float32
        self.cell_list = torch.zeros((L, C), dtype=i32, device=dev)
        self.counts = torch.zeros(L, dtype=i64, device=dev)
        self._list_ws = torch.zeros(L * ops.occ_list_tiles(C), dtype=i32, device=dev)
        self.cell_ids = torch.full((cap,), -1, dtype=i64, device=dev)
        self.positions = torch.zeros((cap, 3), dtype=f32, device=dev)
        self.n_dev = torch.zeros(1, dtype=i64, device=dev)
        self._ema_ws = torch.zeros(cap, dtype=f32, device=dev)
        self._mean_ws = torch.zeros(3 * _lib.LSE_OCC_MEAN_BLOCKS, dtype=torch.float64, device=dev)
        self.threshold = torch.zeros(1, dtype=f32, device=dev)
        self.step_dev = torch.zeros(1, dtype=i64, device=dev)
        estimator._occ_mean_device()                                           # the buffer lse_occ_mean_threshold rewrites in place
        self._graphs: Dict[bool, torch.cuda.CUDAGraph] = {}

    # ---------------------------------------------------------------------------------------------
    def _is_warmup(self, step: int) -> bool:
        return int(step) < self.warmup_steps

    def list_occupied(self) -> None:
        """``cell_list`` / ``counts`` of the grid's current ``binaries`` (sampled branch: once per refresh)."""
        est = self.estimator
        ops.occ_list_occupied(est._binaries_u8().view(est.levels, est.cells_per_lvl), self.cell_list, self.counts, self._list_ws)

    def draw_level(self, level: int, warmup: bool) -> Tuple[Tensor, Tensor]:
        """Draw the cells of ``level`` at the step in ``step_dev``: ``(cell_ids [cap], positions [cap, 3])`` -- views of the
        refresher's buffers of the branch's capacity, valid up to ``n_dev`` -- from the list ``list_occupied`` left."""
        est = self.estimator
        cap = self._cap[bool(warmup)]
        if cap > self.cell_ids.shape[0]:
            raise ValueError("this refresher was built without a warm-up branch (warmup_steps = 0)")
        ids, pos = self.cell_ids[:cap], self.positions[:cap]
        ops.occ_draw_cells(est.occs, self.cell_list, self.counts, est.aabbs, level, est.cells_per_lvl, self._res, warmup,
                           self.step_dev, est.update_seed, ids, pos, self.n_dev)
        return ids, pos

    @torch.no_grad()
    def _density(self, positions: Tensor) -> Tensor:
        if self._field is not None:
            sigma = self._field.density_packed(positions, None, None, None, None, None, self.n_dev)[0]
        else:
            sigma = self.density(positions)
        sigma = sigma.reshape(-1)
        if sigma.shape[0] != positions.shape[0]:
            raise ValueError(f"density returned {sigma.shape[0]} values for {positions.shape[0]} positions")
        return sigma.float().contiguous()

    @torch.no_grad()
    def _body(self, warmup: bool) -> None:
        """One refresh at the step in ``step_dev``: launches only, nothing waits for the device."""
        est = self.estimator
        if not warmup:
            self.list_occupied()
        for level in range(est.levels):
            ids, pos = self.draw_level(level, warmup)
            ops.occ_update_cells_dev(est.occs, ids, self._density(pos), self.render_step_size, self.n_dev, self.ema_decay,
                                     self._ema_ws)
        ops.occ_mean_threshold(est.occs, self.occ_thre, self._mean_ws, est.__dict__["_occ_mean_dev"], self.threshold)
        ops.occ_binarize(est.occs, self.threshold, est._binaries_u8().view(-1))

    def _after(self) -> None:
        """The host bookkeeping of ``_update``.  The device-side mean is already new (written in place by the reduction)."""
        est = self.estimator
        est._bump_grid_version()
        est._occ_mean_host = None
        est.__dict__["_occ_mean_dev_version"] = est.occs._version
        hook = getattr(est, "after_update_hook", None)
        if hook is not None:
            hook()

    # ---------------------------------------------------------------------------------------------
    def refresh(self, step: int) -> None:
        """Refresh the grid as update ``step``: replays the branch's graph when ``capture()`` has run, else launches eagerly.
        Either way the host waits for nothing (``torch.cuda.set_sync_debug_mode("error")`` passes)."""
        warmup = self._is_warmup(step)
        self.step_dev.fill_(int(step))              # (a scalar launch argument: no host buffer a later call could overwrite)
        graph = self._graphs.get(warmup)
        if graph is not None:
            graph.replay()
        else:
            self._body(warmup)
        self._after()

    def capture(self, warmup_runs: int = 2) -> "DeviceGridRefresher":
        """Record one HIP graph per branch (``graph.capture_body``).  The warm-up runs and nothing else of a capture execute, and
        they do modify the grid: ``occs``, ``binaries`` and the device-side mean are saved before and restored after, so
        capturing refreshes nothing.  The graphs share one memory pool -- they never run at the same time."""
        from .graph import capture_body
        est = self.estimator
        mean = est._occ_mean_device()
        saved = (est.occs.clone(), est.binaries.clone(), mean.clone(), self.step_dev.clone())
        stream = torch.cuda.Stream(device=est.occs.device)
        pool = None
        for warmup in ([True, False] if self.warmup_steps > 0 else [False]):
            self.step_dev.fill_(0 if warmup else self.warmup_steps)
            g = capture_body(lambda w=warmup: self._body(w), None, est, warmup=warmup_runs, pool=pool, stream=stream)
            pool = g.pool()
            self._graphs[warmup] = g
        with torch.no_grad():
            est.occs.copy_(saved[0])
            est.binaries.copy_(saved[1])
            mean.copy_(saved[2])
            self.step_dev.copy_(saved[3])
        est.__dict__["_occ_mean_dev_version"] = est.occs._version
        return self

    @property
    def captured(self) -> bool:
        return bool(self._graphs)
