#!/usr/bin/env python3
"""Checkpoint directory + scene directory -> the events an ideal sensor sees of the trained field along the scene's trajectory
(lsenerf_amd.events.simulate_events: log-intensity planes of the eval render, the sensor walk and the ordered stream on the device).

The checkpoint and configuration arguments are those of tools/export_mesh.py.  The trajectory is the spline through the colour
cameras of SCENE_DIR/colcam_set (their poses and times, as recorded: the checkpoint's pose refinement is not applied) times the
colour -> event transform of rel_cam.json; intrinsics, distortion and size are those of SCENE_DIR/ecam_set.  The poses are taken at
--times, or at --rate poses per unit of the cameras' time over the trajectory (or over --t0 .. --t1).  Writes the stream as .npz
(x, y int16; t float64; p int8; H, W) and, with --frames ECAM_DIR --frame-every S, the frames between every S-th pose as
ECAM_DIR/eimgs/eimgs_1x.npy (int8, saturated), which EventSceneReader reads back.

usage: python tools/simulate_events.py CKPT_DIR SCENE_DIR OUT.npz (--times t0,t1,... | --rate R [--t0 A] [--t1 B]) [--threshold C]
           [--threshold-neg C] [--cap-step 127] [--window 16] [--max-events N] [--unsorted] [--frames ECAM_DIR --frame-every S]
           [--appearance-id 0] [--step N] [--scale-factor 1.0] [--scene-scale 1.0] [--config name=value ...]"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def trajectory(scene_dir: str, times, rate, t0, t1, scale_factor: float, scene_scale: float, threshold):
    """``(event cameras, poses [n, 3, 4], times, threshold)`` of a scene directory: the spline through the colour cameras times the
    colour -> event transform, at ``times`` or at ``rate`` poses per unit of time over ``t0 .. t1`` (default: the whole trajectory);
    the threshold defaults to the scene's ``e_thresh``.  Host code only."""
    import numpy as np
    import torch
    from lsenerf_amd import events
    from lsenerf_amd.cameras import CameraOptimizerConfig, SplineCameraOptimizer
    from lsenerf_amd.scene_io import ColorSceneReader, EventSceneReader
    col = ColorSceneReader(os.path.join(scene_dir, "colcam_set"), scale_factor=scale_factor, scene_scale=scene_scale).outputs("train")
    evs = EventSceneReader(os.path.join(scene_dir, "ecam_set"), scale_factor=scale_factor, scene_scale=scene_scale).outputs("train")
    if col.cameras.times is None or col.dM is None:
        raise SystemExit("the colour cameras need times and the scene a rel_cam.json: the trajectory is a spline through them")
    threshold = threshold if threshold is not None else evs.e_thresh
    if threshold is None:
        raise SystemExit("the scene records no e_thresh: pass --threshold")
    cam_ts = col.cameras.times.reshape(-1).double()
    if times is None:
        t0 = float(cam_ts.min()) if t0 is None else t0
        t1 = float(cam_ts.max()) if t1 is None else t1
        n = int(math.floor((t1 - t0) * rate)) + 1
        if n < 2:
            raise SystemExit(f"--rate {rate} over {t0} .. {t1} gives fewer than two poses")
        times = (t0 + np.arange(n, dtype=np.float64) / rate).tolist()
    spline = SplineCameraOptimizer(CameraOptimizerConfig(mode="off", optim_type="spline"), len(col.cameras), "cpu", col.cameras,
                                   dM=col.dM)
    poses = events.spline_event_poses(spline, torch.tensor(times, dtype=torch.float32))
    cams = evs.prev_cameras if evs.prev_cameras is not None else evs.cameras
    return cams, poses, times, float(threshold)


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("checkpoint", help="a nerfstudio_models directory or a step-*.ckpt file")
    ap.add_argument("scene", help="the scene directory (holds colcam_set, ecam_set and rel_cam.json)")
    ap.add_argument("output", help="the .npz file to write")
    ap.add_argument("--times", default=None, help="comma-separated ascending pose times")
    ap.add_argument("--rate", type=float, default=None, help="poses per unit of the cameras' time")
    ap.add_argument("--t0", type=float, default=None)
    ap.add_argument("--t1", type=float, default=None)
    ap.add_argument("--threshold", type=float, default=None, help="contrast threshold (default: the scene's e_thresh)")
    ap.add_argument("--threshold-neg", type=float, default=None)
    ap.add_argument("--cap-step", type=int, default=127)
    ap.add_argument("--window", type=int, default=16)
    ap.add_argument("--max-events", type=int, default=None)
    ap.add_argument("--unsorted", action="store_true", help="keep the stream order (interval, pixel, emission)")
    ap.add_argument("--frames", default=None, metavar="ECAM_DIR")
    ap.add_argument("--frame-every", type=int, default=None, metavar="S")
    ap.add_argument("--appearance-id", type=int, default=0)
    ap.add_argument("--step", type=int, default=None)
    ap.add_argument("--scale-factor", type=float, default=1.0)
    ap.add_argument("--scene-scale", type=float, default=1.0, help="half extent of the scene box the model was built with")
    ap.add_argument("--num-train-data", type=int, default=None)
    ap.add_argument("--config", action="append", default=[], metavar="name=value")
    args = ap.parse_args(argv)

    if (args.times is None) == (args.rate is None):
        raise SystemExit("give --times or --rate (one of them)")
    times = None
    if args.times is not None:
        times = [float(v) for v in args.times.split(",")]
        if len(times) < 2 or any(b <= a for a, b in zip(times, times[1:])) or not all(math.isfinite(v) for v in times):
            raise SystemExit("--times: at least two finite, strictly ascending times")
    elif not (args.rate > 0 and math.isfinite(args.rate)):
        raise SystemExit("--rate must be positive and finite")
    for name, v in (("--threshold", args.threshold), ("--threshold-neg", args.threshold_neg)):
        if v is not None and not (v > 0 and math.isfinite(v)):
            raise SystemExit(f"{name} must be positive and finite")
    if (args.frames is None) != (args.frame_every is None):
        raise SystemExit("--frames needs --frame-every, and the other way round")
    if args.frame_every is not None and args.frame_every < 1:
        raise SystemExit("--frame-every must be at least 1")

    import torch
    from lsenerf_amd import LSENeRFModel, checkpoint, events
    from export_mesh import parse_config, train_images_in

    s = float(args.scene_scale)
    cams, poses, times, threshold = trajectory(args.scene, times, args.rate, args.t0, args.t1, args.scale_factor, s, args.threshold)
    n_train = args.num_train_data if args.num_train_data is not None else train_images_in(args.checkpoint, args.step)
    model = LSENeRFModel(parse_config(args.config), torch.tensor([[-s, -s, -s], [s, s, s]]), n_train).cuda()
    info = checkpoint.load_nerfstudio_checkpoint(args.checkpoint, model, load_step=args.step, drop_camera_optimizer=True)
    field_missing = [k for k in info["missing"] if k.startswith("field.")]
    if field_missing:
        raise SystemExit(f"the checkpoint does not fill the field ({field_missing[:4]} ...): does --config match the training run?")
    stream, _, total = model.simulate_events(cams, poses, times, threshold, threshold_neg=args.threshold_neg, window=args.window,
                                             cap_step=args.cap_step, max_events=args.max_events, sort=not args.unsorted,
                                             appearance_id=args.appearance_id)
    stream.write_npz(args.output)
    dropped = f" ({total - len(stream)} beyond --max-events dropped)" if total > len(stream) else ""
    print(f"step {info['step']}: {len(stream)} events{dropped} from {len(times)} poses at threshold {threshold:g} -> {args.output}")
    if args.frames is not None:
        bounds = times[::args.frame_every]
        if len(bounds) < 2:
            raise SystemExit("--frame-every leaves fewer than two bounds")
        frames = events.accumulate_events(stream, bounds)
        path = events.write_event_frames(args.frames, frames)
        print(f"{frames.shape[0]} frames of {frames.shape[1]} x {frames.shape[2]} -> {path}")


if __name__ == "__main__":
    main()
