#!/usr/bin/env python3
"""Checkpoint directory + scene directory -> point cloud (.ply) of what the scene's colour cameras see of the trained field
(lsenerf_amd.pointcloud.export_point_cloud: unprojected eval renders, merged per voxel, floaters removed by neighbour support -- on
the device).

The checkpoint and configuration arguments are those of tools/export_mesh.py.  The cameras are the colour set of SCENE_DIR (the
directory that holds ``colcam_set``) read through ``lsenerf_amd.scene_io`` and made resident as an ``EvalSet``; the export needs
their poses and intrinsics only, so no image file is opened.

usage: python tools/export_pointcloud.py CKPT_DIR SCENE_DIR OUT.ply [--step N] [--split val] [--images 0,4,8] [--min-accumulation 0.9]
           [--voxel-size 0.01] [--min-support 4] [--bounds x0,y0,z0,x1,y1,z1] [--no-colors] [--no-normals] [--max-points N]
           [--depth expected|median] [--max-depth-spread D]
           [--scale-factor 1.0] [--scene-scale 1.0] [--config name=value ...]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
from lsenerf_amd import EvalSet, LSENeRFModel, checkpoint
from lsenerf_amd.pointcloud import write_ply_points
from lsenerf_amd.scene_io import ColorSceneReader
from export_mesh import parse_config, train_images_in


def scene_eval_set(scene_dir: str, split: str, scale_factor: float, scene_scale: float, device="cuda") -> EvalSet:
    """The colour cameras of ``split`` as an ``EvalSet`` (INTEGRATION.md, E') with blank images: rays need poses and intrinsics only."""
    out = ColorSceneReader(os.path.join(scene_dir, "colcam_set"), scale_factor=scale_factor, scene_scale=scene_scale).outputs(split)
    cams = out.cameras
    blank = torch.zeros((len(cams), cams.height, cams.width, 3), dtype=torch.uint8)
    return EvalSet(device, blank, cams, appearance_ids=out.appearance_ids)


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("checkpoint", help="a nerfstudio_models directory or a step-*.ckpt file")
    ap.add_argument("scene", help="the scene directory (holds colcam_set)")
    ap.add_argument("output", help="the .ply file to write")
    ap.add_argument("--step", type=int, default=None)
    ap.add_argument("--split", default="val", choices=("train", "val", "test"))
    ap.add_argument("--images", default=None, help="comma-separated image indices of the split (default: all)")
    ap.add_argument("--min-accumulation", type=float, default=0.9)
    ap.add_argument("--voxel-size", type=float, default=None)
    ap.add_argument("--min-support", type=int, default=0)
    ap.add_argument("--bounds", default=None)
    ap.add_argument("--no-colors", action="store_true")
    ap.add_argument("--no-normals", action="store_true")
    ap.add_argument("--max-points", type=int, default=None)
    ap.add_argument("--depth", default="expected", choices=("expected", "median"),
                    help="the depth that is unprojected: the render's expected depth, or the depth at which the accumulated weight "
                         "crosses one half")
    ap.add_argument("--max-depth-spread", type=float, default=None,
                    help="with --depth median: drop rays whose 0.25 and 0.75 quantile depths lie further apart (world units)")
    ap.add_argument("--scale-factor", type=float, default=1.0)
    ap.add_argument("--scene-scale", type=float, default=1.0, help="half extent of the scene box the model was built with")
    ap.add_argument("--num-train-data", type=int, default=None)
    ap.add_argument("--config", action="append", default=[], metavar="name=value")
    args = ap.parse_args(argv)

    bounds = None
    if args.bounds is not None:
        b = [float(v) for v in args.bounds.split(",")]
        if len(b) != 6:
            raise SystemExit("--bounds: x0,y0,z0,x1,y1,z1")
        bounds = (b[:3], b[3:])
    images = None if args.images is None else [int(v) for v in args.images.split(",")]
    if args.min_support > 0 and args.voxel_size is None:
        raise SystemExit("--min-support needs --voxel-size")
    n_train = args.num_train_data if args.num_train_data is not None else train_images_in(args.checkpoint, args.step)
    s = float(args.scene_scale)
    model = LSENeRFModel(parse_config(args.config), torch.tensor([[-s, -s, -s], [s, s, s]]), n_train).cuda()
    info = checkpoint.load_nerfstudio_checkpoint(args.checkpoint, model, load_step=args.step, drop_camera_optimizer=True)
    field_missing = [k for k in info["missing"] if k.startswith("field.")]
    if field_missing:
        raise SystemExit(f"the checkpoint does not fill the field ({field_missing[:4]} ...): does --config match the training run?")
    eval_set = scene_eval_set(args.scene, args.split, args.scale_factor, s)
    cloud = model.export_point_cloud(eval_set, image_indices=images, min_accumulation=args.min_accumulation, bounds=bounds,
                                     voxel_size=args.voxel_size, min_support=args.min_support, normals=not args.no_normals,
                                     colors=not args.no_colors, max_points=args.max_points, depth=args.depth,
                                     max_depth_spread=args.max_depth_spread)
    write_ply_points(args.output, cloud)
    views = len(eval_set) if images is None else len(images)
    print(f"step {info['step']}: {cloud.points.shape[0]} points from {views} views -> {args.output}")


if __name__ == "__main__":
    main()
