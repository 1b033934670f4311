#!/usr/bin/env python3
"""Checkpoint directory + scene directory -> triangle mesh (.ply) of the surface the scene's colour cameras see of the trained field
(lsenerf_amd.tsdf.export_tsdf_mesh: eval depth renders fused into a truncated signed distance volume, surface nets that build no
surface against unobserved space, fused colours and analytic normals -- on the device).

The checkpoint and configuration arguments are those of tools/export_mesh.py; the cameras are read as in tools/export_pointcloud.py
(the colour set of SCENE_DIR; poses and intrinsics only, no image file is opened).

usage: python tools/export_tsdf_mesh.py CKPT_DIR SCENE_DIR OUT.ply [--step N] [--split val] [--images 0,4,8] [--resolution 256]
           [--truncation T] [--min-accumulation 0.5] [--no-carve] [--min-weight 1] [--colors fused|field|none] [--no-normals]
           [--bounds x0,y0,z0,x1,y1,z1] [--views-per-launch 8] [--depth expected|median] [--max-depth-spread D]
           [--scale-factor 1.0] [--scene-scale 1.0] [--config name=value ...]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
from lsenerf_amd import LSENeRFModel, checkpoint
from lsenerf_amd.mesh import write_ply
from export_mesh import parse_config, train_images_in
from export_pointcloud import scene_eval_set


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("checkpoint", help="a nerfstudio_models directory or a step-*.ckpt file")
    ap.add_argument("scene", help="the scene directory (holds colcam_set)")
    ap.add_argument("output", help="the .ply file to write")
    ap.add_argument("--step", type=int, default=None)
    ap.add_argument("--split", default="val", choices=("train", "val", "test"))
    ap.add_argument("--images", default=None, help="comma-separated image indices of the split, in fusion order (default: all)")
    ap.add_argument("--resolution", default="256", help="cells per axis: one int or nx,ny,nz")
    ap.add_argument("--truncation", type=float, default=None, help="world units (default: 3 x the longest voxel edge)")
    ap.add_argument("--min-accumulation", type=float, default=0.5)
    ap.add_argument("--no-carve", action="store_true", help="ignore see-through pixels instead of marking their rays as empty")
    ap.add_argument("--min-weight", type=float, default=1)
    ap.add_argument("--colors", default="fused", choices=("fused", "field", "none"))
    ap.add_argument("--no-normals", action="store_true")
    ap.add_argument("--bounds", default=None)
    ap.add_argument("--views-per-launch", type=int, default=8)
    ap.add_argument("--depth", default="expected", choices=("expected", "median"),
                    help="the depth that is fused: the render's expected depth, or the depth at which the accumulated weight crosses one half")
    ap.add_argument("--max-depth-spread", type=float, default=None,
                    help="with --depth median: skip pixels whose 0.25 and 0.75 quantile depths lie further apart (world units)")
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
    res = [int(v) for v in args.resolution.split(",")]
    if len(res) not in (1, 3):
        raise SystemExit("--resolution: one int or nx,ny,nz")
    images = None if args.images is None else [int(v) for v in args.images.split(",")]
    n_train = args.num_train_data if args.num_train_data is not None else train_images_in(args.checkpoint, args.step)
    s = float(args.scene_scale)
    model = LSENeRFModel(parse_config(args.config), torch.tensor([[-s, -s, -s], [s, s, s]]), n_train).cuda()
    info = checkpoint.load_nerfstudio_checkpoint(args.checkpoint, model, load_step=args.step, drop_camera_optimizer=True)
    field_missing = [k for k in info["missing"] if k.startswith("field.")]
    if field_missing:
        raise SystemExit(f"the checkpoint does not fill the field ({field_missing[:4]} ...): does --config match the training run?")
    eval_set = scene_eval_set(args.scene, args.split, args.scale_factor, s)
    mesh = model.export_tsdf_mesh(eval_set, image_indices=images, resolution=res[0] if len(res) == 1 else tuple(res), bounds=bounds,
                                  truncation=args.truncation, min_accumulation=args.min_accumulation, carve=not args.no_carve,
                                  min_weight=args.min_weight, colors=None if args.colors == "none" else args.colors,
                                  normals=not args.no_normals, views_per_launch=args.views_per_launch, depth=args.depth,
                                  max_depth_spread=args.max_depth_spread)
    write_ply(args.output, mesh)
    views = len(eval_set) if images is None else len(images)
    print(f"step {info['step']}: {mesh.vertices.shape[0]} vertices, {mesh.triangles.shape[0]} triangles from {views} views -> {args.output}")


if __name__ == "__main__":
    main()
