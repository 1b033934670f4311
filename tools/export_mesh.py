#!/usr/bin/env python3
"""Checkpoint directory -> triangle mesh (.ply) of the trained field's density isosurface, with analytic normals and optional
vertex colours (lsenerf_amd.mesh.extract_mesh: surface nets on the device).

A nerfstudio checkpoint holds weights, not the model configuration: give the configuration the run was trained with as
``--config name=value`` pairs (fields of LSENeRFModelConfig; values are parsed as Python literals where they are one).  The number
of training images is read from the appearance-embedding table in the checkpoint unless ``--num-train-data`` says otherwise.

usage: python tools/export_mesh.py CKPT_DIR OUT.ply [--step N] [--resolution 256 | --resolution 256,256,128] [--level 10]
           [--bounds x0,y0,z0,x1,y1,z1] [--colors] [--no-normals] [--chunk 4194304] [--scene-scale 1.0] [--config name=value ...]"""
import argparse
import ast
import dataclasses
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig, checkpoint
from lsenerf_amd.mesh import DEFAULT_LEVEL, write_ply


def parse_config(pairs) -> LSENeRFModelConfig:
    names = {f.name for f in dataclasses.fields(LSENeRFModelConfig)}
    kw = {}
    for pair in pairs:
        name, _, value = pair.partition("=")
        if name not in names:
            raise SystemExit(f"--config {pair}: LSENeRFModelConfig has no field {name!r}")
        try:
            kw[name] = ast.literal_eval(value)
        except (ValueError, SyntaxError):
            kw[name] = value
    return LSENeRFModelConfig(**kw)


def train_images_in(path: str, step) -> int:
    if os.path.isdir(path):
        path = checkpoint.checkpoint_path(path, checkpoint.latest_step(path) if step is None else int(step))
    state, _ = checkpoint.convert_pipeline_state(torch.load(path, map_location="cpu", weights_only=True)["pipeline"])
    rows = [v.shape[0] for k, v in state.items() if k.endswith("embedding_appearance.embedding.weight")]
    if not rows:
        raise SystemExit("the checkpoint has no appearance-embedding table: pass --num-train-data")
    return int(rows[0])


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("checkpoint", help="a nerfstudio_models directory or a step-*.ckpt file")
    ap.add_argument("output", help="the .ply file to write")
    ap.add_argument("--step", type=int, default=None)
    ap.add_argument("--resolution", default="256")
    ap.add_argument("--level", type=float, default=DEFAULT_LEVEL)
    ap.add_argument("--bounds", default=None)
    ap.add_argument("--colors", action="store_true")
    ap.add_argument("--no-normals", action="store_true")
    ap.add_argument("--chunk", type=int, default=1 << 22)
    ap.add_argument("--scene-scale", type=float, default=1.0, help="half extent of the scene box the model was built with")
    ap.add_argument("--num-train-data", type=int, default=None)
    ap.add_argument("--config", action="append", default=[], metavar="name=value")
    args = ap.parse_args()

    res = [int(v) for v in args.resolution.split(",")]
    if len(res) not in (1, 3):
        raise SystemExit("--resolution: one count or three")
    bounds = None
    if args.bounds is not None:
        b = [float(v) for v in args.bounds.split(",")]
        if len(b) != 6:
            raise SystemExit("--bounds: x0,y0,z0,x1,y1,z1")
        bounds = (b[:3], b[3:])
    n_train = args.num_train_data if args.num_train_data is not None else train_images_in(args.checkpoint, args.step)
    s = float(args.scene_scale)
    model = LSENeRFModel(parse_config(args.config), torch.tensor([[-s, -s, -s], [s, s, s]]), n_train).cuda()
    info = checkpoint.load_nerfstudio_checkpoint(args.checkpoint, model, load_step=args.step, drop_camera_optimizer=True)
    field_missing = [k for k in info["missing"] if k.startswith("field.")]
    if field_missing:
        raise SystemExit(f"the checkpoint does not fill the field ({field_missing[:4]} ...): does --config match the training run?")
    mesh = model.extract_mesh(resolution=res[0] if len(res) == 1 else tuple(res), level=args.level, bounds=bounds,
                              normals=not args.no_normals, colors=args.colors, chunk=args.chunk)
    write_ply(args.output, mesh)
    print(f"step {info['step']}: {mesh.vertices.shape[0]} vertices, {mesh.triangles.shape[0]} triangles -> {args.output}")


if __name__ == "__main__":
    main()
