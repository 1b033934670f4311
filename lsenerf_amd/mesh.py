"""Mesh export: the trained field's density on a lattice, its surface-nets isosurface (``ops.surface_nets``: one vertex per active
cell, one quad per sign-changing interior lattice edge; include/lse_hip.h, "mesh export"), analytic normals and optional colours at
the vertices, and a binary PLY writer.  Everything but the file stays on the device; the only host read is the pair of totals between
the two surface-nets passes."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import ops

DEFAULT_LEVEL = 10.0      # density iso value: a few render steps of this density are opaque at the scales the presets train at


@dataclass
class Mesh:
    vertices: Tensor                   # [V, 3] float32, world coordinates
    triangles: Tensor                  # [T, 3] int32 vertex ids; the geometric normal points from high to low density
    normals: Optional[Tensor] = None   # [V, 3] float32: unit vectors, zero where the density gradient is
    colors: Optional[Tensor] = None    # [V, 3] float32 in [0, 1]


def _bounds(field, bounds) -> Tuple[list, list]:
    b = field.aabb if bounds is None else bounds
    b = torch.as_tensor(b, dtype=torch.float32).detach().cpu().reshape(2, 3)
    lo, hi = [float(v) for v in b[0]], [float(v) for v in b[1]]
    if not all(h > l for l, h in zip(lo, hi)):
        raise ValueError(f"bounds {lo} .. {hi}: an empty box")
    return lo, hi


def _chunks(n: int, chunk: int):
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"chunk {chunk} < 1")
    return ((lo, min(n, lo + chunk)) for lo in range(0, n, chunk))


@torch.no_grad()
def density_lattice(field, res, lo, hi, chunk: int = 1 << 22) -> Tensor:
    """Density [points] (float32, iz fastest) of ``field`` at the points of the ``res``-cell lattice over ``lo .. hi``, filled in chunks
    of ``chunk`` points: ``lattice_positions`` then the field's density route (what ``density_fn`` runs).  The per-sample kernels do
    not look at their neighbours, so the chunk size does not change a bit."""
    n = ops.lattice_points(res)
    dev = field.aabb.device
    sigma = torch.empty(n, dtype=torch.float32, device=dev)
    for a, b in _chunks(n, chunk):
        pos = ops.lattice_positions(res, lo, hi, a, b - a, device=dev)
        sigma[a:b] = field.density_packed(pos, None, None, None, None, None)[0]
    return sigma


@torch.no_grad()
def vertex_normals(field, vertices: Tensor, chunk: int = 1 << 22) -> Tensor:
    """World-space analytic normals [V, 3] at ``vertices``: ``LSEField.normals_packed`` then ``ops.point_normals_world``, chunked."""
    contraction = field._contraction == "inf"
    aabb6 = None if contraction else field._aabb_list()
    out = torch.empty_like(vertices)
    for a, b in _chunks(vertices.shape[0], chunk):
        v = vertices[a:b]
        x01, _, y = field._encode_packed(v, None, None, None, None, None)
        ops.point_normals_world(field.normals_packed(x01, y), v, contraction, aabb6, out=out[a:b])
    return out


def eval_colour_mapping(model, radiance: Tensor) -> Tensor:
    """What the model's eval-mode ``get_outputs`` does to the composited colour of a ray, applied to ``radiance [n, 3]``:
    ``render_packed``'s NaN removal and clamp (skipped by a linear renderer), then ``route_outputs`` (mappers by map_mode, clamp)."""
    from .renderer import LinearRenderer
    if not isinstance(model.renderer_rgb, LinearRenderer):
        radiance = torch.clamp(torch.nan_to_num(radiance), 0.0, 1.0)
    return model.route_outputs({"rgb": radiance}, None)["rgb"]


@torch.no_grad()
def vertex_colors(model, vertices: Tensor, normals: Tensor, chunk: int = 1 << 22) -> Tensor:
    """Colours [V, 3] at ``vertices``: the field's RGB head seen along ``-normal`` (``(0, 0, 1)`` where the normal is zero) with the
    eval embedding, through ``eval_colour_mapping``."""
    field = model.field
    out = torch.empty_like(vertices)
    for a, b in _chunks(vertices.shape[0], chunk):
        v, n = vertices[a:b], normals[a:b]
        dirs = torch.where((n == 0).all(-1, keepdim=True), n.new_tensor([0.0, 0.0, 1.0]), -n).contiguous()
        _, h, _ = field.density_packed(v, None, None, None, None, None)
        table, eidx = field._eval_emb(b - a, v.device)
        rgb = field.rgb_packed(h, dirs, eidx, None, None, table)[:, :3]
        out[a:b] = eval_colour_mapping(model, rgb)
    return out


def extract_mesh(model, resolution=256, level: float = DEFAULT_LEVEL, bounds=None, normals: bool = True, colors: bool = False,
                 chunk: int = 1 << 22) -> Mesh:
    """Triangle mesh of the density isosurface ``sigma == level`` of ``model.field`` inside ``bounds`` ([2, 3]: lowest and highest
    corner; default: the field's aabb) on a lattice of ``resolution`` cells (an int or three).  Runs without gradients in eval mode
    -- the density is the eval render's (``field.inference_arith``) -- and puts every module's mode back afterwards.  ``normals``:
    analytic world-space normals at the vertices (needs the 32-input base MLP, like every analytic normal here); ``colors``: the
    field's colour seen against the normal.  ``chunk``: lattice points / vertices per field evaluation; it does not change the result."""
    res = ops._res3(resolution)
    field = model.field
    lo, hi = _bounds(field, bounds)
    modes = [(m, m.training) for m in model.modules()]
    model.eval()
    try:
        with torch.no_grad():
            sigma = density_lattice(field, res, lo, hi, chunk)
            vertices, triangles, _ = ops.surface_nets(sigma, res, lo, hi, level)
            del sigma
            nrm = vertex_normals(field, vertices, chunk) if (normals or colors) else None
            col = vertex_colors(model, vertices, nrm, chunk) if colors else None
    finally:
        for m, was in modes:
            m.training = was
    return Mesh(vertices, triangles, nrm if normals else None, col)


def _np(t, dtype) -> np.ndarray:
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=dtype)


def write_ply(path: str, mesh: Mesh) -> None:
    """Binary little-endian PLY: per vertex ``x y z`` (float), ``nx ny nz`` (float) when the mesh has normals, ``red green blue``
    (uchar, round(255 c)) when it has colours; per face a ``uchar`` count of 3 and three ``int`` vertex ids."""
    v = _np(mesh.vertices, "<f4").reshape(-1, 3)
    f = _np(mesh.triangles, "<i4").reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    props = ["property float x", "property float y", "property float z"]
    if mesh.normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        props += ["property float nx", "property float ny", "property float nz"]
    if mesh.colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        props += ["property uchar red", "property uchar green", "property uchar blue"]
    rec = np.zeros(v.shape[0], dtype=np.dtype(fields))
    for k, name in enumerate("xyz"):
        rec[name] = v[:, k]
    if mesh.normals is not None:
        n = _np(mesh.normals, "<f4").reshape(-1, 3)
        for k, name in enumerate(("nx", "ny", "nz")):
            rec[name] = n[:, k]
    if mesh.colors is not None:
        c = np.rint(np.clip(_np(mesh.colors, "<f4").reshape(-1, 3), 0.0, 1.0) * 255.0).astype(np.uint8)
        for k, name in enumerate(("red", "green", "blue")):
            rec[name] = c[:, k]
    faces = np.zeros(f.shape[0], dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    faces["n"] = 3
    faces["v"] = f
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}", *props, f"element face {f.shape[0]}",
              "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(rec.tobytes())
        fh.write(faces.tobytes())
