"""Unsigned distance from points to a triangle mesh on the GPU: what the toolkit's evaluation tool
(gs_toolkit/evaluation/surface_distance: every vertex of a generated PLY against a ground-truth STL, the mean printed
as `Average Error`) computes, one BVH query per point.  The rule is stated in include/gsraster.h (DESIGN.md section
4.7); HIP kernels behind `gsr_mesh_bvh_build` / `gsr_mesh_distance_*` (csrc/mesh_distance.hip); torch for memory and
streams only; no CPU path.
"""
from typing import Dict, Optional

import torch
from torch import Tensor

from rasterizer.cuda import _call, _check, _on, _stream, _typed

_f32, _i32 = torch.float32, torch.int32
GSR_ERANGE = -4
EXHAUSTIVE = 1
BYTES_TREE, BYTES_BUILD, BYTES_QUERY, BYTES_STATS = range(4)
STAT_NAMES = ("count", "invalid", "mean", "rms", "max", "within_threshold", "sum", "sum_squares")


def _bytes(what: int, num_faces: int, num_points: int) -> int:
    n = _typed().gsr_mesh_distance_workspace_bytes(what, num_faces, num_points)
    if n == 0:
        raise ValueError(f"{num_faces} faces / {num_points} points: too large, or a size query failed (no device?)")
    return n


def _space(workspace: Optional[Tensor], nbytes: int, dev) -> Tensor:
    """A fresh workspace, or the one handed in (the tests hand in pre-filled ones)."""
    if workspace is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if workspace.numel() < nbytes or workspace.device != dev or workspace.dtype != torch.uint8:
        raise RuntimeError(f"workspace must hold {nbytes} bytes on {dev}")
    return workspace


class MeshDistance:
    """A triangle mesh (float32 [V,3] vertices, int32 [F,3] triangles; a soup is fine) built into a BVH once and
    queried many times.  An index outside [0, V), an empty mesh or one without a usable triangle raises ValueError;
    triangles with a non-finite vertex are left out and counted in `skipped_triangles`."""

    def __init__(self, vertices: Tensor, triangles: Tensor, _tree: Optional[Tensor] = None,
                 _workspace: Optional[Tensor] = None):
        _check(vertices, "vertices", _f32)
        _check(triangles, "triangles", _i32)
        if vertices.dim() != 2 or vertices.size(1) != 3:
            raise RuntimeError("vertices must be [V,3]")
        if triangles.dim() != 2 or triangles.size(1) != 3:
            raise RuntimeError("triangles must be [F,3]")
        if vertices.device != triangles.device:
            raise RuntimeError("vertices and triangles must be on one device")
        V, F = vertices.size(0), triangles.size(0)
        if F == 0:
            raise ValueError("the mesh has no triangles")
        self.device, self.num_faces = triangles.device, F
        dev = self.device
        with _on(dev):
            self._tree = _space(_tree, _bytes(BYTES_TREE, F, 0), dev)
            ws = _space(_workspace, _bytes(BYTES_BUILD, F, 0), dev)
            state = torch.empty(4, dtype=_i32, device=dev)
            L = _typed()
            rc = L.gsr_mesh_bvh_build(V, F, None if vertices.numel() == 0 else vertices, triangles, self._tree,
                                      self._tree.numel(), ws, ws.numel(), state, _stream(dev))
            if rc == GSR_ERANGE:
                raise ValueError(L.gsr_last_error().decode())
            if rc != 0:
                raise RuntimeError(f"gsr_mesh_bvh_build failed ({rc}): {L.gsr_last_error().decode()}")
            self.skipped_triangles = int(state[1].item())
        if self.skipped_triangles == F:
            raise ValueError(f"the mesh has no usable triangle: all {F} have a non-finite vertex")

    def query(self, points: Tensor, return_closest: bool = False, exhaustive: bool = False,
              _workspace: Optional[Tensor] = None, _out=None):
        """-> (distance float32 [n], face int32 [n][, closest float32 [n,3]]).  A non-finite point gets NaN / -1.
        `exhaustive`: every point against every triangle instead of the tree walk -- the on-device cross-check (and
        fine for tiny meshes); the same per-triangle function, never chosen automatically."""
        _check(points, "points", _f32)
        if points.dim() != 2 or points.size(1) != 3:
            raise RuntimeError("points must be [n,3]")
        if points.device != self.device:
            raise RuntimeError("points and the mesh must be on one device")
        n, dev = points.size(0), self.device
        with _on(dev):
            if _out is not None:
                dist, face, closest = _out
            else:
                dist = torch.empty(n, dtype=_f32, device=dev)
                face = torch.empty(n, dtype=_i32, device=dev)
                closest = torch.empty((n, 3), dtype=_f32, device=dev) if return_closest else None
            if n:
                ws = None if exhaustive else _space(_workspace, _bytes(BYTES_QUERY, 0, n), dev)
                _call("gsr_mesh_distance_query", self.num_faces, self._tree, self._tree.numel(), n, points,
                      EXHAUSTIVE if exhaustive else 0, ws, 0 if ws is None else ws.numel(), dist, face, closest,
                      _stream(dev))
        return (dist, face, closest) if return_closest else (dist, face)

    def stats(self, distance: Tensor, threshold: Optional[float] = None,
              _workspace: Optional[Tensor] = None) -> Dict[str, float]:
        return distance_stats(distance, threshold, _workspace)


def distance_stats(distance: Tensor, threshold: Optional[float] = None,
                   _workspace: Optional[Tensor] = None) -> Dict[str, float]:
    """Statistics of float32 distances, summed in float64 in a fixed order on the device (bit-reproducible):
    count (finite), invalid (non-finite, left out), mean, rms, max, within_threshold (distances <= threshold; None
    without one), sum, sum_squares."""
    _check(distance, "distance", _f32)
    if distance.dim() != 1:
        raise RuntimeError("distance must be [n]")
    if threshold is not None and not float(threshold) >= 0:
        raise ValueError("threshold must not be negative")
    n, dev = distance.size(0), distance.device
    with _on(dev):
        ws = _space(_workspace, _bytes(BYTES_STATS, 0, n), dev) if n else None
        out = torch.empty(8, dtype=torch.float64, device=dev)
        _call("gsr_mesh_distance_stats", n, None if distance.numel() == 0 else distance,
              -1.0 if threshold is None else threshold, ws,
              0 if ws is None else ws.numel(), out, _stream(dev))
        row = out.cpu().tolist()
    res = dict(zip(STAT_NAMES, row))
    for k in ("count", "invalid", "within_threshold"):
        res[k] = int(res[k])
    if threshold is None:
        res["within_threshold"] = None
    return res


def surface_distance(points: Tensor, vertices: Tensor, triangles: Tensor,
                     threshold: Optional[float] = None) -> Dict[str, float]:
    """The one-call form: statistics of the distances from `points` to the mesh (`mean` is the evaluation tool's
    `Average Error` when `points` are the generated mesh's vertices and the mesh is the ground truth)."""
    mesh = MeshDistance(vertices, triangles)
    return mesh.stats(mesh.query(points)[0], threshold)
