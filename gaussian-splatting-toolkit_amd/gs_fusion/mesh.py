"""Mesh cleaning on the GPU: what `ExportTSDF(clean=True)` does to `mesh.ply` with four MeshLab filters
(gs_toolkit/scripts/exporter.py:310-321) -- null faces, duplicate faces, connected components of fewer than
`min_component_faces` faces and unreferenced vertices are removed.  The rules are stated in include/gsraster.h
(DESIGN.md section 4.6); HIP kernels behind `gsr_mesh_*` (csrc/mesh_clean.hip); torch for memory and streams only; no
CPU fallback.
"""
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from rasterizer.cuda import _call, _check, _on, _stream, _typed

_f32, _i32 = torch.float32, torch.int32
GSR_ERANGE = -4
# rows of the `state` tensor (csrc/mesh_clean.hip)
ST_BAD, ST_NULL, ST_DUP, ST_COMPONENTS, ST_COMPONENTS_KEPT, ST_FACES_KEPT, ST_VERTICES_KEPT, ST_UNCONVERGED = range(8)


def _opt(t: Optional[Tensor]) -> Optional[Tensor]:
    """(an absent or empty tensor goes to the library as NULL)"""
    return None if t is None or t.numel() == 0 else t


def _check_mesh(triangles, num_vertices, vertices, vertex_colors) -> int:
    _check(triangles, "triangles", _i32)
    if triangles.dim() != 2 or triangles.size(1) != 3:
        raise RuntimeError("triangles must be [F,3]")
    V = int(num_vertices)
    if V < 0:
        raise ValueError("num_vertices must not be negative")
    for t, name in ((vertices, "vertices"), (vertex_colors, "vertex_colors")):
        if t is None:
            continue
        _check(t, name, _f32)
        if t.dim() != 2 or t.size(0) != V or (name == "vertices" and t.size(1) != 3):
            raise RuntimeError(f"{name} must be [V,{'3' if name == 'vertices' else 'C'}] with V = {V}")
        if t.device != triangles.device:
            raise RuntimeError(f"{name} and triangles must be on one device")
    return V


def _label(triangles: Tensor, V: int, vertices: Optional[Tensor], min_faces: int, labels: Optional[Tensor],
           sizes: Optional[Tensor], workspace: Optional[Tensor] = None):
    """The label call and its one read-back -> (state as a list of 8 ints, workspace).  `workspace`: a uint8 tensor
    of at least the queried size to use instead of a fresh one (the tests hand in a pre-filled one)."""
    dev, F = triangles.device, triangles.size(0)
    n = _typed().gsr_mesh_clean_workspace_bytes(V, F) if F else 0
    if F and n == 0:
        raise ValueError(f"mesh of {V} vertices and {F} faces: too large, or the workspace size query failed (no device?)")
    if workspace is None:
        workspace = torch.empty(n, dtype=torch.uint8, device=dev)
    elif workspace.numel() < n or workspace.device != dev or workspace.dtype != torch.uint8:
        raise RuntimeError(f"workspace must hold {n} bytes on {dev}")
    state = torch.empty(8, dtype=_i32, device=dev)
    L = _typed()
    rc = L.gsr_mesh_label(V, F, _opt(vertices), _opt(triangles), min_faces, state, _opt(workspace), workspace.numel(),
                          _opt(labels), _opt(sizes), _stream(dev))
    if rc == GSR_ERANGE:
        raise ValueError(L.gsr_last_error().decode())
    if rc != 0:
        raise RuntimeError(f"gsr_mesh_label failed ({rc}): {L.gsr_last_error().decode()}")
    st = state.cpu().tolist()  # the one read-back between label and emit
    if st[ST_UNCONVERGED]:
        raise RuntimeError("gsr_mesh_label: faces on one edge ended with different labels (internal error)")
    return st, workspace


def mesh_components(triangles: Tensor, num_vertices: int, vertices: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """-> labels int32 [F]: the lowest face index of the face's edge-connected component, -1 for a null or duplicate
    face; sizes int32 [F]: the number of faces of that component, 0 for a null or duplicate face.  Without `vertices`
    only faces that repeat an index are null.  An index outside [0, num_vertices) raises ValueError."""
    V = _check_mesh(triangles, num_vertices, vertices, None)
    dev, F = triangles.device, triangles.size(0)
    with _on(dev):
        labels, sizes = (torch.empty(F, dtype=_i32, device=dev) for _ in range(2))
        _label(triangles, V, vertices, 0, labels, sizes)
    return labels, sizes


def clean_mesh(vertices: Tensor, triangles: Tensor, vertex_colors: Optional[Tensor] = None,
               min_component_faces: int = 20000, return_info: bool = False):
    """-> (vertices [V',3], vertex_colors [V',C] or None, triangles [F',3] int32[, info]): null faces, duplicate faces
    (the lowest face index of each set of three indices stays) and components of fewer than `min_component_faces`
    faces removed, then the vertices nothing references; what stays keeps its order, rows are copied bit for bit.
    `info`: null_faces, duplicate_faces, components, components_kept, faces_removed_small, vertices_removed."""
    return _clean_mesh(vertices, triangles, vertex_colors, min_component_faces, return_info, None)


def _clean_mesh(vertices, triangles, vertex_colors, min_component_faces, return_info, workspace):
    """`clean_mesh` on a workspace handed in (None: a fresh one)."""
    if not isinstance(vertices, Tensor):
        raise RuntimeError("vertices must be a tensor")
    if vertices.dim() != 2 or vertices.size(1) != 3:
        raise RuntimeError("vertices must be [V,3]")
    V = _check_mesh(triangles, vertices.size(0), vertices, vertex_colors)
    min_faces = int(min_component_faces)
    if min_faces < 0:
        raise ValueError("min_component_faces must not be negative")
    dev, F = triangles.device, triangles.size(0)
    ncol = 0 if vertex_colors is None else vertex_colors.size(1)
    with _on(dev):
        st, ws = _label(triangles, V, vertices, min_faces, None, None, workspace)
        nv, nf = st[ST_VERTICES_KEPT], st[ST_FACES_KEPT]
        out_v = torch.empty((nv, 3), dtype=_f32, device=dev)
        out_c = None if vertex_colors is None else torch.empty((nv, ncol), dtype=_f32, device=dev)
        out_t = torch.empty((nf, 3), dtype=_i32, device=dev)
        if nf:
            _call("gsr_mesh_emit", V, F, ncol, _opt(vertices), _opt(vertex_colors), _opt(triangles), _opt(ws),
                  ws.numel(), nv, nf, _opt(out_v), _opt(out_c), _opt(out_t), _stream(dev))
    if not return_info:
        return out_v, out_c, out_t
    info: Dict[str, int] = {
        "null_faces": st[ST_NULL], "duplicate_faces": st[ST_DUP], "components": st[ST_COMPONENTS],
        "components_kept": st[ST_COMPONENTS_KEPT], "faces_removed_small": F - st[ST_NULL] - st[ST_DUP] - nf,
        "vertices_removed": V - nv}
    return out_v, out_c, out_t, info
