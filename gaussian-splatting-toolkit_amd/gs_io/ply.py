"""Gaussian-splat PLY files, as `gs-export gaussian-splat` writes them.

Layout restated from `ExportGaussianSplat.main` / `construct_list_of_attributes`
(gs_toolkit/scripts/exporter.py:88-147): one `vertex` element, every property
`float` (f4), binary little-endian (what plyfile's `PlyData([el]).write` emits by
default), in this order:

    x y z  nx ny nz  f_dc_0..2  f_rest_0..(3*(K-1)-1)  opacity  scale_0..2  rot_0..3

with RAW (pre-activation) values: log-scales, logit opacities, un-normalised
(w,x,y,z) quaternions, normals all zero, and `f_rest` stored CHANNEL-major
(`features_rest.transpose(1, 2).flatten(1)`: f_rest_{c*(K-1)+k} = features_rest[n,k,c]).
No dependency on plyfile (not installed here); numpy only.
"""
from typing import Dict

import numpy as np


def _attribute_names(n_rest: int):
    names = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]
    names += [f"f_rest_{i}" for i in range(n_rest)]
    names += ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    return names


def write_gaussian_ply(path: str, params: Dict[str, np.ndarray]) -> None:
    """`params`: means [N,3], features_dc [N,3], features_rest [N,K-1,3], opacities [N,1],
    scales [N,3], quats [N,4] (raw values, as held by the model's `gauss_params`)."""
    xyz = np.asarray(params["means"], np.float32)
    n = xyz.shape[0]
    f_dc = np.asarray(params["features_dc"], np.float32).reshape(n, 3)
    rest = np.asarray(params["features_rest"], np.float32)
    # channel-major; the width is spelled out so that an empty model (N = 0) keeps its SH degree
    f_rest = np.ascontiguousarray(rest.transpose(0, 2, 1)).reshape(n, rest.shape[1] * rest.shape[2])
    cols = [xyz, np.zeros_like(xyz), f_dc, f_rest, np.asarray(params["opacities"], np.float32).reshape(n, 1),
            np.asarray(params["scales"], np.float32).reshape(n, 3),
            np.asarray(params["quats"], np.float32).reshape(n, 4)]
    table = np.ascontiguousarray(np.concatenate(cols, axis=1).astype("<f4"))
    names = _attribute_names(f_rest.shape[1])
    assert table.shape[1] == len(names)
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n
    header += "".join(f"property float {a}\n" for a in names) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(table.tobytes())


def read_gaussian_ply(path: str) -> Dict[str, np.ndarray]:
    """Inverse of `write_gaussian_ply`; also accepts files written by the toolkit
    itself or by the original 3DGS code (same property names)."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("not a PLY file")
        fmt, n, props, in_vertex = None, None, [], False
        while True:
            line = f.readline()
            if not line:
                raise ValueError("unexpected end of PLY header")
            tok = line.decode("ascii").split()
            if not tok or tok[0] == "comment":
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                in_vertex = tok[1] == "vertex"
                if in_vertex:
                    n = int(tok[2])
            elif tok[0] == "property" and in_vertex:
                if tok[1] not in ("float", "float32"):
                    raise ValueError(f"unsupported property type {tok[1]}")
                props.append(tok[2])
            elif tok[0] == "end_header":
                break
        if fmt != "binary_little_endian" or n is None:
            raise ValueError("only binary_little_endian PLY files with a vertex element are supported")
        data = np.frombuffer(f.read(n * len(props) * 4), dtype="<f4").reshape(n, len(props))
    col = {p: i for i, p in enumerate(props)}
    take = lambda names: np.ascontiguousarray(data[:, [col[a] for a in names]], dtype=np.float32)
    n_rest = sum(1 for p in props if p.startswith("f_rest_"))
    if n_rest % 3:
        raise ValueError("f_rest count must be a multiple of 3")
    rest = take([f"f_rest_{i}" for i in range(n_rest)]).reshape(n, 3, n_rest // 3).transpose(0, 2, 1)
    return {
        "means": take(["x", "y", "z"]),
        "features_dc": take(["f_dc_0", "f_dc_1", "f_dc_2"]),
        "features_rest": np.ascontiguousarray(rest),
        "opacities": take(["opacity"]),
        "scales": take(["scale_0", "scale_1", "scale_2"]),
        "quats": take(["rot_0", "rot_1", "rot_2", "rot_3"]),
    }


# ---- geometry files of the TSDF exporter (gs_fusion, tools/export_tsdf.py) ------------------------------------------
# `point_cloud.ply` / `mesh.ply` as `ExportTSDF` saves them through Open3D: binary little-endian, positions (and
# normals) as `float`, colours as `uchar` red / green / blue, faces as `list uchar int vertex_indices`.

_PLY_TYPES = {"float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8", "uchar": "u1", "uint8": "u1",
              "char": "i1", "int8": "i1", "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2",
              "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4"}


def colors_to_uint8(colors) -> np.ndarray:
    """float colours -> uchar: clipped to [0, 1], times 255, rounded to nearest."""
    return np.rint(np.clip(np.asarray(colors, np.float32), 0.0, 1.0) * np.float32(255.0)).astype(np.uint8)


def _vertex_block(xyz, normals, colors):
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    if normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    rec = np.empty(len(xyz), dtype=fields)
    for k, a in enumerate("xyz"):
        rec[a] = xyz[:, k]
    if normals is not None:
        normals = np.asarray(normals, np.float32).reshape(-1, 3)
        if len(normals) != len(xyz):
            raise ValueError("one normal per vertex")
        for k, a in enumerate(("nx", "ny", "nz")):
            rec[a] = normals[:, k]
    if colors is not None:
        colors = np.asarray(colors)
        if colors.dtype != np.uint8:
            colors = colors_to_uint8(colors)
        colors = colors.reshape(-1, 3)
        if len(colors) != len(xyz):
            raise ValueError("one colour per vertex")
        for k, a in enumerate(("red", "green", "blue")):
            rec[a] = colors[:, k]
    header = "element vertex %d\n" % len(xyz)
    header += "".join("property %s %s\n" % ("uchar" if t == "u1" else "float", a) for a, t in fields)
    return header, rec


def write_point_cloud_ply(path: str, points, colors, normals=None) -> None:
    """points [M,3] float, colors [M,3] float in [0,1] (or uint8), normals [M,3] or None."""
    vh, rec = _vertex_block(points, normals, colors)
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\n" + vh + "end_header\n").encode("ascii"))
        f.write(rec.tobytes())


def write_mesh_ply(path: str, vertices, triangles, vertex_colors=None) -> None:
    """vertices [V,3] float, triangles [F,3] int, vertex_colors [V,3] float in [0,1] (or uint8) or None."""
    vh, rec = _vertex_block(vertices, None, vertex_colors)
    tri = np.asarray(triangles).reshape(-1, 3)
    if len(tri) and (tri.min() < 0 or tri.max() >= len(rec)):
        raise ValueError("triangle index out of range")
    faces = np.empty(len(tri), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    faces["n"] = 3
    faces["v"] = tri
    header = "ply\nformat binary_little_endian 1.0\n" + vh
    header += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(tri)
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())
        f.write(faces.tobytes())


def _read_geometry_ply(path: str):
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("not a PLY file")
        fmt, elements = None, []
        while True:
            line = f.readline()
            if not line:
                raise ValueError("unexpected end of PLY header")
            tok = line.decode("ascii").split()
            if not tok or tok[0] == "comment":
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append((tok[1], int(tok[2]), []))
            elif tok[0] == "property":
                if tok[1] == "list":
                    elements[-1][2].append((tok[4], ("list", _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]])))
                else:
                    elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        if fmt != "binary_little_endian":
            raise ValueError("only binary_little_endian PLY files are supported")
        out = {}
        for name, n, props in elements:
            fields = []
            for p, t in props:
                if isinstance(t, tuple):  # a list of constant length 3 (triangles)
                    fields += [(p + "_n", t[1]), (p, t[2], (3,))]
                else:
                    fields.append((p, t))
            dt = np.dtype(fields)
            out[name] = np.frombuffer(f.read(n * dt.itemsize), dtype=dt, count=n)
            for p, t in props:
                if isinstance(t, tuple) and n and not (out[name][p + "_n"] == 3).all():
                    raise ValueError("only triangle faces are supported")
    return out


def _vertex_arrays(v):
    names = v.dtype.names
    take = lambda cols, dt: np.stack([v[c] for c in cols], 1).astype(dt) if all(c in names for c in cols) else None  # noqa: E731
    return (take("xyz", np.float32), take(("nx", "ny", "nz"), np.float32), take(("red", "green", "blue"), np.uint8))


def read_point_cloud_ply(path: str) -> Dict[str, np.ndarray]:
    """-> points [M,3] f32, colors [M,3] uint8 or None, normals [M,3] f32 or None"""
    xyz, normals, colors = _vertex_arrays(_read_geometry_ply(path)["vertex"])
    return {"points": xyz, "colors": colors, "normals": normals}


def read_mesh_ply(path: str) -> Dict[str, np.ndarray]:
    """-> vertices [V,3] f32, triangles [F,3] int32, vertex_colors [V,3] uint8 or None"""
    el = _read_geometry_ply(path)
    xyz, _, colors = _vertex_arrays(el["vertex"])
    tri = np.ascontiguousarray(el["face"]["vertex_indices"], dtype=np.int32) if "face" in el else np.zeros((0, 3), np.int32)
    return {"vertices": xyz, "triangles": tri.reshape(-1, 3), "vertex_colors": colors}
