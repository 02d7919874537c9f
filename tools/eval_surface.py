"""Surface distance of a generated mesh against ground truth: gs_toolkit/evaluation/surface_distance on the GPU.

    python tools/eval_surface.py --gt GT.{stl,ply} --mesh MESH.ply [--both] [--threshold T] [--device cuda:0]

Prints one JSON line.  `average_error` is the toolkit tool's `Average Error`: the mean unsigned distance from every
vertex of MESH.ply to the ground-truth triangle mesh; `rms`, `max`, `invalid` (non-finite vertices, left out) and
`within_threshold` (vertices no farther than T; null without --threshold) describe the same distances.  With --both the
same fields with the prefix `completeness_` are added for the other direction: every ground-truth vertex against the
generated mesh.  An STL file is a soup: each facet's three vertices, nothing welded (distances do not depend on it).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-splatting-toolkit_amd")]
import numpy as np

FIELDS = (("average_error", "mean"), ("rms", "rms"), ("max", "max"), ("invalid", "invalid"),
          ("within_threshold", "within_threshold"))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gt", required=True, help="ground truth: .stl (binary or ASCII) or .ply")
    ap.add_argument("--mesh", required=True, help="generated mesh: .ply")
    ap.add_argument("--both", action="store_true", help="also ground-truth vertices against the generated mesh")
    ap.add_argument("--threshold", type=float, default=None)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if a.threshold is not None and not a.threshold >= 0:
        ap.error("--threshold must not be negative")
    if os.path.splitext(a.gt)[1].lower() not in (".stl", ".ply"):
        ap.error("--gt must be an .stl or a .ply file")
    return a


def load_mesh(path):
    """-> (vertices float32 [V,3], triangles int32 [F,3]) of an STL (a soup) or a PLY file."""
    from gs_io import read_mesh_ply, read_stl

    if os.path.splitext(path)[1].lower() == ".stl":
        tri = read_stl(path)
        return np.ascontiguousarray(tri.reshape(-1, 3)), np.arange(3 * len(tri), dtype=np.int32).reshape(-1, 3)
    m = read_mesh_ply(path)
    return np.ascontiguousarray(m["vertices"], np.float32), np.ascontiguousarray(m["triangles"], np.int32)


def evaluate(gt, mesh, device, both=False, threshold=None, prefix=""):
    """gt, mesh: (vertices, triangles) NumPy pairs -> the rows of the JSON line."""
    import torch

    from gs_fusion import MeshDistance

    dev = torch.device(device)
    gv, gtri = (torch.from_numpy(x).to(dev) for x in gt)
    mv, mtri = (torch.from_numpy(x).to(dev) for x in mesh)
    truth = MeshDistance(gv, gtri)
    s = truth.stats(truth.query(mv)[0], threshold)
    row = {prefix + k: s[src] for k, src in FIELDS}
    row[prefix + "gt_triangles_skipped"] = truth.skipped_triangles
    if both:
        if mtri.shape[0] == 0:
            raise SystemExit("eval_surface: --both needs faces in the generated mesh")
        ours = MeshDistance(mv, mtri)
        s = ours.stats(ours.query(gv)[0], threshold)
        row.update({prefix + "completeness_" + k: s[src] for k, src in FIELDS})
    return row


def main(argv=None):
    a = parse_args(argv)
    row = evaluate(load_mesh(a.gt), load_mesh(a.mesh), a.device, a.both, a.threshold)
    print(json.dumps(row))


if __name__ == "__main__":
    main()
