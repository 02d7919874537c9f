"""Start a model from a point cloud, as `populate_modules` does (vanilla_gs.py:126-174), with the neighbour search on the GPU.

    python tools/seed_from_points.py --points CLOUD.ply --out SEED.ply [--sh-degree 3] [--seed 0] [--device cuda:0]

Reads a point-cloud PLY (positions and, if present, 8-bit colours -- what tools/export_tsdf.py writes as
point_cloud.ply), and writes a Gaussian PLY in the toolkit's layout: means = the points; log-scales = log of the mean
distance to the three nearest other points on all three axes (gs_fused.initial_log_scales; duplicate points give -inf,
as in the reference); random unit quaternions; opacity logit(0.1); features_dc = RGB2SH(colour / 255) (uniform random
without colours, as the reference does without seed colours); higher bands zero.  Points with a non-finite coordinate
are dropped and counted.  Prints one JSON line.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-splatting-toolkit_amd")]
import numpy as np

SH_C0 = 0.28209479177387814


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", required=True, help="point cloud: .ply")
    ap.add_argument("--out", required=True, help="Gaussian .ply to write")
    ap.add_argument("--sh-degree", type=int, default=3, choices=[0, 1, 2, 3, 4])
    ap.add_argument("--seed", type=int, default=0, help="seed of the random quaternions (and colours, if the cloud has none)")
    ap.add_argument("--device", default="cuda:0")
    return ap.parse_args(argv)


def seed_gaussians(points, colors, sh_degree, seed, device):
    """points float32 [n,3], colors uint8 [n,3] or None -> (the model's raw parameters as NumPy, rows dropped)."""
    import torch

    from gs_fused import initial_log_scales
    from harness.scene import num_sh_bases
    from harness.train import random_quats

    keep = np.isfinite(points).all(1)
    points = np.ascontiguousarray(points[keep], np.float32)
    n = len(points)
    if n < 4:
        raise SystemExit(f"seed_from_points: {n} usable points; the three nearest neighbours need at least 4")
    rng = np.random.default_rng(seed)
    scales = initial_log_scales(torch.from_numpy(points).to(device), 3).cpu().numpy()
    quats = random_quats(n, rng)
    if colors is not None:
        dc = (np.asarray(colors)[keep].astype(np.float32) / np.float32(255) - np.float32(0.5)) / np.float32(SH_C0)
    else:
        dc = rng.uniform(size=(n, 3))
    return {
        "means": points, "scales": scales, "quats": quats,
        "opacities": np.full((n, 1), math.log(0.1 / 0.9), np.float32), "features_dc": dc.astype(np.float32),
        "features_rest": np.zeros((n, num_sh_bases(sh_degree) - 1, 3), np.float32),
    }, int((~keep).sum())


def main(argv=None):
    from gs_io import read_point_cloud_ply, write_gaussian_ply

    a = parse_args(argv)
    cloud = read_point_cloud_ply(a.points)
    params, dropped = seed_gaussians(cloud["points"], cloud["colors"], a.sh_degree, a.seed, a.device)
    write_gaussian_ply(a.out, params)
    s = params["scales"][:, 0]
    fin = np.isfinite(s)
    print(json.dumps({"gaussians": len(s), "dropped_points": dropped, "coloured": cloud["colors"] is not None,
                      "duplicate_points": int((~fin).sum()), "median_scale": float(np.exp(np.median(s[fin]))) if fin.any() else None,
                      "out": a.out}))


if __name__ == "__main__":
    main()
