"""Time the GPU neighbour search behind the model's initial scales next to scikit-learn's on the same host.

    python tools/knn_bench.py [--sizes 200000 1000000 5000000] [--k 3] [--repeats 5] [--no-sklearn] [--sklearn-max N]

For every size and two clouds (a uniform cube; a "surface": three nested noisy spheres, like an SfM or TSDF cloud):
build (gs_fused.KNN: tree and workspace allocated outside the timing) and self-mode tree query, each the median of
`--repeats` runs timed with device events after a warm-up, and the wall-clock time of the reference's method for the
same call (NearestNeighbors(n_neighbors=k+1).fit(x).kneighbors(x), once).  One JSON line per row.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-splatting-toolkit_amd")]
import numpy as np


def cloud(kind, n, seed=0):
    g = np.random.default_rng(seed)
    if kind == "cube":
        return g.uniform(-1, 1, (n, 3)).astype(np.float32)
    u = g.standard_normal((n, 3))
    radius = np.array([0.7, 1.1, 1.5])[g.integers(0, 3, n)][:, None]
    return (u / np.linalg.norm(u, axis=1, keepdims=True) * (radius + 0.004 * g.standard_normal((n, 1)))).astype(np.float32)


def gpu_times(points, k, repeats, device):
    import torch

    from gs_fused import KNN
    from gs_fused.knn import BYTES_BUILD, BYTES_QUERY, BYTES_TREE, _bytes

    n = len(points)
    p = torch.from_numpy(points).to(device)
    tree = torch.empty(_bytes(BYTES_TREE, n, 0), dtype=torch.uint8, device=device)
    build_ws = torch.empty(_bytes(BYTES_BUILD, n, 0), dtype=torch.uint8, device=device)
    query_ws = torch.empty(_bytes(BYTES_QUERY, 0, n, k), dtype=torch.uint8, device=device)
    out = (torch.empty((n, k), dtype=torch.float32, device=device), torch.empty((n, k), dtype=torch.int32, device=device))

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms))

    build_ms = timed(lambda: KNN(p, _tree=tree, _workspace=build_ws))  # (one read-back of two words inside)
    knn = KNN(p, _tree=tree, _workspace=build_ws)
    query_ms = timed(lambda: knn.query(None, k, _workspace=query_ws, _out=out))
    return build_ms, query_ms, float(out[0].mean().item())


def sklearn_time(points, k):
    from sklearn.neighbors import NearestNeighbors

    t0 = time.perf_counter()
    d, _ = NearestNeighbors(n_neighbors=k + 1, algorithm="auto", metric="euclidean").fit(points).kneighbors(points)
    return 1e3 * (time.perf_counter() - t0), float(d[:, 1:].astype(np.float32).mean())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[200_000, 1_000_000, 5_000_000])
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--sklearn-max", type=int, default=5_000_000, help="largest size scikit-learn is timed at")
    a = ap.parse_args(argv)
    for n in a.sizes:
        for kind in ("cube", "surface"):
            pts = cloud(kind, n)
            build_ms, query_ms, mean = gpu_times(pts, a.k, a.repeats, a.device)
            row = {"cloud": kind, "n": n, "k": a.k, "gpu_build_ms": round(build_ms, 3), "gpu_query_ms": round(query_ms, 3),
                   "gpu_mean_distance": mean, "sklearn_ms": None}
            if not a.no_sklearn and n <= a.sklearn_max:
                row["sklearn_ms"], row["sklearn_mean_distance"] = sklearn_time(pts, a.k)
                row["sklearn_ms"] = round(row["sklearn_ms"], 1)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
