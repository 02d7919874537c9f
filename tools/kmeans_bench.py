#!/usr/bin/env python3
"""The records behind DESIGN.md section 4.24 (k-means for the compressed export): `gs_fused.kmeans_assign`,
`kmeans_update` and one whole iteration of `gs_fused.kmeans` (assign, inertia, sort, update) against the torch path.

    python tools/kmeans_bench.py [--points 1000000] [--clusters 4096 16384 65536] [--dims 45 9 24] [--rounds 5]
        [--torch-rounds 2] [--out profiles/kmeans_bench.json]

Per (D, K): N rows of standard-normal float32, the centres K of them (seeded).  Every time is the median over
`--rounds` calls of device events around the call after three warm-up calls (the host launch path included).  The torch
path is what a caller without the kernel writes: `torch.cdist` + `argmin` over chunks of points whose [chunk, K]
distance matrix fits 2 GiB, and `index_add_` + `bincount` for the update (float32 sums with atomics: neither the
kernel's rounding rule nor reproducible, which is why it is a comparison of time only).

lane_ops_per_s: the 3 N K D float32 operations of the rule (a subtraction, a product, an addition per term; the padding
to a multiple of four columns is not counted) over the assign time.  share_of_fp32_vector_peak divides it by
157.3e12, the vector peak of the MI355X -- which counts a fused multiply-add as two operations; the rule forbids
contraction, so a kernel issuing one unfused, unpacked operation per lane and clock tops out at half of it.
D other than 45 is timed at the first K only.  Merges one record per (D, K) into the JSON file; prints them.

    python tools/kmeans_bench.py --config3 [--iters 7000] [--clusters 4096 16384 65536] [--kmeans-iters 10]

trains the bench's config 3 once and compresses the trained model without a codebook and at every K (gs_io.compressed):
bytes on disk against the PLY, PSNR on the evaluation views raw and decompressed, PSNR between the two models' renders
of the training views, the seconds the clustering took.  One run; the record goes under "config3".
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-splatting-toolkit_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402

FP32_VECTOR_PEAK = 157.3e12


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--clusters", type=int, nargs="+", default=[4096, 16384, 65536])
    ap.add_argument("--dims", type=int, nargs="+", default=[45, 9, 24])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch-rounds", type=int, default=2, help="0: skip the torch path")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_bench.json"))
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--config3", action="store_true", help="the trained model's record instead of the kernel times")
    ap.add_argument("--iters", type=int, default=7000, help="--config3: training iterations")
    ap.add_argument("--kmeans-iters", type=int, default=10, help="--config3: Lloyd iterations per codebook")
    return ap.parse_args(argv)


def _time(fn, rounds, warmup=3):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(float(np.median(ms)), 4)


def torch_assign(x, c):
    import torch

    chunk = max(1, (1 << 29) // c.shape[0])
    labels = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    for s in range(0, x.shape[0], chunk):
        labels[s:s + chunk] = torch.cdist(x[s:s + chunk], c).argmin(dim=1)
    return labels


def torch_update(x, labels, c):
    import torch

    sums = torch.zeros_like(c).index_add_(0, labels, x)
    counts = torch.bincount(labels, minlength=c.shape[0]).clamp_(min=1)
    return sums / counts[:, None]


def record(n, d, k, rounds, torch_rounds, device):
    import torch

    from gs_fused import kmeans, kmeans_assign, kmeans_update

    gen = torch.Generator(device="cpu").manual_seed(d * 100003 + k)
    x = torch.randn((n, d), generator=gen).to(device)
    c = x[torch.randperm(n, generator=gen)[:k].to(device)].contiguous()
    labels, _ = kmeans_assign(x, c)
    rec = {"points": n, "dim": d, "clusters": k, "rounds": rounds,
           "assign_ms": _time(lambda: kmeans_assign(x, c), rounds),
           "update_ms": _time(lambda: kmeans_update(x, labels, c), rounds),
           "iteration_ms": _time(lambda: kmeans(x, k, iters=1, init=c), rounds, warmup=1)}
    # (kmeans(iters=1) is one iteration plus the final assignment and its inertia)
    rec["iteration_ms"] = round(rec["iteration_ms"] - rec["assign_ms"], 4)
    ops = 3.0 * n * k * d
    rec["lane_ops_per_s"] = ops / (rec["assign_ms"] * 1e-3)
    rec["share_of_fp32_vector_peak"] = round(rec["lane_ops_per_s"] / FP32_VECTOR_PEAK, 4)
    if torch_rounds > 0:
        tl = torch_assign(x, c)
        rec["torch_labels_equal"] = round(float((tl == labels).double().mean()), 6)
        rec["torch_assign_ms"] = _time(lambda: torch_assign(x, c), torch_rounds, warmup=1)
        rec["torch_update_ms"] = _time(lambda: torch_update(x, tl, c), torch_rounds, warmup=1)
        rec["assign_speedup"] = round(rec["torch_assign_ms"] / rec["assign_ms"], 3)
        rec["update_speedup"] = round(rec["torch_update_ms"] / rec["update_ms"], 3)
    return rec


def config3(a, device):
    """The bench's config 3 trained once (as tools/contribution_bench.py trains it), then per K the model compressed,
    written, read and decompressed: bytes on disk against the PLY, PSNR on the evaluation views of the raw and of the
    decompressed model, and the mean PSNR between their renders of the training views."""
    import dataclasses
    import tempfile

    import torch

    import bench
    import harness.train as HT
    from gs_io import (compress_gaussians, decompress_gaussians, read_compressed, read_gaussian_ply,
                       write_compressed)
    from gs_io.compressed import bytes_per_gaussian

    tmp = tempfile.mkdtemp()
    ply = os.path.join(tmp, "config3.ply")
    cfg = dataclasses.replace(bench.config3(iters=a.iters), export_ply=ply)
    res = HT.train(cfg, device)
    data = HT.make_data(cfg, device)  # (the same seed: the views and their ground truth again)
    raw = read_gaussian_ply(ply)
    model = HT.GaussianParams(raw, device)
    cams = data.cams_by_d[1]
    rec = {"iters": a.iters, "seed": cfg.seed, "num_gaussians": model.num_points, "ply_bytes": os.path.getsize(ply),
           "psnr_raw": round(HT.evaluate(model, data, cfg)["psnr"], 3), "iters_per_s": round(res["iters_per_s"], 1),
           "rows": []}
    on_device = {k: torch.from_numpy(v).to(device) for k, v in raw.items()}
    with torch.no_grad():
        views = [model.render(c, data.bg, cfg.sh_degree, rasterize_mode=cfg.rasterize_mode)["rgb"] for c in cams]
        for k in [0] + list(a.clusters):
            blob = compress_gaussians(on_device, sh_clusters=k, iters=a.kmeans_iters, seed=0)
            out = os.path.join(tmp, f"config3_k{k}.npz")
            write_compressed(out, blob)
            back = decompress_gaussians(read_compressed(out))
            small = HT.GaussianParams({n: v.numpy() for n, v in back.items()}, device)
            between = [HT.psnr(small.render(c, data.bg, cfg.sh_degree, rasterize_mode=cfg.rasterize_mode)["rgb"], v)
                       for c, v in zip(cams, views)]
            report = blob["kmeans"]
            rec["rows"].append({
                "sh_clusters": blob["meta"]["sh_clusters"], "kmeans_iters": a.kmeans_iters,
                "bytes_on_disk": os.path.getsize(out), "bytes_per_gaussian": bytes_per_gaussian(blob["meta"]),
                "ratio_to_ply": round(os.path.getsize(ply) / os.path.getsize(out), 2),
                "psnr": round(HT.evaluate(small, data, cfg)["psnr"], 3),
                "psnr_between_renders": round(float(np.mean(between)), 3),
                "kmeans_seconds": None if report is None else round(report["seconds"], 3),
                "inertia_first_last": None if report is None else [report["inertia"][0], report["inertia"][-1]]})
            print(json.dumps(rec["rows"][-1]), flush=True)
    return rec


def main(argv=None):
    a = parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("kmeans_bench: needs a GPU (a time taken anywhere else says nothing)")
    device = torch.device(a.device)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    data = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.config3:
        data["config3"] = config3(a, device)
        print(json.dumps(data["config3"]), flush=True)
        with open(a.out, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
        return data
    sizes = [(a.dims[0], k) for k in a.clusters] + [(d, a.clusters[0]) for d in a.dims[1:]]
    for d, k in sizes:
        rec = record(a.points, d, k, a.rounds, a.torch_rounds, device)
        data[f"n{a.points}_d{d}_k{k}"] = rec
        print(json.dumps(rec), flush=True)
        with open(a.out, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
    return data


if __name__ == "__main__":
    main()
