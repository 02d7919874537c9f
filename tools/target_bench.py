#!/usr/bin/env python3
"""Time the three ways a training step's target is formed, at 1920x1080 and 3840x2160, RGBA and RGB, d = 1, 2, 4:

  (a) `fused_target`, the trainer's path without a dataset: RGBA -- one `addcmul` of two cached float planes per
      (view, factor) with the step's background; RGB -- `downscale_image` of the cached float image;
  (b) the reference's per-step sequence on a cached float image: resize, then composite (get_gt_img,
      vanilla_gs.py:859-881); for RGB it is (a);
  (c) gs_fused.target_from_u8 on the uint8 image (csrc/target.hip).

    python tools/target_bench.py [--sizes 1920x1080 3840x2160] [--calls 20] [--repeats 9] [--output FILE.json]

Device events around `--calls` back-to-back calls after a warm-up of the same; the median of `--repeats` such
windows, the three paths alternating inside every repeat.  Bytes are what each path's kernels must move, computed
from the shapes (`path_bytes`); the share of peak is bytes / time over the HBM peak (8.0 TB/s specified; a float4 copy
reaches 6.29 TB/s).  Also: bytes per cached view under the three schemes, and images per second of the upload into a
gs_fused.ImageCache (pinned host memory, one copy per file).  Needs a GPU: there is nothing to time without one.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-splatting-toolkit_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12
HBM_COPY = 6.29e12


def path_bytes(path: str, H: int, W: int, C: int, d: int) -> int:
    """Bytes the kernels of a path read and write for one target, from the shapes alone (caches ignored)."""
    src, out = H * W, (H // d) * (W // d)
    taps = src if d == 1 else min(src, 4 * out)  # source pixels a resize touches
    if path == "c":
        return C * taps + 12 * out
    resize = 0 if d == 1 else 4 * C * taps + 4 * C * out  # float image in, float image out
    if C == 3:
        return resize
    if path == "a":
        return (12 + 4) * out + 12 * out  # addcmul: two planes in, the target out
    # (b) composite on the resized RGBA: a * rgb (16 in, 12 out), 1 - a (4, 4), * background (4, 12), + (24, 12)
    return resize + 88 * out


def cache_bytes_per_view(H: int, W: int, C: int, factors) -> dict:
    px = H * W
    planes = sum(16 * (H // d) * (W // d) for d in factors) if C == 4 else 0
    return {"reference_float32": 4 * C * px,
            "trainer_without_dataset": 12 * px + (16 * px if C == 4 else 0) + planes,
            "image_cache_uint8": C * px}


def timed_windows(fns: dict, calls: int, repeats: int) -> dict:
    for fn in fns.values():  # warm-up of every shape
        for _ in range(calls):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():  # alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b) / calls)
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ms.items()}


def bench_shape(H: int, W: int, C: int, d: int, dev, calls: int, repeats: int) -> dict:
    import harness.train as HT
    from gs_fused import target_from_u8

    rng = np.random.default_rng(H + C + d)
    u8 = torch.from_numpy(rng.integers(0, 256, (H, W, C), dtype=np.uint8)).to(dev)
    f32 = u8.float() / 255.0
    bg = torch.rand(3, device=dev)
    h, w = H // d, W // d
    out = torch.empty((h, w, 3), device=dev)
    if C == 4:
        small = HT.downscale_image(f32, d)
        a = small[..., 3:4]
        planes = ((a * small[..., :3]).contiguous(), (1 - a).contiguous())
        fns = {"a": lambda: torch.addcmul(planes[0], planes[1], bg),
               "b": lambda: HT.composite_with_background(HT.downscale_image(f32, d), bg)}
    else:
        fns = {"a": lambda: HT.downscale_image(f32, d)}
    fns["c"] = lambda: target_from_u8(u8, bg, (h, w), out=out)
    agree = float((fns["c"]() - (fns["b"]() if C == 4 else fns["a"]())).abs().max())
    row = {"height": H, "width": W, "channels": C, "d": d, "max_abs_difference_c_vs_torch": agree, "paths": {}}
    for k, (med, lo, hi) in timed_windows(fns, calls, repeats).items():
        nbytes = path_bytes(k, H, W, C, d)
        row["paths"][k] = {"ms_median": med, "ms_min": lo, "ms_max": hi, "bytes": nbytes,
                           "tb_per_s": nbytes / (med * 1e-3) / 1e12 if nbytes else None,
                           "share_of_hbm_peak": nbytes / (med * 1e-3) / HBM_PEAK if nbytes else None}
    return row


def bench_upload(H: int, W: int, C: int, n: int, dev) -> dict:
    from gs_fused import ImageCache

    rng = np.random.default_rng(7)
    imgs = [rng.integers(0, 256, (H, W, C), dtype=np.uint8) for _ in range(n)]
    ImageCache(imgs[:2], device=dev)  # warm-up: pinned allocator, first copy
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cache = ImageCache(imgs, device=dev)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"height": H, "width": W, "channels": C, "images": n, "seconds": dt, "images_per_s": n / dt,
            "gb_per_s": cache.nbytes / dt / 1e9}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="+", default=["1920x1080", "3840x2160"])
    ap.add_argument("--factors", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--upload-images", type=int, default=16)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "target_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("target_bench: no GPU -- nothing is timed on the CPU")
    dev = torch.device(a.device)
    rows, uploads, caches = [], [], []
    for size in a.sizes:
        W, H = (int(v) for v in size.lower().split("x"))
        for C in (4, 3):
            caches.append({"height": H, "width": W, "channels": C, "factors": a.factors,
                           "bytes_per_view": cache_bytes_per_view(H, W, C, a.factors)})
            for d in a.factors:
                rows.append(bench_shape(H, W, C, d, dev, a.calls, a.repeats))
                print(json.dumps(rows[-1]), flush=True)
            uploads.append(bench_upload(H, W, C, a.upload_images, dev))
            print(json.dumps(uploads[-1]), flush=True)
    rec = {"device": torch.cuda.get_device_name(dev), "calls_per_window": a.calls, "repeats": a.repeats,
           "hbm_peak_bytes_per_s": HBM_PEAK, "hbm_float4_copy_bytes_per_s": HBM_COPY,
           "paths": {"a": "fused_target: addcmul of cached float planes (RGBA) / downscale_image of the float image (RGB)",
                     "b": "per-step resize + composite on the float RGBA image",
                     "c": "gs_fused.target_from_u8 on the uint8 image"},
           "targets": rows, "cache": caches, "upload": uploads}
    os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
    with open(a.output, "w", encoding="utf-8") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({"wrote": a.output, "rows": len(rows)}))
    return rec


if __name__ == "__main__":
    main()
