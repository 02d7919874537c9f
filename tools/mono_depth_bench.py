"""The monocular-depth terms of the co-gs loss on the device: the fused heads (gs_fused.local_pearson_loss,
log_depth_loss, tv_loss; csrc/mono_depth.hip) next to harness/cogs_losses.py's torch ops, medians by device events.

    python tools/mono_depth_bench.py [--reps 30] [--train-iters 200] [--out profiles/mono_depth_bench.json]

Reported (one JSON line):
  heads_ms           per term and size (1920x1080, 3840x2160; box 128, p_corr 0.5): forward + backward of the fused head
                     and of the torch version in the same process, alternated (ms per call, median and the 10th / 90th
                     percentile), the two losses, and for the fused head the bytes its kernels must move at the least
                     over its time as a fraction of the 8 TB/s HBM peak;
  cogs_iters_per_s   harness.train's co-gs loop with use_est_depth + use_pearson_depth + use_scaled_est_depth +
                     using_tv_loss at 96x64 and 1920x1080, `fused_mono_depth` off / on / off again.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-splatting-toolkit_amd")]
import torch

HBM_PEAK = 8.0e12


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fns, reps, warmup=5):
    """{name: sorted times in ms}: the candidates take turns, so that what else runs on the machine hits them alike."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(timed(fn))
    return {k: sorted(v) for k, v in times.items()}


def summary(ts):
    return {"median": statistics.median(ts), "p10": ts[len(ts) // 10], "p90": ts[(9 * len(ts)) // 10]}


def smooth(h, w, dev, seed, channels=1):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.rand((1, channels, h // 8, w // 8), device=dev, generator=g)
    x = torch.nn.functional.interpolate(x, size=(h, w), mode="bicubic", align_corners=False)
    return x[0].permute(1, 2, 0).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--train-iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mono_depth_bench needs a GPU")
    import gs_fused
    from harness import cogs_losses as CL
    from harness.train import TrainConfig, train

    dev = torch.device("cuda", 0)
    box = 128
    out = {"heads_ms": {}, "cogs_iters_per_s": {}}
    for size, (h, w) in (("1080p", (1080, 1920)), ("4k", (2160, 3840))):
        gt = 3.0 + smooth(h, w, dev, 1)[..., 0] + 0.01 * torch.rand((h, w), device=dev)
        pred = (0.9 * gt + 0.2 + 0.01 * torch.rand((h, w), device=dev)).requires_grad_(True)
        img = smooth(h, w, dev, 2, channels=3).clamp(0, 1)
        rows, cols = CL.local_pearson_patches(h, w, box, 0.5, torch.Generator(device=dev).manual_seed(3), dev)
        n_corr, px = int(rows.numel()), h * w
        heads = {
            "local_pearson": (lambda: gs_fused.local_pearson_loss(pred, gt, box, rows, cols),
                              lambda: CL.local_pearson_loss(pred, gt, box, 0.5, corners=(rows, cols)),
                              # forward: two images over every patch (the second pass from L2); backward: two images, v_pred
                              4.0 * (2 * n_corr * box * box + 3 * px)),
            "log_depth": (lambda: gs_fused.log_depth_loss(pred, gt, img, 0.9, 0.1),
                          lambda: CL.scaled_log_depth_loss(pred, gt, img, 0.9, 0.1),
                          4.0 * px * (5 + 5 + 1)),     # pred, gt, image each way, v_pred
            "tv": (lambda: gs_fused.tv_loss(pred), lambda: CL.tv_loss(pred), 4.0 * px * 3),
        }
        out["heads_ms"][size] = {"patches": n_corr}
        for name, (fused, plain, least_bytes) in heads.items():
            def step(fn):
                pred.grad = None
                fn().backward()

            t = alternate({"fused": lambda: step(fused), "torch": lambda: step(plain)}, args.reps)
            with torch.no_grad():
                losses = {"fused": float(fused()), "torch": float(plain())}
            row = {k: summary(v) for k, v in t.items()}
            row["loss"] = losses
            row["speedup_median"] = row["torch"]["median"] / row["fused"]["median"]
            row["fused_hbm_fraction_of_peak"] = least_bytes / (row["fused"]["median"] * 1e-3) / HBM_PEAK
            out["heads_ms"][size][name] = row
    for size, kw in (("96x64", dict(num_gaussians=2000, width=96, height=64, local_patch_size=16, sh_degree=1)),
                     ("1080p", dict(num_gaussians=200_000, width=1920, height=1080, local_patch_size=128, sh_degree=3))):
        out["cogs_iters_per_s"][size] = {}
        for name, on in (("off", False), ("on", True), ("off_again", False)):
            # (cam_radius 2: the scene fills the frame -- a patch of empty background is 0 / 0 in the local Pearson)
            cfg = TrainConfig(model="co-gs", num_views=8, iters=args.train_iters, depth_loss_start_iteration=10,
                              background_color="random", densify=False, scene_scale=(0.15, 0.5) if size == "96x64"
                              else (0.01, 0.06), cam_radius=2.0, use_est_depth=True, use_pearson_depth=True,
                              use_scaled_est_depth=True, using_tv_loss=True, fused_mono_depth=on, log_every=50, **kw)
            res = train(cfg, dev)
            out["cogs_iters_per_s"][size][name] = {"iters_per_s": res["iters_per_s"], "last_loss": res["losses"][-1]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
