"""The bilateral-grid slice on the device: gs_fused.bilagrid_slice (csrc/bilagrid.hip) next to the torch-op route a
user would otherwise write (F.grid_sample over the channel-first volume + the affine map), medians by device events;
and what the feature costs and buys in training.  Needs an MI355X: there is no CPU path.

    python tools/bilagrid_bench.py [--reps 50] [--train-iters 7000] [--no-train] [--out profiles/bilagrid_bench.json]

Reported (one JSON line):
  slice_ms     per size (480x270, 1920x1080; grid 16x16x8, 48 views): forward alone and forward + backward of both
               routes, alternated in one process (ms per call: median, 10th / 90th percentile), the speed-up of the
               medians, the largest difference of the two routes' outputs and gradients, and whether two runs of each
               route give the same gradient bits;
  errors       e(X) = max |X - X64| / max |X64| of the kernel and of the float32 CPU restatement against the float64
               CPU restatement, over the shapes of tests/test_gpu_bilagrid.py (the largest per output);
  train        config 3 of the bench at full size over a fixed background with view_exposure = (0.15, 0.03):
               iterations/s and the PSNR on the TRUE images with the grids off, on, and off again; and config 3 as the
               reference runs it (coarse-to-fine, random background) without exposure error, grids off / on: the
               step cost of the feature alone.
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-splatting-toolkit_amd"), os.path.join(ROOT, "tests")]
import torch
import torch.nn.functional as F


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


def torch_slice(grids, rgb, view):
    """The torch-op route on the device: what tests/_bilagrid_ref.py states, from the same channel-last parameter."""
    H, W, _ = rgb.shape
    x = ((torch.arange(W, device=rgb.device, dtype=rgb.dtype) + 0.5) / W)[None, :].expand(H, W)
    y = ((torch.arange(H, device=rgb.device, dtype=rgb.dtype) + 0.5) / H)[:, None].expand(H, W)
    g = 0.299 * rgb[..., 0] + 0.587 * rgb[..., 1] + 0.114 * rgb[..., 2]
    xyz = torch.stack((x, y, g), dim=-1)
    vol = grids[view:view + 1].permute(0, 4, 1, 2, 3)
    m = F.grid_sample(vol, (2.0 * (xyz - 0.5))[None, None], mode="bilinear", align_corners=True, padding_mode="border")
    m = m[0, :, 0].permute(1, 2, 0).reshape(H, W, 3, 4)
    return (m[..., :3] * rgb[..., None, :]).sum(-1) + m[..., 3]


def slice_rows(reps):
    import gs_fused
    import _bilagrid_ref as B

    dev = torch.device("cuda", 0)
    rows = {}
    for size, (h, w) in (("480x270", (270, 480)), ("1920x1080", (1080, 1920))):
        gen = torch.Generator().manual_seed(h)
        grids = (B.identity_grids(48, 16, 16, 8) + 0.1 * torch.randn((48, 8, 16, 16, 12), generator=gen)).to(dev)
        grids.requires_grad_(True)
        rgb = B.draw_rgb(h, w, 8, gen).to(dev).requires_grad_(True)
        v_out = torch.randn((h, w, 3), generator=gen).to(dev)
        routes = {"hip": lambda: gs_fused.bilagrid_slice(grids, rgb, 17), "torch": lambda: torch_slice(grids, rgb, 17)}

        def both(fn):
            grids.grad = rgb.grad = None
            fn().backward(v_out)
            return grids.grad, rgb.grad

        def forward(fn):
            with torch.no_grad():
                return fn()

        t_f = alternate({k: (lambda fn=fn: forward(fn)) for k, fn in routes.items()}, reps)
        t_fb = alternate({k: (lambda fn=fn: both(fn)) for k, fn in routes.items()}, reps)
        row = {"forward": {k: summary(v) for k, v in t_f.items()}, "forward_backward": {k: summary(v) for k, v in t_fb.items()}}
        for part in ("forward", "forward_backward"):
            row[part]["speedup_median"] = row[part]["torch"]["median"] / row[part]["hip"]["median"]
        row["backward_by_difference"] = {k: row["forward_backward"][k]["median"] - row["forward"][k]["median"]
                                         for k in routes}
        outs = {k: forward(fn) for k, fn in routes.items()}
        grads = {k: [g.clone() for g in both(fn)] for k, fn in routes.items()}
        again = {k: both(fn) for k, fn in routes.items()}
        row["max_abs_difference"] = {"out": float((outs["hip"] - outs["torch"]).abs().max()),
                                     "v_grids": float((grads["hip"][0] - grads["torch"][0]).abs().max()),
                                     "v_rgb": float((grads["hip"][1] - grads["torch"][1]).abs().max())}
        row["v_grids_bit_equal_over_two_runs"] = {k: bool(torch.equal(grads[k][0], again[k][0])) for k in routes}
        rows[size] = row
    return rows


def error_rows():
    import _bilagrid_ref as B
    import gs_fused

    dev = torch.device("cuda", 0)
    worst = {"kernel": [0.0, 0.0, 0.0], "float32_restatement": [0.0, 0.0, 0.0], "largest_ratio": [0.0, 0.0, 0.0]}
    for (h, w) in ((1, 1), (5, 7), (37, 53), (64, 64), (270, 480)):
        for (gw, gh, gl) in ((2, 2, 2), (3, 2, 5), (16, 16, 8), (64, 64, 16)):
            (grids, rgb, v_out), want, base = B.slice_case(h, w, gw, gh, gl, 1)
            a, x = grids.to(dev).requires_grad_(True), rgb.to(dev).requires_grad_(True)
            out = gs_fused.bilagrid_slice(a, x, 1)
            out.backward(v_out.to(dev))
            for i, (got, w64, b32) in enumerate(zip((out.detach(), x.grad, a.grad), want, base)):
                e, e32 = B.rel_err(got, w64), B.rel_err(b32, w64)
                worst["kernel"][i] = max(worst["kernel"][i], e)
                worst["float32_restatement"][i] = max(worst["float32_restatement"][i], e32)
                worst["largest_ratio"][i] = max(worst["largest_ratio"][i], e / (4.0 * e32 + B.ULP))
    return {k: dict(zip(("out", "v_rgb", "v_grids"), v)) for k, v in worst.items()}


def train_rows(iters):
    import bench
    from harness.train import train

    dev = torch.device("cuda", 0)
    rows = {"exposure_full_size_fixed_background": {}, "reference_schedule_no_exposure": {}}
    full = dataclasses.replace(bench.config3(iters=iters, schedule="full"), view_exposure=(0.15, 0.03))
    for name, on in (("off", False), ("on", True), ("off_again", False)):
        res = train(dataclasses.replace(full, bilateral_grid=on), dev)
        rows["exposure_full_size_fixed_background"][name] = {
            "iters_per_s": res["iters_per_s"], "psnr_true_start": res["psnr_start"], "psnr_true_end": res["psnr_end"],
            "last_loss": res["losses"][-1], "num_gaussians_end": res["num_gaussians_end"],
            "grids_max_abs_from_identity": max(res["bilateral_grid"]["max_abs_from_identity"]) if on else None}
    ref = bench.config3(iters=iters)
    for name, on in (("off", False), ("on", True)):
        res = train(dataclasses.replace(ref, bilateral_grid=on), dev)
        rows["reference_schedule_no_exposure"][name] = {"iters_per_s": res["iters_per_s"], "psnr_end": res["psnr_end"],
                                                        "num_gaussians_end": res["num_gaussians_end"]}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--train-iters", type=int, default=7000)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--no-errors", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bilagrid_bench needs a GPU")
    out = {"slice_ms": slice_rows(args.reps)}
    if not args.no_errors:
        out["errors"] = error_rows()
    if not args.no_train:
        out["train"] = train_rows(args.train_iters)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
