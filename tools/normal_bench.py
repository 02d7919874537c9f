"""The depth-normal consistency head and the per-Gaussian normals on the device: gs_fused.normal_consistency_loss /
gaussian_normals (csrc/normals.hip) next to the same rule written as torch ops (tests/_normals_ref.py in float32 on
the device -- what a user would otherwise write), medians by device events; and what the option costs and buys in
training.  Needs an MI355X: there is no CPU path.

    python tools/normal_bench.py [--reps 50] [--train-iters 7000] [--no-train] [--out profiles/normal_bench.json]

Reported (one JSON line):
  loss_ms      per size (480x270, 1920x1080): forward alone and forward + backward of both routes, alternated in one
               process (ms per call: median, 10th / 90th percentile), the speed-up of the medians, the largest difference
               of the two routes' loss and gradients, and whether two runs of each route give the same gradient bits;
  gaussians_ms the per-Gaussian normals at 1 M Gaussians, forward and forward + backward, both routes;
  errors       e(X) = max |X - X64| / max |X64| of the kernels and of the float32 CPU restatement against the float64
               CPU restatement over the shapes of tests/test_gpu_normals.py (the largest per output);
  train        config 3 of the bench as the reference runs it (coarse-to-fine, random background), the option off, on
               with `normal_start_iteration` at half of the run, and off again: iterations/s, PSNR, the term's first and
               last value, the median phase times of the sampled steps; and the share of a step the third compositing
               pass and the head take, from the on / off iteration rates of the steps after the start.
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


def compare(routes, leaves, reps):
    """routes: {name: fn() -> scalar}; leaves: the tensors whose .grad the backward fills."""
    def forward(fn):
        with torch.no_grad():
            return fn()

    def both(fn):
        for t in leaves:
            t.grad = None
        fn().backward()
        return [t.grad for t in leaves]

    t_f = alternate({k: (lambda fn=fn: forward(fn)) for k, fn in routes.items()}, reps)
    t_fb = alternate({k: (lambda fn=fn: both(fn)) for k, fn in routes.items()}, reps)
    row = {"forward": {k: summary(v) for k, v in t_f.items()}, "forward_backward": {k: summary(v) for k, v in t_fb.items()}}
    for part in ("forward", "forward_backward"):
        row[part]["speedup_median"] = row[part]["torch"]["median"] / row[part]["hip"]["median"]
    outs = {k: float(forward(fn)) for k, fn in routes.items()}
    grads = {k: [g.clone() for g in both(fn)] for k, fn in routes.items()}
    again = {k: both(fn) for k, fn in routes.items()}
    row["max_abs_difference"] = {"out": abs(outs["hip"] - outs["torch"]),
                                 "grads": [float((a - b).abs().max()) for a, b in zip(grads["hip"], grads["torch"])]}
    row["grads_bit_equal_over_two_runs"] = {k: all(bool(torch.equal(a, b)) for a, b in zip(grads[k], again[k]))
                                            for k in routes}
    return row


def loss_rows(reps):
    import _normals_ref as R
    import gs_fused

    dev = torch.device("cuda", 0)
    rows = {}
    for size, (h, w) in (("480x270", (270, 480)), ("1920x1080", (1080, 1920))):
        case = R.image_case(h, w, h, True)
        depth = case["depth"].to(dev).requires_grad_(True)
        nimg = case["nimg"].to(dev).requires_grad_(True)
        alpha, mask, K = case["alpha"].to(dev), case["mask"].to(dev), case["K"]
        rows[size] = compare({"hip": lambda: gs_fused.normal_consistency_loss(nimg, depth, alpha, *K, mask=mask),
                              "torch": lambda: R.normal_consistency_loss(nimg, depth, alpha, *K, mask=mask,
                                                                         dtype=torch.float32)}, [nimg, depth], reps)
        rows[size]["bytes_streamed"] = {"forward": h * w * 4 * 6, "backward": h * w * 4 * 10}
    return rows


def gaussian_rows(reps, n=1_000_000):
    import _normals_ref as R
    import gs_fused

    dev = torch.device("cuda", 0)
    case, _ = R.gaussian_case(n, 7)
    q = case["quats"].to(dev).requires_grad_(True)
    s, m, V = case["scales"].to(dev), case["means"].to(dev), case["viewmat"].to(dev)
    w = torch.randn((n, 3), generator=torch.Generator().manual_seed(1)).to(dev)
    row = compare({"hip": lambda: (gs_fused.gaussian_normals(q, s, m, V) * w).sum(),
                   "torch": lambda: (R.gaussian_normals(q, s, m, V, dtype=torch.float32)[0] * w).sum()}, [q], reps)
    row["num_gaussians"] = n
    return row


def error_rows():
    import _normals_ref as R
    import gs_fused

    dev = torch.device("cuda", 0)
    keys = ("normals", "loss", "v_nimg", "v_depth")
    worst = {"kernel": dict.fromkeys(keys, 0.0), "float32_restatement": dict.fromkeys(keys, 0.0),
             "largest_share_of_the_bound": dict.fromkeys(keys, 0.0)}
    for (h, w) in ((3, 3), (5, 7), (17, 33), (64, 64), (270, 480)):
        for masked in (False, True):
            case = R.image_case(h, w, 100 + h, masked)
            want = R.image_reference(case)
            nimg, depth = case["nimg"].to(dev).requires_grad_(True), case["depth"].to(dev).requires_grad_(True)
            alpha = case["alpha"].to(dev)
            loss = gs_fused.normal_consistency_loss(nimg, depth, alpha, *case["K"],
                                                    mask=None if not masked else case["mask"].to(dev))
            loss.backward()
            got = {"normals": gs_fused.depth_to_normal(depth.detach(), alpha, *case["K"]), "loss": loss.detach().reshape(1),
                   "v_nimg": nimg.grad, "v_depth": depth.grad}
            for k in keys:
                e, e32 = R.rel_err(got[k].cpu(), want[k]), want["e32"][k]
                worst["kernel"][k] = max(worst["kernel"][k], e)
                worst["float32_restatement"][k] = max(worst["float32_restatement"][k], e32)
                worst["largest_share_of_the_bound"][k] = max(worst["largest_share_of_the_bound"][k],
                                                             e / (4.0 * e32 + 2.0 ** -23))
    return worst


def train_rows(iters):
    import bench
    from harness.train import train

    dev = torch.device("cuda", 0)
    ref = bench.config3(iters=iters)
    start = iters // 2
    rows = {"normal_start_iteration": start}
    for name, on in (("off", False), ("on", True), ("off_again", False)):
        res = train(dataclasses.replace(ref, normal_consistency=on, normal_start_iteration=start), dev)
        print(f"train {name}: {res['iters_per_s']:.1f} iterations/s, PSNR {res['psnr_end']:.2f} dB", file=sys.stderr, flush=True)
        rows[name] = {"iters_per_s": res["iters_per_s"], "seconds": res["seconds"], "psnr_start": res["psnr_start"],
                      "psnr_end": res["psnr_end"], "num_gaussians_end": res["num_gaussians_end"],
                      "phase_ms_median": res.get("phase_ms_median"),
                      "phase_ms_median_by_resolution": res.get("phase_ms_median_by_resolution"),
                      "normal_consistency": res.get("normal_consistency")}
    # the seconds the option adds, over the steps that had it: its share of such a step
    base = 0.5 * (rows["off"]["seconds"] + rows["off_again"]["seconds"])
    extra = rows["on"]["seconds"] - base
    steps_on = iters - start - 1
    rows["added_ms_per_step_with_the_term"] = 1e3 * extra / max(steps_on, 1)
    rows["spread_of_the_two_off_runs_s"] = abs(rows["off"]["seconds"] - rows["off_again"]["seconds"])
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
        raise SystemExit("normal_bench needs a GPU")
    out = {"loss_ms": loss_rows(args.reps), "gaussians_ms": gaussian_rows(args.reps)}
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
