"""The records behind DESIGN.md section 4.16 (absgrad): what the `ABS` instance of the compositing backward costs, and
what the switch does to a training run.  Each sub-command merges its record into one JSON file
(default `profiles/absgrad_bench.json`).

    python tools/absgrad_bench.py kernel [--rounds K]
        Two workloads, backward with the switch off and on alternating:
          default   the bench default (1 M Gaussians, 1920x1080, `harness.scene.make_scene(seed=42)`)
          young     config 3's model as it starts (200 k seeded Gaussians), one of its cameras at 480x270
        Times forward + backward pairs with device events (host launch path included).  For the kernel alone run it
        under a kernel trace of its own and reduce that:
          rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/absgrad_bench.py kernel
          python tools/absgrad_bench.py trace DIR
        The off / on instances carry different template arguments (`<4, false, false, false>` / `<.., true>`) and the
        two workloads different grids, so one trace holds all four figures.

    python tools/absgrad_bench.py train [--iters N] [--thresholds 2e-4 4e-4 8e-4]
        Config 3 of the bench with `absgrad` off (the reference's threshold) and on at each threshold, same seed:
        final PSNR, N and iterations/s.
"""
import argparse
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-splatting-toolkit_amd")]
import numpy as np  # noqa: E402


def merge(path, key, record):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[key] = record
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({key: record}))


def _workloads(dev):
    """-> {name: (step(absgrad) -> None, description)}: one forward + backward through the separate ops."""
    import torch

    import bench
    from harness import scene as S
    from harness.pipeline import CameraTensors, render_view
    from harness.train import initial_model, orbit_cameras

    out = {}
    cam = S.make_camera(1920, 1080)
    sc = S.make_scene(1_000_000, cam, sh_degree=3, seed=42, scale_lo=0.0025, scale_hi=0.025)
    p = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in sc.items()}
    camt = CameraTensors.from_numpy(cam, dev)
    bg = torch.tensor(S.BACKGROUND, device=dev)
    v_img, _ = S.make_cotangents(cam)
    v_img = torch.from_numpy(v_img).to(dev)

    def default(absgrad):
        for t in p.values():
            t.grad = None
        o = render_view(p["means3d"], p["scales"], p["quats"], p["opacities"], p["sh_coeffs"], camt, bg, 3,
                        clamp_rgb=False, absgrad=absgrad)
        o["rgb"].backward(v_img)

    out["default"] = (default, "1 M Gaussians, 1920x1080, make_scene(seed=42)")

    cfg = bench.config3(iters=1)
    model = initial_model(cfg, dev)
    cam_y = CameraTensors.from_numpy(orbit_cameras(cfg.num_views, 480, 270, radius=cfg.cam_radius)[0], dev)
    v_y = torch.rand(270, 480, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(0)) * 2 - 1

    def young(absgrad):
        for t in model.gauss.values():
            t.grad = None
        o = model.render(cam_y, bg, 0, clamp_rgb=False, absgrad=absgrad)
        o["rgb"].backward(v_y)

    out["young"] = (young, f"config 3's initial model ({model.num_points} Gaussians), 480x270")
    return out


def kernel(a):
    import torch

    dev = torch.device("cuda:0")
    rec = {}
    for name, (step, what) in _workloads(dev).items():
        for _ in range(3):
            step(False), step(True)
        torch.cuda.synchronize()
        ms = {False: [], True: []}
        for _ in range(a.rounds):
            for flag in (False, True):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(flag)
                e1.record()
                torch.cuda.synchronize()
                ms[flag].append(e0.elapsed_time(e1))
        rec[name] = {"what": what, "rounds": a.rounds,
                     "forward_backward_ms_median": {"off": round(float(np.median(ms[False])), 4),
                                                    "on": round(float(np.median(ms[True])), 4)}}
    merge(a.out, "kernel_events", rec)


def trace(a):
    """Reduce a kernel trace of `kernel` to the compositing backward's instances, per grid."""
    rows = []
    for f in glob.glob(os.path.join(a.dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    groups = {}
    for r in rows:
        m = re.search(r"raster_bwd_tile16_kernel<([^>]*)>", r["Kernel_Name"])
        if not m:
            continue
        grid = r.get("Grid_Size") or r.get("Grid_Size_X", "?")
        groups.setdefault((m.group(1).replace(" ", ""), str(grid)), []).append(
            (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    rec = []
    for (targs, grid), us in sorted(groups.items(), key=lambda kv: (int(kv[0][1]) if kv[0][1].isdigit() else 0, kv[0][0])):
        us = np.array(us[len(us) // 4:])  # (the first quarter: warm-up)
        rec.append({"instance": f"raster_bwd_tile16_kernel<{targs}>", "abs": targs.endswith("true"), "grid_size": grid,
                    "launches": int(us.size), "us_median": round(float(np.median(us)), 2),
                    "us_p10_p90": [round(float(np.percentile(us, 10)), 2), round(float(np.percentile(us, 90)), 2)]})
    merge(a.out, "kernel_trace", rec)


def train(a):
    import dataclasses

    import torch

    import bench
    from harness.train import train as run

    dev = torch.device("cuda:0")
    rows = []
    for absgrad, thresh in [(False, None)] + [(True, t) for t in a.thresholds]:
        cfg = bench.config3(iters=a.iters)
        if thresh is not None:
            cfg = dataclasses.replace(cfg, refine=dataclasses.replace(cfg.refine, densify_grad_thresh=thresh))
        cfg = dataclasses.replace(cfg, absgrad=absgrad)
        res = run(cfg, dev)
        rows.append({"absgrad": absgrad, "densify_grad_thresh": res["densify_grad_thresh"],
                     "psnr_end": round(res["psnr_end"], 3), "num_gaussians_end": res["num_gaussians_end"],
                     "iters_per_s": round(res["iters_per_s"], 1), "iters": a.iters, "seed": cfg.seed})
        print(json.dumps(rows[-1]), flush=True)
    merge(a.out, "train_config3", rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "absgrad_bench.json"))
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--rounds", type=int, default=30)
    t = sub.add_parser("trace")
    t.add_argument("dir")
    r = sub.add_parser("train")
    r.add_argument("--iters", type=int, default=7000)
    r.add_argument("--thresholds", type=float, nargs="*", default=[2e-4, 4e-4, 8e-4])
    a = ap.parse_args()
    {"kernel": kernel, "trace": trace, "train": train}[a.cmd](a)


if __name__ == "__main__":
    main()
