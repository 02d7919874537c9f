"""The records behind DESIGN.md section 4.20 (depth distortion and median depth).  Each sub-command merges its record
into one JSON file (default `profiles/distortion_bench.json`).

    python tools/distortion_bench.py kernel [--rounds K] [--ply MODEL.ply]
        The new pass (gs_fused.depth_distortion) against the 3-channel `rasterize_gaussians` pass over the SAME cached
        tile lists, forward and forward + backward, device events around the calls (host launch path included):
          default   the bench default (1 M Gaussians, 1920x1080, `harness.scene.make_scene(seed=42)`)
          trained   with --ply: a trained model (the trainer's `export_ply`), config 3's first camera at 1920x1080
        and the same term as dense torch ops (all pairs of a ray's Gaussians, [P,N,N]) at a size where that fits:
        64 x 64 pixels, 256 Gaussians, without the skip and stop rules.

    python tools/distortion_bench.py train [--iters N] [--lambdas 100 10 1]
        Config 3 of the bench with `depth_distortion` off and on at each `distortion_lambda` (the term from iteration
        `--start`), same seed: iterations/s, final PSNR, final N and the term.
"""
import argparse
import json
import os
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


def _time(fn, rounds):
    import torch

    for _ in range(3):
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


def _view_record(p, camt, rounds, what):
    """Project once; then the two passes on the projection's outputs (every call after the first hits the list cache)."""
    import torch

    from gs_fused import depth_distortion
    from rasterizer import rasterize_gaussians
    from rasterizer.project_gaussians import project_gaussians

    H, W = camt.height, camt.width
    dev = p["means3d"].device
    with torch.no_grad():
        xys, depths, radii, conics, _, tiles, _ = project_gaussians(
            p["means3d"], p["scales"], 1, p["quats"], camt.viewmat[:3, :], camt.projmat, camt.fx, camt.fy, camt.cx,
            camt.cy, H, W, 16)
    g = torch.Generator(device=dev).manual_seed(0)
    colors = torch.rand((xys.shape[0], 3), device=dev, generator=g)
    v_img = torch.rand((H, W, 3), device=dev, generator=g) * 2 - 1
    v_d = torch.rand((H, W), device=dev, generator=g) * 2 - 1
    bg = torch.zeros(3, device=dev)
    opac = p["opacities"].detach()
    leaves = [t.detach().clone().requires_grad_(True) for t in (xys, conics, colors, opac, depths)]

    def rgb(backward):
        xy, co, col, op, _ = leaves if backward else [t.detach() for t in leaves]
        img = rasterize_gaussians(xy, depths, radii, co, tiles, col, op, H, W, 16, background=bg)
        if backward:
            torch.autograd.grad((img * v_img).sum(), [xy, co, col, op])

    def dist(backward):
        xy, co, _, op, z = leaves if backward else [t.detach() for t in leaves]
        d, _ = depth_distortion(xy, depths, radii, co, tiles, z, op, H, W)
        if backward:
            torch.autograd.grad((d * v_d).sum(), [xy, co, z, op])

    rec = {"what": what, "rounds": rounds, "num_gaussians": int(xys.shape[0]),
           "list_entries": None,
           "rgb_forward_ms": _time(lambda: rgb(False), rounds), "rgb_forward_backward_ms": _time(lambda: rgb(True), rounds),
           "distortion_forward_ms": _time(lambda: dist(False), rounds),
           "distortion_forward_backward_ms": _time(lambda: dist(True), rounds)}
    from rasterizer import rasterize as R

    rec["list_entries"] = int(R._cache_snapshot()["value"].num_intersects)
    rec["forward_ratio"] = round(rec["distortion_forward_ms"] / rec["rgb_forward_ms"], 3)
    rec["forward_backward_ratio"] = round(rec["distortion_forward_backward_ms"] / rec["rgb_forward_backward_ms"], 3)
    return rec


def _dense_record(rounds, dev):
    """The term as dense torch ops: alpha [P,N] in depth order, T by cumprod, all pairs |z_i - z_j| [N,N]."""
    import torch

    from gs_fused import depth_distortion
    from rasterizer.project_gaussians import project_gaussians

    from harness import scene as S
    from harness.pipeline import CameraTensors

    cam = S.make_camera(64, 64)
    sc = S.make_scene(256, cam, sh_degree=0, seed=1, scale_lo=0.02, scale_hi=0.15)
    camt = CameraTensors.from_numpy(cam, dev)
    t = {k: torch.from_numpy(v).to(dev) for k, v in sc.items()}
    with torch.no_grad():
        xys, depths, radii, conics, _, tiles, _ = project_gaussians(
            t["means3d"], t["scales"], 1, t["quats"], camt.viewmat[:3, :], camt.projmat, camt.fx, camt.fy, camt.cx, camt.cy,
            64, 64, 16)
    keep = radii > 0
    order = torch.argsort(depths[keep])
    xy0, co0, op0, z0 = (a[keep][order].clone() for a in (xys, conics, t["opacities"].reshape(-1), depths))
    py, px = torch.meshgrid(torch.arange(64, device=dev, dtype=torch.float32),
                            torch.arange(64, device=dev, dtype=torch.float32), indexing="ij")
    px, py = px.reshape(-1, 1), py.reshape(-1, 1)
    v_d = torch.rand((64 * 64,), device=dev, generator=torch.Generator(device=dev).manual_seed(0))

    def dense(backward):
        xy, co, op, z = [a.clone().requires_grad_(backward) for a in (xy0, co0, op0, z0)]
        dx, dy = xy[:, 0][None] - px, xy[:, 1][None] - py
        sigma = 0.5 * (co[:, 0][None] * dx * dx + co[:, 2][None] * dy * dy) + co[:, 1][None] * dx * dy
        alpha = torch.clamp(op[None] * torch.exp(-sigma), max=0.999)
        alpha = torch.where(alpha < 1 / 255, torch.zeros_like(alpha), alpha)
        T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1 - alpha[:, :-1]], 1), 1)
        w = alpha * T
        d = torch.einsum("pi,ij,pj->p", w, (z[:, None] - z[None, :]).abs(), w)
        if backward:
            torch.autograd.grad((d * v_d).sum(), [xy, co, op, z])

    leaves = [a.detach().clone().requires_grad_(True) for a in (xys, conics, t["opacities"], depths)]

    def hip(backward):
        xy, co, op, z = leaves if backward else [a.detach() for a in leaves]
        d, _ = depth_distortion(xy, depths, radii, co, tiles, z, op, 64, 64)
        if backward:
            torch.autograd.grad((d.reshape(-1) * v_d).sum(), [xy, co, op, z])

    return {"what": f"64 x 64, {int(keep.sum())} Gaussians on screen, no skip / stop rule in the dense form",
            "rounds": rounds,
            "torch_forward_ms": _time(lambda: dense(False), rounds), "torch_forward_backward_ms": _time(lambda: dense(True), rounds),
            "hip_forward_ms": _time(lambda: hip(False), rounds), "hip_forward_backward_ms": _time(lambda: hip(True), rounds)}


def kernel(a):
    import torch

    from harness import scene as S
    from harness.pipeline import CameraTensors

    dev = torch.device("cuda:0")
    rec = {}
    cam = S.make_camera(1920, 1080)
    sc = S.make_scene(1_000_000, cam, sh_degree=0, seed=42, scale_lo=0.0025, scale_hi=0.025)
    p = {k: torch.from_numpy(v).to(dev) for k, v in sc.items()}
    rec["default"] = _view_record(p, CameraTensors.from_numpy(cam, dev), a.rounds,
                                  "1 M Gaussians, 1920x1080, make_scene(seed=42)")
    if a.ply:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bench
        from export_tsdf import activated
        from gs_io import read_gaussian_ply
        from harness.train import orbit_cameras

        cfg = bench.config3(iters=1)
        camt = CameraTensors.from_numpy(orbit_cameras(cfg.num_views, 1920, 1080, radius=cfg.cam_radius)[0], dev)
        rec["trained"] = _view_record(activated(read_gaussian_ply(a.ply), dev), camt, a.rounds,
                                      f"{os.path.basename(a.ply)}, config 3's first camera at 1920x1080")
    rec["dense_torch"] = _dense_record(a.rounds, dev)
    merge(a.out, "kernel_events", rec)


def train(a):
    import dataclasses

    import torch

    import bench
    from harness.train import train as run

    dev = torch.device("cuda:0")
    rows = []
    for lam in [None] + list(a.lambdas):
        on = lam is not None
        cfg = dataclasses.replace(bench.config3(iters=a.iters), depth_distortion=on, distortion_start_iteration=a.start,
                                  **({"distortion_lambda": lam} if on else {}),
                                  **({"export_ply": a.export_ply} if (a.export_ply and on and lam == a.lambdas[0]) else {}))
        res = run(cfg, dev)
        rows.append({"depth_distortion": on, "start_iteration": a.start, "iters": a.iters, "seed": cfg.seed,
                     "iters_per_s": round(res["iters_per_s"], 1), "psnr_end": round(res["psnr_end"], 3),
                     "num_gaussians_end": res["num_gaussians_end"], **({"term": res["depth_distortion"]} if on else {})})
        print(json.dumps(rows[-1]), flush=True)
    merge(a.out, "train_config3", rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distortion_bench.json"))
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernel")
    k.add_argument("--rounds", type=int, default=20)
    k.add_argument("--ply", default=None, help="a trained model (the trainer's export_ply)")
    t = sub.add_parser("train")
    t.add_argument("--iters", type=int, default=7000)
    t.add_argument("--start", type=int, default=3000)
    t.add_argument("--lambdas", type=float, nargs="+", default=[100.0], help="one run with the option per value")
    t.add_argument("--export-ply", default=None, help="write the model trained with the option here")
    a = ap.parse_args()
    {"kernel": kernel, "train": train}[a.cmd](a)


if __name__ == "__main__":
    main()
