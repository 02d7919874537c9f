"""The records behind DESIGN.md section 4.22 (Mip-Splatting's 3D smoothing filter).  Each sub-command merges its record
into one JSON file (default `profiles/filter3d_bench.json`).

    python tools/filter3d_bench.py sampling [--n 1000000] [--views 48 300] [--rounds K]
        The sampling pass (`gs_fused.sampling_filter_3d`, three launches) at N Gaussians and V cameras, device events
        around the call (host launch path included), against the same rule written as torch ops looping over the
        cameras; and whether the two agree bit for bit (the torch ops contract nothing either).

    python tools/filter3d_bench.py activation [--n 1000000] [--rounds K]
        `activate_gaussians(filter_3d=...)` forward and forward + backward against the unfiltered kernels and against
        `apply_filter_3d` (torch ops) on top of the unfiltered kernels.

    python tools/filter3d_bench.py train [--iters 7000]
        Config 3 of the bench trained at a quarter of the resolution THROUGHOUT and evaluated at full resolution
        (Mip-Splatting's single-scale training, zoom-in test), in antialiased mode, without and with the filter, same
        seed: PSNR at full resolution, iterations/s, final N.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-splatting-toolkit_amd")]
import numpy as np  # noqa: E402

from distortion_bench import _time, merge  # noqa: E402


def sampling_torch(means, table, variance=0.2, near=0.2, margin=0.15):
    """The rule of gsr_filter3d_sampling as torch ops, one camera at a time (float32; every op rounds on its own).
    The two divisions with a constant numerator divide a 0-dim TENSOR: `scalar / tensor` is `tensor.reciprocal() *
    scalar` in torch, two roundings where the rule has one."""
    import torch

    X, Y, Z = means[:, 0], means[:, 1], means[:, 2]
    nu = torch.zeros_like(X)
    for c in table.cpu().tolist():
        x = ((c[0] * X + c[1] * Y) + c[2] * Z) + c[3]
        y = ((c[4] * X + c[5] * Y) + c[6] * Z) + c[7]
        z = ((c[8] * X + c[9] * Y) + c[10] * Z) + c[11]
        fx, fy, cx, cy, W, H = c[12:18]
        u, w = (x / z) * fx + cx, (y / z) * fy + cy
        mw, mh = float(np.float32(margin) * np.float32(W)), float(np.float32(margin) * np.float32(H))
        seen = (z > near) & (u >= -mw) & (u <= float(np.float32(W) + np.float32(mw))) & (w >= -mh) & \
            (w <= float(np.float32(H) + np.float32(mh)))
        rate = torch.tensor(fx, device=z.device) / z
        nu = torch.where(seen & (rate > nu), rate, nu)
    k = torch.tensor(float(np.float32(np.sqrt(np.float64(variance)))), device=nu.device)
    pos = nu > 0
    if not bool(pos.any()):
        return torch.zeros_like(nu)
    return k / torch.where(pos, nu, nu[pos].min())


def _scene(n, views, dev):
    import torch

    from gs_fused import filter_cameras
    from harness import scene as S
    from harness.train import orbit_cameras

    cams = orbit_cameras(views, 1920, 1080)
    sc = S.make_scene(n, cams[0], sh_degree=0, seed=42)
    return torch.from_numpy(sc["means3d"]).to(dev), filter_cameras(cams, dev)


def sampling(a):
    import torch

    from gs_fused import sampling_filter_3d

    dev = torch.device("cuda:0")
    rows = []
    for views in a.views:
        means, table = _scene(a.n, views, dev)
        out = torch.empty(a.n, device=dev)
        hip = _time(lambda: sampling_filter_3d(means, table, out=out), a.rounds)
        ops = _time(lambda: sampling_torch(means, table), max(a.rounds // 4, 3))
        same = bool(torch.equal(sampling_filter_3d(means, table), sampling_torch(means, table)))
        rows.append({"num_gaussians": a.n, "views": views, "hip_ms": hip, "torch_ops_ms": ops, "bit_equal": same,
                     "seen": round(float((out > 0).double().mean()), 4)})
        print(json.dumps(rows[-1]), flush=True)
    merge(a.out, "sampling", rows)


def activation(a):
    import torch

    from gs_fused import activate_gaussians, apply_filter_3d

    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    l = (torch.rand(a.n, 3, generator=g) * 6 - 7).to(dev).requires_grad_(True)
    q = torch.randn(a.n, 4, generator=g).to(dev).requires_grad_(True)
    o = torch.randn(a.n, 1, generator=g).to(dev).requires_grad_(True)
    means = torch.randn(a.n, 3, generator=g).to(dev)
    campos = torch.tensor([0.0, 0.0, 5.0], device=dev)
    filt = torch.exp(torch.rand(a.n, generator=g) * 4 - 7).to(dev)
    cots = [torch.randn(a.n, k, generator=g).to(dev) for k in (3, 4, 1)]

    def fused(filter_3d):
        kw = {} if filter_3d is None else {"filter_3d": filter_3d}
        return activate_gaussians(means, l, q, o, campos, **kw)[:3]

    def torch_ops():
        s, qq, oo = fused(None)
        s2, o2 = apply_filter_3d(s, oo, filt)
        return s2, qq, o2

    def both(fn):
        outs = fn()
        torch.autograd.grad(outs, (l, q, o), cots)

    rec = {"num_gaussians": a.n}
    for name, fn in (("unfiltered", lambda: fused(None)), ("filtered", lambda: fused(filt)), ("torch_ops", torch_ops)):
        with torch.no_grad():
            rec[name + "_fwd_ms"] = _time(fn, a.rounds)
        rec[name + "_fwd_bwd_ms"] = _time(lambda fn=fn: both(fn), a.rounds)
    merge(a.out, "activation", rec)


def train(a):
    import dataclasses

    import torch

    import bench
    from harness.train import train as run

    dev = torch.device("cuda:0")
    rows = []
    for on in (False, True):
        # a quarter of the resolution at every step (the schedule never advances); `evaluate` renders full size
        cfg = dataclasses.replace(bench.config3(iters=a.iters), num_downscales=2, resolution_schedule=a.iters + 1,
                                  rasterize_mode="antialiased", filter_3d=on)
        res = run(cfg, dev)
        rows.append({"filter_3d": on, "iters": a.iters, "seed": cfg.seed, "train_resolution": "480x270",
                     "eval_resolution": "1920x1080", "psnr_start": round(res["psnr_start"], 3),
                     "psnr_end": round(res["psnr_end"], 3), "iters_per_s": round(res["iters_per_s"], 1),
                     "num_gaussians_end": res["num_gaussians_end"],
                     "filter_updates": (res.get("filter_3d") or {}).get("updates")})
        print(json.dumps(rows[-1]), flush=True)
    merge(a.out, "train_config3_quarter_resolution", rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter3d_bench.json"))
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("sampling")
    s.add_argument("--n", type=int, default=1_000_000)
    s.add_argument("--views", type=int, nargs="+", default=[48, 300])
    s.add_argument("--rounds", type=int, default=20)
    k = sub.add_parser("activation")
    k.add_argument("--n", type=int, default=1_000_000)
    k.add_argument("--rounds", type=int, default=20)
    t = sub.add_parser("train")
    t.add_argument("--iters", type=int, default=7000)
    a = ap.parse_args()
    {"sampling": sampling, "activation": activation, "train": train}[a.cmd](a)


if __name__ == "__main__":
    main()
