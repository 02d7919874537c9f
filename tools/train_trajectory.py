#!/usr/bin/env python3
"""The trainer's trajectory on a list of small cases, to the bit: one JSON line per case with the whole result of
`harness.train.train` (floats as `float.hex`, the timing keys left out).  Two checkouts that print the same bytes
compute the same thing.  On the CPU the native ops are the oracle-backed stand-ins of tests/cpu_standins.py (the
trainer is deterministic there); `--device cuda` runs the real ops under `rasterize.set_deterministic(True)`.

    python tools/train_trajectory.py [--device cuda] [--world 2 [--sharded]] [case ...]
"""
import argparse
import json
import os
import socket
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-splatting-toolkit_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

BASE = dict(num_gaussians=600, init_gaussians=200, width=64, height=48, num_views=4, eval_views=2, sh_degree=1,
            sh_degree_interval=10, scene_scale=(0.03, 0.15), log_every=1)
REFINE = dict(warmup_length=9, refine_every=10, reset_alpha_every=3, stop_screen_size_at=30, stop_split_at=55,
              densify_grad_thresh=2e-5, cull_alpha_thresh=0.05)  # refines at steps 20 / 50 / 60
COGS = dict(iters=12, model="co-gs", depth_loss_start_iteration=1)
CASES = {
    "refine": dict(iters=62, densify=True),
    "schedule_mask": dict(iters=24, background_color="random", num_downscales=1, resolution_schedule=8, mask="box"),
    "cogs_mask": dict(COGS, mask="alpha", depth_loss_start_iteration=3, background_color="random"),
    "cogs_terms": dict(COGS, use_est_depth=True, use_scaled_est_depth=True, using_tv_loss=True,
                       use_scale_regularization=True),  # (use_sparse_loss: nan from step 0, as in the source)
    "cogs_terms_mask": dict(COGS, use_est_depth=True, use_scaled_est_depth=True, using_tv_loss=True, mask="box"),
    "per_step_target": dict(iters=24, background_color="random", num_downscales=1, resolution_schedule=8,
                            fused_target=False),
    "means_lr": dict(iters=32, densify=True, means_lr_schedule=True),
    "sfm": dict(iters=12, init="sfm", init_gaussians=150),
    "caller_syncs": dict(iters=12, caller_syncs=True),
    "torch_adam": dict(iters=12, fused_adam=False, fused_loss=False),
    "resume": dict(iters=45, densify=True, save_every=30),  # ... and a second run resumed from the step-30 file
    # the shape of test_deterministic_mode_makes_training_bitwise_reproducible (--device cuda)
    "gpu": dict(num_gaussians=20_000, init_gaussians=4_000, width=320, height=180, num_views=8, iters=150, sh_degree=3,
                sh_degree_interval=40, densify=True, scene_scale=(0.01, 0.06), log_every=0),
    # strategy="mcmc" (--device cuda only: relocation, noise and regularisers are HIP kernels): 2 000 -> cap 3 000
    "gpu_mcmc": dict(num_gaussians=6000, init_gaussians=2000, width=160, height=90, num_views=4, iters=300, sh_degree=3,
                     sh_degree_interval=60, strategy="mcmc", scene_scale=(0.01, 0.06), log_every=0),
}
MCMC = dict(cap_max=3000, refine_start_iter=20, refine_every=20)
GPU_ONLY = ("gpu", "gpu_mcmc")
GPU_REFINE = dict(warmup_length=40, refine_every=20, reset_alpha_every=6, stop_screen_size_at=200, stop_split_at=260)
TIMING = ("seconds", "iters_per_s", "views_per_s", "peak_memory_bytes")


def _hex(x):
    if isinstance(x, float):
        return x.hex()
    if isinstance(x, dict):
        return {k: _hex(v) for k, v in x.items()}
    return [_hex(v) for v in x] if isinstance(x, (list, tuple)) else x


def _run(rank, world, port, q, name, device, sharded, ckpt):
    import torch.distributed as dist

    import harness.train as HT
    from gs_fused import RefineConfig

    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
    if device == "cpu":  # wired as tests/test_dp_train_gloo.py::_run wires them
        import cpu_standins as SI
        import harness.pipeline as HP
        from oracle import oracle as O

        torch.set_num_threads(2)
        O.set_threads(2)
        HP.project_gaussians, HP.spherical_harmonics, HP.rasterize_gaussians = (
            SI.project_gaussians, SI.spherical_harmonics, SI.rasterize_gaussians)
        HT._refine = lambda params, moments, stats, rcfg, step, ntd, max_dim, seed: SI.refine_gaussians(
            params, moments, stats, rcfg, step, ntd, max_dim, seed=seed)
    else:
        from rasterizer import rasterize as R

        R.set_deterministic(True)
    kw = dict(BASE, **CASES[name])
    runs = [kw] if name != "resume" else [dict(kw, checkpoint_dir=ckpt), dict(kw, save_every=0, resume_from=ckpt)]
    for kw in runs:
        rcfg = RefineConfig(**(GPU_REFINE if name == "gpu" else REFINE)) if kw.get("densify") else None
        if kw.get("strategy") == "mcmc":
            from gs_fused import MCMCConfig

            kw = dict(kw, mcmc=MCMCConfig(**MCMC))
        res = HT.train(HT.TrainConfig(refine=rcfg, sharded_adam=sharded, **kw),
                       torch.device(device, 0) if device == "cuda" else torch.device(device), rank, world)
        q.put((rank, {k: _hex(v) for k, v in res.items() if k not in TIMING and not k.startswith("phase_")}))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", help=f"default: every CPU case; known: {', '.join(CASES)}")
    ap.add_argument("--device", default="cpu", choices=["cpu", "cuda"])
    ap.add_argument("--world", type=int, default=1, help="ranks over gloo, spawned as tests/test_dp_train_gloo.py spawns")
    ap.add_argument("--sharded", action="store_true", help="TrainConfig.sharded_adam")
    args = ap.parse_args()
    ctx = mp.get_context("spawn")
    for name in args.cases or [c for c in CASES if c not in GPU_ONLY]:
        with tempfile.TemporaryDirectory() as ckpt:
            with socket.socket() as s:
                s.bind(("127.0.0.1", 0))
                port = s.getsockname()[1]
            q = ctx.Queue()
            procs = [ctx.Process(target=_run, args=(r, args.world, port, q, name, args.device, args.sharded, ckpt))
                     for r in range(args.world)]
            for p in procs:
                p.start()
            n_runs = 2 if name == "resume" else 1
            got = sorted((q.get(timeout=900) for _ in range(args.world * n_runs)), key=lambda x: x[0])
            for p in procs:
                p.join(timeout=120)
                assert p.exitcode == 0, (name, p.exitcode)
        for rank, res in got:
            print(json.dumps({"case": name, "world": args.world, "sharded": args.sharded, "rank": rank, **res}),
                  flush=True)


if __name__ == "__main__":
    main()
