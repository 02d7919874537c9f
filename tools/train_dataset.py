#!/usr/bin/env python3
"""Train on a dataset directory (a `transforms.json` with images and, optionally, masks, depth and a seed cloud).

    python tools/train_dataset.py DATA [--model gaussian-splatting|co-gs] [--iters 30000] [--output-dir outputs]
        [--eval-mode fraction|filename|interval|all] [--fused-render] [--use-graph] [--camera-optimizer SO3xR3]
        [--strategy default|mcmc [--cap-max 1000000]] [--bilateral-grid [--bilagrid-shape X Y L]]
        [--normal-consistency [--normal-lambda 0.05] [--normal-start 7000]]
        [--depth-distortion [--distortion-lambda 100] [--distortion-start 3000]]
        [--prune-at 16000,24000 [--prune-rule max_weight|weight_sum|dominant] [--prune-keep 0.6 | --prune-threshold T]]
        [--filter-3d [--filter-3d-every 100]] ...

`harness.train.train` with `TrainConfig.dataset`: the files are uploaded as integers into a
gs_fused.ImageCache and every step's target comes from one kernel.  Writes `OUTPUT_DIR/step-*.ckpt` (the toolkit's
checkpoint layout, harness/checkpoint.py; the last step always) and `OUTPUT_DIR/result.json`: the trainer's record,
with the held-out split's metrics under `dataset.heldout`.  Prints a one-line JSON summary.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-splatting-toolkit_amd")]

import torch  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("data")
    ap.add_argument("--model", default="gaussian-splatting", choices=["gaussian-splatting", "co-gs"])
    ap.add_argument("--iters", type=int, default=30000)
    ap.add_argument("--output-dir", default="outputs")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--num-downscales", type=int, default=2)
    ap.add_argument("--resolution-schedule", type=int, default=2000)
    ap.add_argument("--background-color", default="random", choices=["random", "fixed"])
    ap.add_argument("--no-densify", action="store_true")
    ap.add_argument("--strategy", default="default", choices=["default", "mcmc"],
                    help="densification: the reference's schedule, or MCMC relocation with growth to --cap-max")
    ap.add_argument("--cap-max", type=int, default=1_000_000, help="--strategy mcmc: the model never exceeds this")
    ap.add_argument("--fused-render", action="store_true")
    ap.add_argument("--use-graph", action="store_true")
    ap.add_argument("--camera-optimizer", default="off", choices=["off", "SO3xR3", "SE3"])
    ap.add_argument("--bilateral-grid", action="store_true",
                    help="per-view bilateral grids between the render and the loss (exposure, white balance); not with "
                         "--use-graph")
    ap.add_argument("--bilagrid-shape", type=int, nargs=3, default=[16, 16, 8], metavar=("X", "Y", "L"))
    ap.add_argument("--normal-consistency", action="store_true",
                    help="depth-normal consistency loss (a third compositing pass for the normal image); not with "
                         "--fused-render or --use-graph")
    ap.add_argument("--normal-lambda", type=float, default=0.05)
    ap.add_argument("--normal-start", type=int, default=7000, help="the term joins the loss after this iteration")
    ap.add_argument("--depth-distortion", action="store_true",
                    help="depth distortion loss (one more walk over the tile lists, forward and backward); not with "
                         "--fused-render or --use-graph")
    ap.add_argument("--distortion-lambda", type=float, default=100.0)
    ap.add_argument("--distortion-start", type=int, default=3000, help="the term joins the loss after this iteration")
    ap.add_argument("--prune-at", default="", help="comma-separated steps after which the model is pruned by its blend-"
                                                   "weight statistics over all training views (DESIGN.md 4.21)")
    ap.add_argument("--prune-rule", default="max_weight", choices=["max_weight", "weight_sum", "dominant"])
    ap.add_argument("--prune-keep", type=float, default=None, help="the fraction of the Gaussians that stays")
    ap.add_argument("--prune-threshold", type=float, default=None,
                    help="scores below it are removed (default: the rule's: max_weight 0.01, dominant 1)")
    ap.add_argument("--filter-3d", action="store_true",
                    help="Mip-Splatting's 3D smoothing filter from the training cameras' sampling rate (DESIGN.md 4.22); "
                         "not with --fused-render, --use-graph or --strategy mcmc")
    ap.add_argument("--filter-3d-every", type=int, default=100, help="steps between recomputations of the filter")
    ap.add_argument("--depth-loss-start-iteration", type=int, default=6000)
    ap.add_argument("--save-every", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--eval-mode", default="fraction", choices=["fraction", "filename", "interval", "all"])
    ap.add_argument("--train-split-fraction", type=float, default=0.9)
    ap.add_argument("--eval-interval", type=int, default=8)
    ap.add_argument("--orientation-method", default="up", choices=["up", "none"])
    ap.add_argument("--center-method", default="poses", choices=["poses", "none"])
    ap.add_argument("--auto-scale-poses", action="store_true")
    ap.add_argument("--scale-factor", type=float, default=1.0)
    ap.add_argument("--random-init", action="store_true")
    ap.add_argument("--num-random", type=int, default=50000)
    ap.add_argument("--random-scale", type=float, default=10.0)
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    import harness.train as HT

    device = torch.device(a.device)
    # the last step is always saved: the trainer saves at the multiples of `save_every`; where the last step is none
    # of them, only the last step is saved
    save_every = a.save_every if 0 < a.save_every < a.iters and (a.iters - 1) % a.save_every == 0 else max(a.iters - 1, 1)
    mcmc = None
    if a.strategy == "mcmc":
        from gs_fused import MCMCConfig

        mcmc = MCMCConfig(cap_max=a.cap_max)
    cfg = HT.TrainConfig(
        strategy=a.strategy, mcmc=mcmc,
        dataset=a.data, model=a.model, iters=a.iters, sh_degree=a.sh_degree, num_downscales=a.num_downscales,
        resolution_schedule=a.resolution_schedule, background_color=a.background_color, densify=not a.no_densify,
        fused_render=a.fused_render, use_graph=a.use_graph, camera_optimizer=a.camera_optimizer,
        bilateral_grid=a.bilateral_grid, bilagrid_shape=tuple(a.bilagrid_shape),
        normal_consistency=a.normal_consistency, normal_lambda=a.normal_lambda, normal_start_iteration=a.normal_start,
        depth_distortion=a.depth_distortion, distortion_lambda=a.distortion_lambda,
        distortion_start_iteration=a.distortion_start,
        prune_at=tuple(int(s) for s in a.prune_at.split(",") if s.strip()), prune_rule=a.prune_rule,
        prune_keep=a.prune_keep, prune_threshold=a.prune_threshold,
        filter_3d=a.filter_3d, filter_3d_every=a.filter_3d_every,
        depth_loss_start_iteration=a.depth_loss_start_iteration, checkpoint_dir=a.output_dir, save_every=save_every,
        seed=a.seed, means_lr_schedule=True, log_every=max(a.iters // 100, 1),
        dataset_eval_mode=a.eval_mode, dataset_train_split_fraction=a.train_split_fraction,
        dataset_eval_interval=a.eval_interval, dataset_orientation_method=a.orientation_method,
        dataset_center_method=a.center_method, dataset_auto_scale_poses=a.auto_scale_poses,
        dataset_scale_factor=a.scale_factor, dataset_random_init=a.random_init, dataset_num_random=a.num_random,
        dataset_random_scale=a.random_scale,
        dataset_allow_fisheye=True)  # (an OPENCV_FISHEYE dataset with zero distortion trains as camera_model="fisheye")
    os.makedirs(a.output_dir, exist_ok=True)
    res = HT.train(cfg, device)
    with open(os.path.join(a.output_dir, "result.json"), "w", encoding="utf-8") as f:
        json.dump(res, f, indent=1)
    held = res["dataset"]["heldout"] or {}
    print(json.dumps({"output_dir": a.output_dir, "iters": res["iters"], "iters_per_s": res["iters_per_s"],
                      "num_gaussians_end": res["num_gaussians_end"], "psnr_train_views": res["psnr_end"],
                      "psnr_heldout": held.get("psnr"), "ssim_heldout": held.get("ssim"),
                      "cache_bytes": res["dataset"]["cache_bytes"]}))
    return res


if __name__ == "__main__":
    main()
