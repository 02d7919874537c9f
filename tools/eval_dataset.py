#!/usr/bin/env python3
"""Held-out evaluation of a checkpoint on a dataset directory, written as the toolkit's `gs-eval` writes it.

    python tools/eval_dataset.py DATA CHECKPOINT --output output.json [--split val] [--model gaussian-splatting]

CHECKPOINT is a `step-*.ckpt` file in the toolkit's layout or a directory of them (the latest step).  Every view of the
split is rendered at full size (with the 3D smoothing filter the checkpoint holds, if any) and measured by `harness.train.evaluate_dataset` (PSNR, SSIM, rays per second and frames
per second, with their standard deviations; LPIPS is not computed: no network weights ship with this package).  The
output file has the four top-level keys of gs_toolkit/scripts/eval.py:39-44: `experiment_name`, `method_name`,
`checkpoint`, `results`.  The dataparser options must be the ones the model was trained with.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-splatting-toolkit_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("data")
    ap.add_argument("checkpoint")
    ap.add_argument("--output", required=True, help="a .json file")
    ap.add_argument("--split", default="val", choices=["train", "val", "test"])
    ap.add_argument("--model", default="gaussian-splatting", choices=["gaussian-splatting", "co-gs"])
    ap.add_argument("--rasterize-mode", default="classic", choices=["classic", "antialiased"])
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--eval-mode", default="fraction", choices=["fraction", "filename", "interval", "all"])
    ap.add_argument("--train-split-fraction", type=float, default=0.9)
    ap.add_argument("--eval-interval", type=int, default=8)
    ap.add_argument("--orientation-method", default="up", choices=["up", "none"])
    ap.add_argument("--center-method", default="poses", choices=["poses", "none"])
    ap.add_argument("--auto-scale-poses", action="store_true")
    ap.add_argument("--scale-factor", type=float, default=1.0)
    ap.add_argument("--trust-pickle", action="store_true")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    if not a.output.endswith(".json"):
        raise SystemExit("eval_dataset: --output must be a .json file")
    import harness.train as HT
    from export_gaussians import checkpoint_filter_3d, checkpoint_parameters
    from harness.checkpoint import latest_checkpoint

    device = torch.device(a.device)
    path = latest_checkpoint(a.checkpoint) if os.path.isdir(a.checkpoint) else a.checkpoint
    params = checkpoint_parameters(path, a.trust_pickle)
    bands = params["features_rest"].shape[1] + 1
    sh_degree = {1: 0, 4: 1, 9: 2, 16: 3, 25: 4}[bands]
    model = HT.GaussianParams({k: v.numpy() for k, v in params.items()}, device)
    filter_3d = checkpoint_filter_3d(path, a.trust_pickle)
    if filter_3d is not None:  # trained with TrainConfig.filter_3d: evaluated as trained
        model.filter_3d = filter_3d.to(device)
    cfg = HT.TrainConfig(dataset=a.data, model=a.model, sh_degree=sh_degree, rasterize_mode=a.rasterize_mode,
                         dataset_eval_mode=a.eval_mode, dataset_train_split_fraction=a.train_split_fraction,
                         dataset_eval_interval=a.eval_interval, dataset_orientation_method=a.orientation_method,
                         dataset_center_method=a.center_method, dataset_auto_scale_poses=a.auto_scale_poses,
                         dataset_scale_factor=a.scale_factor, dataset_allow_fisheye=True)
    results = HT.evaluate_dataset(model, a.data, cfg, a.split, device)
    info = {"experiment_name": os.path.basename(os.path.normpath(os.path.dirname(a.data) if a.data.endswith(".json")
                                                                  else a.data)),
            "method_name": a.model, "checkpoint": str(path), "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
    with open(a.output, "w", encoding="utf8") as f:
        f.write(json.dumps(info, indent=2))
    print(json.dumps({"output": a.output, "psnr": results["psnr"], "ssim": results["ssim"],
                      "num_images": results["num_images"]}))
    return info


if __name__ == "__main__":
    main()
