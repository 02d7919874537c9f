"""The oriented crop box on a viewer frame (forward only, `gs_fused.render_gaussians` under `torch.no_grad()`): three
ways to one view, timed with HIP events per frame (warm-up, then the median and the 10th / 90th percentile).

    python tools/crop_bench.py [--gaussians N] [--width W] [--height H] [--frames K] [--warmup K]

  (i)   uncropped: the view of all N Gaussians
  (ii)  gather: `index_select` of the six parameter tensors with a READY index of the kept rows, then the view on the
        subset -- what a caller can do without `crop=` (the toolkit's `get_outputs`, vanilla_gs.py:703-757).  Forming
        the index (the mask, `nonzero` and its read-back) is NOT in the timed region: the figure flatters this route
  (iii) `crop=`: the test inside the projection kernel, N unchanged

The events bracket whole frames as a caller issues them: the figures include the host-side launch path ((ii) makes six
more launches from Python per frame than (iii)), not GPU time alone.

The box is axis-aligned around the scene's median and keeps the middle half of the means along x and along y: a quarter
if the two were independent, 30 % on this scene (the means fill a frustum: x and y spread with the depth).  Prints one
JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-splatting-toolkit_amd")]
import numpy as np
import torch

from harness import scene as S
from harness.pipeline import CameraTensors


def timed(fn, frames, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(frames + 1)]
    ev[0].record()
    for k in range(frames):
        fn()
        ev[k + 1].record()
    torch.cuda.synchronize()
    ms = np.array([ev[k].elapsed_time(ev[k + 1]) for k in range(frames)])
    return {"ms_median": round(float(np.median(ms)), 4),
            "ms_p10_p90": [round(float(np.percentile(ms, 10)), 4), round(float(np.percentile(ms, 90)), 4)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    from gs_fused import CropBox, ViewSpec, render_gaussians

    dev = torch.device("cuda:0")
    cam = S.make_camera(a.width, a.height)
    sc = S.make_scene(a.gaussians, cam, sh_degree=a.sh_degree, seed=42, scale_lo=0.0025, scale_hi=0.025)
    p = {k: torch.from_numpy(v).to(dev) for k, v in sc.items()}
    raw = {"means": p["means3d"], "scales": p["scales"].log(), "quats": p["quats"],
           "opacities": torch.logit(p["opacities"]), "features_dc": p["sh_coeffs"][:, 0, :].contiguous(),
           "features_rest": p["sh_coeffs"][:, 1:, :].contiguous()}
    names = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")
    c = CameraTensors.from_numpy(cam, dev)
    bg = torch.tensor(S.BACKGROUND, device=dev)
    spec = ViewSpec(a.height, a.width, c.fx, c.fy, c.cx, c.cy, a.sh_degree)

    m = sc["means3d"].astype(np.float64)
    lo, hi = np.percentile(m, [25.0, 75.0], axis=0)
    lo[2], hi[2] = m[:, 2].min() - 1.0, m[:, 2].max() + 1.0
    box = CropBox(np.eye(3), (lo + hi) / 2, hi - lo)
    crop = box.tensor(dev)
    index = torch.nonzero(box.within(raw["means"])).reshape(-1)
    kept = int(index.numel())

    def view(q, capacity, crop=None):
        return render_gaussians(q["means"], q["scales"], q["quats"], q["opacities"], q["features_dc"], q["features_rest"],
                                c.viewmat, c.projmat, c.campos, bg, spec, capacity, crop=crop)

    with torch.no_grad():
        full = int(view(raw, 1 << 24)["count"].item())
        cropped = int(view(raw, 1 << 24, crop)["count"].item())
        cap_full = ((int(1.3 * full) + (1 << 20)) >> 20) << 20
        cap_crop = ((int(1.3 * cropped) + (1 << 20)) >> 20) << 20

        def gather():
            return view({k: raw[k].index_select(0, index) for k in names}, cap_crop)

        a_img, b_img = view(raw, cap_crop, crop)["rgb"], gather()["rgb"]
        same = float((a_img - b_img).abs().max())
        res = {"uncropped": timed(lambda: view(raw, cap_full), a.frames, a.warmup),
               "gather_then_view": timed(gather, a.frames, a.warmup),
               "crop": timed(lambda: view(raw, cap_crop, crop), a.frames, a.warmup)}
    print(json.dumps({"metric": "forward-only view, ms per frame (gs_fused.render_gaussians, no_grad)",
                      "gaussians": a.gaussians, "kept": kept, "resolution": f"{a.width}x{a.height}",
                      "list_entries": {"uncropped": full, "cropped": cropped},
                      "crop_vs_gather_max_abs_diff": same, "frames": a.frames, "warmup": a.warmup, **res}))


if __name__ == "__main__":
    main()
