"""The toolkit's `gaussians.ply` from a checkpoint, optionally cut to an oriented crop box.

    python tools/export_gaussians.py CHECKPOINT OUT.ply
        [--obb-pos X Y Z --obb-rpy R P Y --obb-scale SX SY SZ] [--no-bake-filter] [--device cuda:0]

CHECKPOINT is a `step-*.ckpt` file in the toolkit's layout (harness/checkpoint.py) or a directory of them (the latest
step is taken).  The six raw parameter tensors are written with gs_io.write_gaussian_ply, the file
`ExportGaussianSplat` writes (gs_toolkit/scripts/exporter.py).  With --obb-* (all three, or none: the viewer's crop
box, `OrientedBox.from_params`) only the Gaussians whose centre lies inside the box are written, in their order:
gs_fused.crop_gaussians -- the mask and the count come from the kernel the cropped projection shares its rule with
(--device cpu: the same float32 arithmetic on the host).  A checkpoint trained with the 3D smoothing filter
(`TrainConfig.filter_3d`) holds the filter next to the parameters: the file then gets the BAKED
log-scales and opacity logits (gs_fused.bake_filter_3d) -- rendered by any viewer, without a filter, it is the filtered
model -- unless --no-bake-filter asks for the raw parameters.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-splatting-toolkit_amd"), os.path.join(ROOT, "tools")]
import torch

from export_tsdf import add_obb_arguments, obb_from_args
from gs_fused.crop import crop_gaussians
from gs_io import write_gaussian_ply
from harness.checkpoint import _FILTER_KEY, PARAM_NAMES, latest_checkpoint

_PREFIXES = ("_model.gauss_params.", "gauss_params.", "")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("checkpoint")
    ap.add_argument("out")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--trust-pickle", action="store_true",
                    help="load a checkpoint that holds more than tensors, dicts, numbers and strings")
    ap.add_argument("--no-bake-filter", action="store_true",
                    help="write the raw parameters of a checkpoint that holds a 3D smoothing filter")
    add_obb_arguments(ap)
    a = ap.parse_args(argv)
    a.crop_box = obb_from_args(ap, a)
    return a


def _checkpoint_state(path: str, trust_pickle: bool):
    if os.path.isdir(path):
        path = latest_checkpoint(path)
    loaded = torch.load(path, map_location="cpu", weights_only=not trust_pickle)
    return loaded["pipeline"] if isinstance(loaded, dict) and "pipeline" in loaded else loaded


def checkpoint_filter_3d(path: str, trust_pickle: bool = False):
    """-> the 3D smoothing filter float32 [N] a checkpoint holds (harness/checkpoint.py), or None."""
    saved = _checkpoint_state(path, trust_pickle).get(_FILTER_KEY)
    return None if saved is None else saved.detach().to(torch.float32).contiguous()


def checkpoint_parameters(path: str, trust_pickle: bool = False):
    """-> {name: tensor} of the six raw parameters, under any of the key prefixes `load_model_state` accepts."""
    state = _checkpoint_state(path, trust_pickle)
    out = {}
    for name in PARAM_NAMES:
        for prefix in _PREFIXES:
            if prefix + name in state:
                out[name] = state[prefix + name].detach().to(torch.float32).contiguous()
                break
        else:
            raise SystemExit(f"export_gaussians: the checkpoint has no parameter '{name}'")
    return out


def main(argv=None):
    a = parse_args(argv)
    params = checkpoint_parameters(a.checkpoint, a.trust_pickle)
    total = params["means"].shape[0]
    filter_3d = checkpoint_filter_3d(a.checkpoint, a.trust_pickle)
    baked = filter_3d is not None and not a.no_bake_filter
    if baked:
        from gs_fused import bake_filter_3d

        params["scales"], params["opacities"] = bake_filter_3d(params["scales"], params["opacities"], filter_3d)
    if a.crop_box is not None:
        params = crop_gaussians({k: v.to(a.device) for k, v in params.items()}, a.crop_box)
    write_gaussian_ply(a.out, {k: v.cpu().numpy() for k, v in params.items()})
    summary = {"gaussians": total, "written": int(params["means"].shape[0]), "out": a.out,
               "filter_3d": None if filter_3d is None else ("baked" if baked else "left out (raw parameters)")}
    if a.crop_box is not None:
        summary["crop_box"] = {"pos": list(a.obb_pos), "rpy": list(a.obb_rpy), "scale": list(a.obb_scale)}
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
