#!/usr/bin/env python3
"""Generate tests/golden/dataset_poses.npz from the REFERENCE's own dataparser helpers, on the CPU in float32.

Needs a checkout of the reference toolkit (its root as the first argument, or in GS_TOOLKIT_REFERENCE).
`gs_toolkit.cameras.camera_utils` imports jaxtyping, which is not importable here; as in make_golden_camera_opt.py the
pieces are lifted out with `ast` AT GENERATION TIME and executed unmodified:
  * cameras/camera_utils.py: `rotation_matrix`, `focus_of_attention` (named by the next, never reached) and
    `auto_orient_and_center_poses` (their annotations dropped: they name jaxtyping);
  * data/utils/dataparsers_utils.py: the four `get_train_eval_split_*` functions.
Nothing of the reference's source is stored: the committed .npz holds inputs and the values that code produced.

Pose sets: "orbit" (12 cameras around the origin, up near +z), "tilted" (the same turned so that the mean up vector
is far from +z, and moved off the origin), "single" (one frame).  Each through orientation "up" / "none" and centring
"poses" / "none".  Splits: fraction 0.9 and 0.5, interval 8 and 3, for several frame counts; filename; all.

    python tests/golden/make_golden_dataset.py /path/to/reference
"""
import ast
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _functions(path, names, ns):
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {n.name for n in body} == set(names)
    for fn in body:  # annotations name jaxtyping's Float: dropped, nothing else is touched
        fn.returns = None
        for a in fn.args.args:
            a.annotation = None
    mod = ast.Module(body=body, type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, path, "exec"), ns)
    return ns


def look_at(eye, target, up):
    """camera-to-world [4,4] in the dataset's convention: x right, y up, z backwards."""
    z = eye - target
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
    return m


def pose_sets():
    rng = np.random.default_rng(20250211)
    orbit = []
    for i in range(12):
        th = 2 * math.pi * i / 12
        eye = np.array([4 * math.cos(th), 4 * math.sin(th), 1.0 + 0.5 * math.sin(3 * th)]) + rng.normal(0, 0.05, 3)
        orbit.append(look_at(eye, rng.normal(0, 0.05, 3), np.array([0.0, 0.0, 1.0])))
    orbit = np.stack(orbit)
    a, b = 2.1, -0.7  # a fixed turn about x then y: the mean up vector ends far from +z
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Ry @ Rx, (3.0, -2.0, 5.0)
    tilted = T @ orbit
    return {"orbit": orbit.astype(np.float32), "tilted": tilted.astype(np.float32),
            "single": tilted[3:4].astype(np.float32)}


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["GS_TOOLKIT_REFERENCE"]
    cu = _functions(os.path.join(ref, "gs_toolkit/cameras/camera_utils.py"),
                    ("rotation_matrix", "focus_of_attention", "auto_orient_and_center_poses"),
                    {"torch": torch, "math": math})
    du = _functions(os.path.join(ref, "gs_toolkit/data/utils/dataparsers_utils.py"),
                    ("get_train_eval_split_fraction", "get_train_eval_split_filename", "get_train_eval_split_interval",
                     "get_train_eval_split_all"), {"np": np, "math": math, "os": os})
    out = {}
    for name, poses in pose_sets().items():
        out[f"poses_{name}"] = poses
        for method in ("up", "none"):
            for centre in ("poses", "none"):
                oriented, transform = cu["auto_orient_and_center_poses"](torch.from_numpy(poses.copy()), method=method,
                                                                         center_method=centre)
                out[f"oriented_{name}_{method}_{centre}"] = oriented.numpy()
                out[f"transform_{name}_{method}_{centre}"] = transform.numpy()
    for n in (1, 2, 9, 10, 12, 31, 100):
        names = [f"frame_{i:05d}.png" for i in range(n)]
        for frac in (0.9, 0.5):
            tr, ev = du["get_train_eval_split_fraction"](names, frac)
            out[f"fraction_{n}_{frac}_train"], out[f"fraction_{n}_{frac}_eval"] = np.asarray(tr), np.asarray(ev)
        for k in (8, 3):
            tr, ev = du["get_train_eval_split_interval"](names, k)
            out[f"interval_{n}_{k}_train"], out[f"interval_{n}_{k}_eval"] = np.asarray(tr), np.asarray(ev)
        tr, ev = du["get_train_eval_split_all"](names)
        out[f"all_{n}_train"], out[f"all_{n}_eval"] = np.asarray(tr), np.asarray(ev)
    names = ["a/train_0.png", "a/eval_0.png", "a/train_1.png", "b/train_2.png", "b/eval_1.png"]
    tr, ev = du["get_train_eval_split_filename"](names)
    out["filename_names"] = np.array(names)
    out["filename_train"], out["filename_eval"] = np.asarray(tr), np.asarray(ev)
    path = os.path.join(HERE, "dataset_poses.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays")


if __name__ == "__main__":
    main()
