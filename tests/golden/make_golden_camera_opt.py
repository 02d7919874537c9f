#!/usr/bin/env python3
"""Generate tests/golden/camera_opt_maps.npz from the REFERENCE's own pose code, on the CPU in float32.

Runs ONLY in the build container (it reads /root/reference).  `gs_toolkit.cameras.lie_groups` imports jaxtyping and
`gs_toolkit.cameras.camera_optimizers` half of the toolkit, neither importable here; as in make_golden_cogs.py the
pieces are lifted out with `ast` AT GENERATION TIME and executed unmodified on torch CPU tensors:
  * cameras/lie_groups.py: `exp_map_SO3xR3` and `exp_map_SE3` (their annotations dropped: they name jaxtyping);
  * cameras/camera_optimizers.py: the bodies of `CameraOptimizer.get_loss_dict` and `get_metrics_dict`, run with a
    bare `self` carrying `pose_adjustment` and the config's default penalties (1e-2, 1e-3).
Nothing of the reference's source is stored: the committed .npz holds inputs and the values that code produced.

Inputs: zero; angles on either side of both thresholds (squared angle 1e-4 of SO3xR3, theta = 1e-2 of SE3); large
angles near pi; a random batch.

    python tests/golden/make_golden_camera_opt.py
"""
import ast
import math
import os
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF_LIE = "/root/reference/gs_toolkit/cameras/lie_groups.py"
REF_OPT = "/root/reference/gs_toolkit/cameras/camera_optimizers.py"


def _functions(path, names):
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {n.name for n in body} == set(names)
    for fn in body:  # annotations name jaxtyping's Float: dropped, nothing else is touched
        fn.returns = None
        for a in fn.args.args:
            a.annotation = None
    mod = ast.Module(body=body, type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"torch": torch}
    exec(compile(mod, path, "exec"), ns)
    return ns


def _methods(path, cls, names):
    tree = ast.parse(open(path).read())
    klass = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls)
    body = [n for n in klass.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {n.name for n in body} == set(names)
    for fn in body:
        fn.returns = None
        for a in fn.args.args:
            a.annotation = None
    mod = ast.Module(body=body, type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"torch": torch}
    exec(compile(mod, path, "exec"), ns)
    return ns


def inputs():
    rng = np.random.default_rng(20241019)
    unit = lambda v: v / np.linalg.norm(v)  # noqa: E731
    rows = [np.zeros(6)]
    # either side of SO3xR3's clamp (|w|^2 = 1e-4, |w| = 1e-2) and of SE3's series switch (theta = 1e-2)
    for theta in (1e-4, 3e-3, 0.999e-2, 0.99999e-2, 1.00001e-2, 1.001e-2, 3e-2):
        rows.append(np.concatenate([rng.uniform(-0.5, 0.5, 3), theta * unit(rng.standard_normal(3))]))
    for theta in (math.pi - 1e-3, math.pi - 0.05, 3.0, 2.0):  # large angles near pi
        rows.append(np.concatenate([rng.uniform(-2, 2, 3), theta * unit(rng.standard_normal(3))]))
    rows.append(np.concatenate([np.zeros(3), 0.3 * unit(rng.standard_normal(3))]))  # rotation only
    rows.append(np.concatenate([rng.uniform(-1, 1, 3), np.zeros(3)]))               # translation only
    batch = np.concatenate([rng.uniform(-1, 1, (16, 3)), rng.standard_normal((16, 3)) * 0.4], axis=1)
    return np.concatenate([np.stack(rows), batch]).astype(np.float32)


def main():
    lie = _functions(REF_LIE, ("exp_map_SO3xR3", "exp_map_SE3"))
    opt = _methods(REF_OPT, "CameraOptimizer", ("get_loss_dict", "get_metrics_dict"))
    x = torch.from_numpy(inputs())
    out = {"tangent": x.numpy(), "so3xr3": lie["exp_map_SO3xR3"](x).numpy(), "se3": lie["exp_map_SE3"](x).numpy()}
    # one at a time too: a batch of one must give the same rows (recorded, not assumed)
    out["so3xr3_single"] = torch.cat([lie["exp_map_SO3xR3"](x[i:i + 1]) for i in range(len(x))]).numpy()
    out["se3_single"] = torch.cat([lie["exp_map_SE3"](x[i:i + 1]) for i in range(len(x))]).numpy()
    config = types.SimpleNamespace(mode="SO3xR3", trans_l2_penalty=1e-2, rot_l2_penalty=1e-3)
    regs, trans, rots = [], [], []
    sets = [x, x[:1], x[1:8], x[-16:]]
    for k, p in enumerate(sets):
        self = types.SimpleNamespace(config=config, pose_adjustment=p)
        loss, metrics = {}, {}
        opt["get_loss_dict"](self, loss)
        opt["get_metrics_dict"](self, metrics)
        regs.append(float(loss["camera_opt_regularizer"]))
        trans.append(float(metrics["camera_opt_translation"]))
        rots.append(float(metrics["camera_opt_rotation"]))
        out[f"reg_input_{k}"] = p.numpy()
    out["regulariser"] = np.array(regs, np.float32)
    out["metric_translation"] = np.array(trans, np.float32)
    out["metric_rotation"] = np.array(rots, np.float32)
    path = os.path.join(HERE, "camera_opt_maps.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
