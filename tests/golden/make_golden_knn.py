#!/usr/bin/env python3
"""Generate tests/golden/knn.npz from the REFERENCE's own code for the model's initial scales.

Runs ONLY in the build container (it reads /root/reference and needs scikit-learn).  `gs_toolkit.models.vanilla_gs`
imports half of the toolkit, so it cannot be imported here; as in make_golden_depth_reg.py the pieces are lifted out
with `ast` AT GENERATION TIME and executed unmodified on torch CPU float32 tensors:
  * models/vanilla_gs.py, the method `k_nearest_sklearn` (lines 260-280);
  * `populate_modules`: the three assignments to `distances`, `avg_dist` and `scales` that follow the call
    (lines 137-140), run with the method's result as a local.
Nothing of the reference's source is stored: the committed .npz holds the clouds, the float32 distances the method
returned and the log-scales those lines made of them.

    python tests/golden/make_golden_knn.py
"""
import ast
import os
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF_MODEL = "/root/reference/gs_toolkit/models/vanilla_gs.py"


def _lift():
    src = open(REF_MODEL).read()
    tree = ast.parse(src)
    method = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "k_nearest_sklearn")
    populate = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "populate_modules")

    def targets(node):
        return {t.id for tgt in node.targets for t in ast.walk(tgt) if isinstance(t, ast.Name)}

    wanted = [n for n in populate.body if isinstance(n, ast.Assign) and targets(n) & {"distances", "avg_dist", "scales"}]
    assert len(wanted) == 4, [ast.get_source_segment(src, n) for n in wanted]  # the call and the three lines after it
    ns = {"torch": torch, "np": np}
    mod = ast.Module(body=[method], type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, REF_MODEL, "exec"), ns)
    scales = ast.Module(body=wanted, type_ignores=[])
    ast.fix_missing_locations(scales)
    return ns["k_nearest_sklearn"], compile(scales, REF_MODEL, "exec")


def clouds():
    g = np.random.default_rng(20241101)
    u = g.standard_normal((800, 3))
    shell = u / np.linalg.norm(u, axis=1, keepdims=True) * (1.0 + 0.004 * g.standard_normal((800, 1)))
    base = g.uniform(-1, 1, (150, 3))
    a = g.uniform(0, 1, (150, 3))
    b = g.uniform(0, 1e-3, (150, 3)) + np.array([[1000.0, 0, 0]])
    return [
        ("cube_1000", g.uniform(-1, 1, (1000, 3))),
        ("shell_800", shell),
        ("duplicates_400", base[g.integers(0, 150, 400)]),  # twins and triplets: zero distances, -inf log-scales
        ("clusters_300", np.concatenate([a, b])[g.permutation(300)]),
        ("tiny_5", g.uniform(-1, 1, (5, 3))),
    ]


def main():
    method, scale_lines = _lift()
    out = {"cases": np.array([c[0] for c in clouds()])}
    for name, p in clouds():
        p = np.ascontiguousarray(p, np.float32)
        self_ = types.SimpleNamespace()
        self_.k_nearest_sklearn = types.MethodType(method, self_)
        ns = {"torch": torch, "np": np, "self": self_, "means": torch.nn.Parameter(torch.from_numpy(p))}
        exec(scale_lines, ns)
        dist, _ = self_.k_nearest_sklearn(torch.from_numpy(p), 3)
        scales = ns["scales"].detach().numpy()
        assert dist.dtype == np.float32 and dist.shape == (len(p), 3) and scales.dtype == np.float32
        assert scales.shape == (len(p), 3) and np.array_equal(ns["distances"].numpy(), dist)
        out[name + "_points"], out[name + "_dist"], out[name + "_log_scales"] = p, dist, scales
        print(f"{name}: n={len(p)}, zero distances {(dist == 0).sum()}, -inf scales {np.isinf(scales[:, 0]).sum()}")
    path = os.path.join(HERE, "knn.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
