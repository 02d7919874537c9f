"""CPU: the float64 restatement of the projection's VJP (tests/projection_reference.py: torch, autograd) -- the
high-precision reference the GPU stage tests (tests/test_gpu_heldout.py) hold csrc/project.hip's backward to on
ill-conditioned covariances.

It follows the oracle's rules (oracle/gsr_oracle.c, gsr_oracle_project_backward): the quaternion is differentiated as
the unit quaternion q / |q| (no projection onto the tangent space), the backward's EWA Jacobian has no fov clamp (so
only Gaussians inside the 1.3x guard band are comparable), and the compensation's cotangent is scaled by
0.5 / (compensation + 1e-6) with the compensation that was handed in.  Pinned here against the oracle on a
well-conditioned scene and against the goldens of the reference's own autograd."""
import os

import numpy as np
import pytest
import torch

from harness import scene as S
from oracle import oracle as O
from projection_reference import project_vjp_fp64, row_err, row_max  # noqa: F401  (re-exported: test_gpu_heldout.py)


def oracle_project_vjp(sc, cam, cov3d, radii, conics, comp, v_xy, v_depth, v_conic, v_comp):
    return O.project_gaussians_backward(len(radii), sc["means3d"], sc["scales"], 1.0, sc["quats"], cam.viewmat[:3],
                                        cam.projmat, cam.fx, cam.fy, cam.cx, cam.cy, cam.height, cam.width, cov3d,
                                        radii, conics, comp, v_xy, v_depth, v_conic, v_comp)[2:]


@pytest.mark.parametrize("cotangent", ["xy_conic", "depth", "compensation"])
def test_fp64_projection_vjp_equals_the_oracle_on_a_well_conditioned_scene(cotangent):
    n, W, H = 3000, 320, 208
    cam = S.make_camera(W, H, yaw=0.1, pitch=-0.05)
    sc = S.make_scene(n, cam, sh_degree=0, seed=3, scale_lo=0.02, scale_hi=0.06)
    rng = np.random.default_rng(4)
    # near-isotropic splats: every covariance well conditioned
    sc["scales"] = (sc["scales"][:, :1] * rng.uniform(0.7, 1.3, (n, 3))).astype(np.float32)
    cov3d, xys, depths, radii, conics, comp, tiles = O.project_gaussians_forward(
        n, sc["means3d"], sc["scales"], 1.0, sc["quats"], cam.viewmat[:3], cam.projmat, cam.fx, cam.fy, cam.cx,
        cam.cy, H, W, 16, 0.01)
    z = lambda *shape: np.zeros(shape, np.float32)  # noqa: E731
    r = lambda *shape: rng.standard_normal(shape).astype(np.float32)  # noqa: E731
    cot = {"xy_conic": (r(n, 2), z(n), r(n, 3), z(n)), "depth": (z(n, 2), r(n), z(n, 3), z(n)),
           "compensation": (z(n, 2), z(n), z(n, 3), r(n))}[cotangent]
    ref = project_vjp_fp64(sc["means3d"], sc["scales"], 1.0, sc["quats"], cam.viewmat[:3], cam.projmat, cam.fx, cam.fy,
                           cam.cx, cam.cy, H, W, comp, *cot)
    orc = oracle_project_vjp(sc, cam, cov3d, radii, conics, comp, *cot)
    rows = (radii > 0) & ref[3]
    if cotangent == "compensation":
        # (the compensation's VJP is ill-conditioned in fp32 where it nears 1 -- splats far larger than the blur:
        #  the oracle forms 1 - compensation^2)
        rows &= comp < 0.9
    assert rows.sum() > 0.3 * n and (comp[rows] > 0.1).all()
    for o, f, nm in zip(orc, ref[:3], ("v_mean3d", "v_scale", "v_quat")):
        e = row_err(o[rows], f[rows]) / np.maximum(row_max(f[rows]), 1e-12)
        print(f"{cotangent} {nm}: oracle vs fp64 per row {e.max():.2e}")
        assert e.max() < 1e-5, f"{nm}: {e.max():.3e}"


@pytest.mark.parametrize("name", ["g0", "g1a", "g1b", "g2", "g3"])
def test_fp64_projection_vjp_equals_the_goldens(golden_dir, name):
    """The goldens' g_means3d / g_scales / g_quats: the reference's fp32 autograd for the cotangents g_xys / g_conics
    (the same rule as tests/test_oracle_golden.py::test_project_backward, on the guard band's Gaussians)."""
    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    fx, fy, cx, cy = (float(v) for v in g["intrinsics"])
    W, H = (int(v) for v in g["img_size"])
    n = g["means3d"].shape[0]
    zeros = np.zeros(n, np.float32)
    ref = project_vjp_fp64(g["means3d"], g["scales"], float(g["glob_scale"]), g["quats"], g["viewmat"][:3],
                           g["projmat"], fx, fy, cx, cy, H, W, np.ones(n, np.float32), g["g_xys"], zeros, g["g_conics"],
                           zeros)
    rows = (g["radii"] > 0) & ref[3]
    assert rows.any()
    for mine, key in zip(ref[:3], ("g_means3d", "g_scales", "g_quats")):
        gold = g[key][rows].astype(np.float64)
        floor = 1e-3 * max(1.0, float(np.abs(gold).max()))
        e = np.abs(mine[rows] - gold) / np.maximum(np.abs(gold), floor)
        assert e.max() < 2e-3, f"{key}: {e.max():.3e}"
