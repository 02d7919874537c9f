"""The camera's gradient through the projection, in float64: `project_vjp_fp64`'s forward (tests/projection_reference.py)
with `viewmat[:3]` and `projmat` as the autograd leaves.  A restatement of the rules listed in that file's header --
no fov clamp in the backward, the compensation's cotangent scaled by 0.5 / (compensation + 1e-6) with the compensation
that was handed in, a cotangent that is None is zero -- not of csrc/project.hip.

Every Gaussian gets its OWN copy of the two matrices, so autograd returns the per-Gaussian terms; the gradient of an
entry is their sum over the Gaussians, and its MASS is the sum of their magnitudes: what a sum of float32 rows, each
held to a relative bound, can be held to.  Only the rows of `visible` (the forward's radii > 0) contribute."""
import numpy as np
import torch

from projection_reference import _f32


def project_pose_vjp_fp64(means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy, img_height, img_width,
                          compensation, visible, v_xy, v_depth, v_conic, v_compensation, cov3d=None):
    """-> dict of float64 numpy: v_viewmat [3,4], v_projmat [4,4], mass_viewmat [3,4], mass_projmat [4,4], and guard
    [n] (inside the 1.3x guard band: where the unclamped backward is the forward's derivative).  `cov3d` [n,6] in
    place of `scales` / `quats` (both None): handed in."""
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    fx, fy, cx, cy, glob_scale = (_f32(v) for v in (fx, fy, cx, cy, glob_scale))
    vis = np.asarray(visible, bool)
    n_all = len(vis)
    zeros = dict(v_viewmat=np.zeros((3, 4)), v_projmat=np.zeros((4, 4)), mass_viewmat=np.zeros((3, 4)),
                 mass_projmat=np.zeros((4, 4)), guard=np.zeros(n_all, bool))
    if not vis.any():
        return zeros
    pick = lambda a: None if a is None else d(np.asarray(a)[vis])  # noqa: E731
    m = pick(means3d)
    n = m.shape[0]
    vm = d(viewmat).reshape(-1, 4)[:3].expand(n, 3, 4).clone().requires_grad_(True)  # one copy per Gaussian
    pm = d(projmat).reshape(4, 4).expand(n, 4, 4).clone().requires_grad_(True)
    if cov3d is None:
        q = pick(quats)
        w, x, y, z = (q / q.norm(dim=-1, keepdim=True)).unbind(-1)
        R = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                         torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                         torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)
        M = R * (glob_scale * pick(scales))[:, None, :]
        S = M @ M.transpose(1, 2)
    else:
        assert scales is None and quats is None
        c6 = pick(cov3d)
        S = torch.stack([c6[:, [0, 1, 2]], c6[:, [1, 3, 4]], c6[:, [2, 4, 5]]], -2)
    hom = torch.cat([m, torch.ones(n, 1, dtype=torch.float64)], -1)
    t = (vm @ hom[:, :, None])[:, :, 0]
    tx, ty, tz = t.unbind(-1)
    zero = torch.zeros_like(tz)
    J = torch.stack([torch.stack([fx / tz, zero, -fx * tx / tz ** 2], -1),
                     torch.stack([zero, fy / tz, -fy * ty / tz ** 2], -1)], -2)
    T = J @ vm[:, :, :3]
    Cv = T @ S @ T.transpose(1, 2)
    a, b, c = Cv[:, 0, 0] + 0.3, Cv[:, 0, 1], Cv[:, 1, 1] + 0.3
    det = a * c - b * b
    conic = torch.stack([c / det, -b / det, a / det], -1)
    comp_sq = (Cv[:, 0, 0] * Cv[:, 1, 1] - Cv[:, 0, 1] ** 2) / det
    h = (pm @ hom[:, :, None])[:, :, 0]
    rw = 1.0 / (h[:, 3] + 1e-6)
    xy = torch.stack([0.5 * img_width * h[:, 0] * rw + cx - 0.5, 0.5 * img_height * h[:, 1] * rw + cy - 0.5], -1)
    loss = (vm * 0.0).sum() + (pm * 0.0).sum()
    if v_xy is not None:
        loss = loss + (xy * pick(v_xy)).sum()
    if v_depth is not None:
        loss = loss + (tz * pick(v_depth)).sum()
    if v_conic is not None:
        loss = loss + (conic * pick(v_conic)).sum()
    if v_compensation is not None:
        loss = loss + (comp_sq * (pick(v_compensation) * 0.5 / (pick(compensation) + 1e-6))).sum()
    gv, gp = torch.autograd.grad(loss, (vm, pm))
    with torch.no_grad():
        limx, limy = 1.3 * 0.5 * img_width / fx, 1.3 * 0.5 * img_height / fy
        guard = np.zeros(n_all, bool)
        guard[vis] = (((tx / tz).abs() < limx) & ((ty / tz).abs() < limy)).numpy()
    return dict(v_viewmat=gv.sum(0).numpy(), v_projmat=gp.sum(0).numpy(), mass_viewmat=gv.abs().sum(0).numpy(),
                mass_projmat=gp.abs().sum(0).numpy(), guard=guard)


def mass_ratio(mine, ref, mass):
    """max over the entries of |mine - ref| / mass; an entry of zero mass must be exactly zero (ratio 0, else inf)."""
    err = np.abs(np.asarray(mine, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(mass > 0, err / mass, np.where(err == 0, 0.0, np.inf))
    return float(r.max())
