#!/usr/bin/env python3
"""Golden vectors for the projection on cameras off the family of make_golden.py (fy != fx, W != H, off-centre
principal point, glob_scale != 1, raw quaternions, and all of it at once): the reference's own pure-PyTorch
`_torch_impl.project_gaussians_forward` and torch.autograd on rows of the cases of tests/projection_cases.py.

Runs ONLY where the reference is checked out (the import shim of make_golden.py); the committed project.npz is data:
inputs, the reference's outputs and its autograd gradients.  Nothing of the reference's source is stored.

    python tests/golden/make_golden_project.py

What that torch code is comparable on (the quirks at the top of make_golden.py, and two more):
  * its near-plane cull is `z < clip` where the CUDA source's is `z <= clip`: no stored row has z within 1e-3 of the
    threshold;
  * its tile box ends at trunc((u + r) / bw) + 1 where the CUDA source's ends at trunc((u + r) / bw + 1): a Gaussian
    whose box ends up to one tile left of (above) the image counts as touching the first tile column (row) there, and
    is culled by the CUDA source.  No stored row has (u + r) / bw or (v + r) / bw in (-1, 0), 1e-3 around it included;
  * the CUDA backward ignores the derivative of the 1.3x fov clamp, autograd does not: the tests compare gradients on
    rows inside the guard band only (all rows are stored);
  * its `scale_rot_to_cov3d` takes the quaternion as a unit quaternion and does not renormalise, where the CUDA source
    renormalises and differentiates as if the result were the input: the torch code is handed q / |q| (float32, torch's
    own normalize), and `g_quats` is its gradient with respect to THAT unit quaternion.  `quats` holds the raw input;
  * it evaluates every row, behind the camera too, and zeroes the culled ones afterwards: gradient rows of culled
    Gaussians can be 0 * inf there.  They are stored as zeros (the CUDA source writes zeros where radii <= 0).

Rows: at most ROWS per case (far fewer than 1500: the file stays below g3.npz).  EVEN of them are evenly strided over the
case, so that every population of it (thirds of the guard band, quarters of the near plane) is kept in proportion;
the others are the rows on which float64 (projection_reference.forward_condition_fp64) says an fp32 evaluation loses
most, output by output: the tests take the reference's largest distance from float64 as the measure of what fp32
costs on a case, and an even sample of a few per cent would miss the rows that decide it.  Keys: `<case>__<array>`."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

from make_golden import _import_reference  # noqa: E402
import projection_cases as PC  # noqa: E402
import projection_reference as PR  # noqa: E402

ROWS, EVEN = 120, 60


def pick_rows(c, ok):
    """`ok`: the rows the torch code is comparable on."""
    rows = list(ok[np.linspace(0, len(ok) - 1, min(EVEN, len(ok))).round().astype(int)])
    cond = PR.forward_condition_fp64(c.means3d, c.scales, c.glob_scale, c.quats, c.viewmat, c.projmat, c.fx, c.fy,
                                     c.cx, c.cy, c.H, c.W)
    vis = PR.project_forward_fp64(c.means3d, c.scales, c.glob_scale, c.quats, c.viewmat, c.projmat, c.fx, c.fy, c.cx,
                                  c.cy, c.H, c.W, c.bw, c.clip)["visible"]
    ranked = [[i for i in np.argsort(-np.where(vis, k, -np.inf), kind="stable") if vis[i] and i in set(ok)]
              for k in cond.values()]
    for j in range(max(len(r) for r in ranked)):  # the worst row of each output, then the second worst of each, ...
        for r in ranked:
            if j < len(r) and len(rows) < ROWS and r[j] not in rows:
                rows.append(r[j])
    return np.sort(np.array(rows[:ROWS]))


def main():
    ti = _import_reference()
    out = {}
    for c in PC.cases():
        if not c.in_golden:
            continue
        tz = c.means3d.astype(np.float64) @ c.viewmat[2, :3].astype(np.float64) + float(c.viewmat[2, 3])
        hi = PR.project_forward_fp64(c.means3d, c.scales, c.glob_scale, c.quats, c.viewmat, c.projmat, c.fx, c.fy, c.cx,
                                     c.cy, c.H, c.W, c.bw, c.clip)["box_hi"]
        ok = np.nonzero((np.abs(tz - float(np.float32(c.clip))) > 1e-3)
                        & ~((hi > -1.001) & (hi < 0.001)).any(axis=1))[0]
        rows = pick_rows(c, ok)
        t = lambda a: torch.from_numpy(np.array(a))  # noqa: E731
        means, scales = t(c.means3d[rows]).requires_grad_(True), t(c.scales[rows]).requires_grad_(True)
        qn = torch.nn.functional.normalize(t(c.quats[rows]), dim=-1).requires_grad_(True)
        cov3d, _, xys, depths, radii, conics, comp, tiles, mask = ti.project_gaussians_forward(
            means, scales, c.glob_scale, qn, t(c.viewmat), t(c.projmat), (c.fx, c.fy, c.cx, c.cy), (c.W, c.H), c.bw,
            c.clip)
        gen = torch.Generator().manual_seed(1234)
        g_xys, g_conics = torch.randn(len(rows), 2, generator=gen), torch.randn(len(rows), 3, generator=gen)
        ((xys * g_xys).sum() + (conics * g_conics).sum()).backward()
        grads = {}
        for key, leaf in (("g_means3d", means), ("g_scales", scales), ("g_quats", qn)):
            assert torch.isfinite(leaf.grad[mask]).all(), (c.name, key)
            grads[key] = torch.where(mask[:, None], leaf.grad, torch.zeros_like(leaf.grad))
        a = lambda x, dt=None: x.detach().numpy().astype(dt) if dt else x.detach().numpy()  # noqa: E731
        rec = dict(rows=rows.astype(np.int32), means3d=c.means3d[rows], scales=c.scales[rows], quats=c.quats[rows],
                   viewmat=c.viewmat, projmat=c.projmat, intrinsics=np.array([c.fx, c.fy, c.cx, c.cy], np.float64),
                   img_size=np.array([c.W, c.H], np.int32), block_width=np.int32(c.bw),
                   glob_scale=np.float32(c.glob_scale), clip_thresh=np.float32(c.clip),
                   cov3d=a(cov3d), xys=a(xys), depths=a(depths), radii=a(radii, np.int32), conics=a(conics),
                   compensation=a(comp), num_tiles_hit=a(tiles, np.int32), mask=a(mask),
                   g_xys=a(g_xys), g_conics=a(g_conics), **{k: a(v) for k, v in grads.items()})
        out.update({f"{c.name}__{k}": v for k, v in rec.items()})
        print(f"{c.name}: {len(rows)} rows, {int(mask.sum())} visible")
    path = os.path.join(HERE, "project.npz")
    np.savez_compressed(path, **out)
    size, limit = os.path.getsize(path), os.path.getsize(os.path.join(HERE, "g3.npz"))
    print(f"project.npz: {size} bytes (g3.npz: {limit})")
    assert size < limit


if __name__ == "__main__":
    main()
