"""GPU: `gs_fusion.fuse_views(masks=...)` -- a view's depth is fused only where its object mask keeps it -- against the
same loop written out with `valid` multiplied by the NumPy restatement of the mask (tests/export_mask_reference.py).
Scene: 6000 flat opaque Gaussians on the radius-0.5 sphere of tests/tsdf_reference.py, two of its cameras."""
import math

import numpy as np
import pytest
import torch

import export_mask_reference as M
import tsdf_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _sphere_params(n=6000, seed=3):
    from harness.scene import SH_C0

    rng = np.random.default_rng(seed)
    nrm = rng.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = nrm[nrm[:, 2] > -0.999]
    n = len(nrm)
    q = np.concatenate([1.0 + nrm[:, 2:3], -nrm[:, 1:2], nrm[:, 0:1], np.zeros((n, 1))], 1)  # z axis -> normal
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)  # noqa: E731
    return {"means3d": t(R.SPHERE_RADIUS * nrm), "scales": t(np.tile([0.03, 0.03, 0.002], (n, 1))), "quats": t(q),
            "opacities": t(np.full((n, 1), 0.9975)), "sh_coeffs": t((0.5 * nrm / SH_C0)[:, None, :])}


def _cameras():
    from harness.scene import Camera, projection_matrix

    fx, fy, cx, cy = R.sphere_intrinsics()
    S = R.SPHERE_SIZE
    P = projection_matrix(0.001, 1000.0, 2 * math.atan(S / (2 * fx)), 2 * math.atan(S / (2 * fy)))
    return [Camera(S, S, fx, fy, cx, cy, V.astype(np.float32), (P @ V).astype(np.float32))
            for V in (R.sphere_cameras()[0], R.sphere_cameras()[6])]


def _masks():
    """Two annotation images [H,W,3] uint8: a blob over part of the sphere's silhouette with values around the
    gray thresholds at its rim, and a small rectangle."""
    S = R.SPHERE_SIZE
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:S, 0:S]
    a = np.zeros((S, S, 3), np.uint8)
    blob = (yy - 70) ** 2 + (xx - 95) ** 2 < 38 ** 2
    a[blob] = rng.integers(0, 16, (int(blob.sum()), 3), dtype=np.uint8)
    core = (yy - 70) ** 2 + (xx - 95) ** 2 < 25 ** 2
    a[core] = (0, 255, 0)
    b = np.zeros((S, S, 3), np.uint8)
    b[60:100, 50:90] = (255, 255, 255)
    return [a, b]


@pytest.mark.parametrize("bounding_box", [False, True])
def test_masked_fusion_equals_valid_times_reference_mask(bounding_box):
    from gs_fusion import TSDFVolume, fuse_views, view_depth
    from harness.pipeline import CameraTensors, render_view

    params, cams, masks = _sphere_params(), _cameras(), _masks()
    bg = torch.zeros(3, device=DEV)
    args = R.sphere_volume_args()
    plain, masked, by_hand = (TSDFVolume(device=DEV, **args) for _ in range(3))
    fuse_views(plain, params, cams, bg, 0)
    fuse_views(masked, params, cams, bg, 0, masks=masks, bounding_box=bounding_box)
    with torch.no_grad():
        for cam, mask in zip(cams, masks):
            out = render_view(params["means3d"], params["scales"], params["quats"], params["opacities"],
                              params["sh_coeffs"], CameraTensors.from_numpy(cam, DEV), bg, 0, render_depth=True,
                              fused_depth=True, normalise_depth=False)
            depth, valid = view_depth(out["depth_acc"], out["alpha"], 0.5)
            keep = torch.from_numpy(M.export_mask(mask, bounding_box).astype(np.uint8)).to(DEV)
            assert 500 < int((valid * keep).sum()) < int(valid.sum())
            by_hand.integrate(depth, out["rgb"].contiguous(), cam.fx, cam.fy, cam.cx, cam.cy, cam.viewmat,
                              valid=valid * keep, depth_trunc=10.0)
    a, b = masked.state_dict(), by_hand.state_dict()
    assert a["num_allocated"] == b["num_allocated"] > 10
    for k in ("table", "tsdf", "weight", "color"):
        assert torch.equal(a[k], b[k]), k
    assert masked.num_allocated_blocks < plain.num_allocated_blocks


def test_masked_fusion_errors():
    from gs_fusion import TSDFVolume, fuse_views

    params, cams, masks = _sphere_params(500), _cameras(), _masks()
    bg = torch.zeros(3, device=DEV)
    vol = TSDFVolume(device=DEV, **R.sphere_volume_args())
    with pytest.raises(ValueError):
        fuse_views(vol, params, cams, bg, 0, masks=[masks[0], masks[1][:-1]])          # wrong size
    with pytest.raises(ValueError):
        fuse_views(vol, params, cams, bg, 0, masks=[masks[0], masks[1].transpose(1, 0, 2)[:, :-1]])
    with pytest.raises(ValueError):
        fuse_views(vol, params, cams, bg, 0, masks=masks[:1])                          # one mask, two cameras
    with pytest.raises(ValueError):
        fuse_views(vol, params, cams, bg, 0, masks=[masks[0], np.zeros_like(masks[1])], bounding_box=True)
    assert vol.num_allocated_blocks == 0  # nothing was fused before the masks were checked
