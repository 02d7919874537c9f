#!/usr/bin/env python3
"""Golden vectors for the masked loss head.

The models multiply a per-view mask into both images in front of the loss
(gs_toolkit/models/vanilla_gs.py:915-924, surface_gs.py:917-925, depth_gs.py:424-437):

    gt_img = gt_img * mask
    pred_img = pred_img * mask

and then compute `(1-l)*|gt-pred|.mean() + l*(1 - SSIM(gt, pred))` as without one: the mask is
multiplied in, not selected, and both means stay over all pixels.  Restated here in float64 torch
on top of the SSIM restatement of make_golden_loss.py (the toolkit itself cannot be imported);
loss, terms and gradient come from torch.autograd.  The inputs are rounded to float32 FIRST, so
the stored arrays are exactly what the float64 reference saw.

Per shape one prediction / ground truth pair (a patch with pred == gt, ~5 % of the values above
1) and several masks; a case is (shape, mask, clamp_pred):
  ones, zeros    constant masks
  box            0/1 rectangle; for (24,37) and (48,33) its edges lie between rows 15|16 and
                 columns 31|32, the borders of the kernels' 32x16 tiles
  frac           a 0/1 mask of twice the size resized bilinearly (what the resolution schedule
                 does to a mask): values 0, 1/4, 1/2, 3/4, 1

    python tests/golden/make_golden_masked_loss.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_loss import ssim_msssim  # noqa: E402

LAMBDA = 0.2
SHAPES = {"s": (12, 12), "a": (24, 37), "b": (48, 33)}
BOXES = {"s": (3, 9, 2, 10), "a": (6, 16, 10, 32), "b": (16, 40, 12, 32)}  # rows r0:r1, columns c0:c1
# (shape, mask, clamp_pred)
CASES = (("s", "ones", False), ("s", "zeros", True), ("s", "box", True), ("s", "frac", False),
         ("a", "ones", False), ("a", "zeros", True), ("a", "box", True), ("a", "frac", False),
         ("a", "box", False), ("a", "frac", True),
         ("b", "ones", False), ("b", "zeros", True), ("b", "box", True), ("b", "frac", False))
UNSTABLE = 1e-6      # 0 < |m (pred - gt)| <= this: the sign term may flip between precisions
UNSTABLE_CAP = 1e-3  # at most this fraction of a case's elements


def case_name(shape, mask, clamp):
    return f"{shape}_{mask}_{'clamp' if clamp else 'raw'}"


def make_mask(kind, shape_key, g):
    H, W = SHAPES[shape_key]
    if kind == "ones":
        return torch.ones(H, W)
    if kind == "zeros":
        return torch.zeros(H, W)
    if kind == "box":
        r0, r1, c0, c1 = BOXES[shape_key]
        m = torch.zeros(H, W)
        m[r0:r1, c0:c1] = 1.0
        return m
    hi = (torch.rand(2 * H, 2 * W, generator=g) > 0.4).float()
    hi[: H // 2, : W] = 0.0       # a region of exact zeros ...
    hi[-(H // 2):, -W:] = 1.0     # ... and one of exact ones
    return F.interpolate(hi[None, None], size=[H, W], mode="bilinear", align_corners=False, antialias=False)[0, 0]


def reference(pred32, gt32, mask32, clamp, lam=LAMBDA):
    pred = torch.from_numpy(pred32).double().requires_grad_(True)
    gt = torch.from_numpy(gt32).double()
    m = torch.from_numpy(mask32).double()[..., None]
    x = (torch.clamp(pred, max=1.0) if clamp else pred) * m
    y = gt * m
    l1 = (y - x).abs().mean()
    ss = ssim_msssim(y.permute(2, 0, 1)[None], x.permute(2, 0, 1)[None])
    loss = (1 - lam) * l1 + lam * (1 - ss)
    loss.backward()
    d = (m * ((torch.clamp(pred, max=1.0) if clamp else pred) - gt)).detach().abs()
    unstable = float(((d > 0) & (d <= UNSTABLE)).double().mean())
    return loss.item(), l1.item(), ss.item(), pred.grad.numpy(), unstable


def main():
    out = {"lambda": np.float32(LAMBDA)}
    for si, (key, (H, W)) in enumerate(SHAPES.items()):
        g = torch.Generator().manual_seed(100 + si)
        gt = torch.rand(H, W, 3, generator=g)
        pred = (gt + 0.15 * torch.randn(H, W, 3, generator=g)).clamp(0, 1)
        over = torch.rand(H, W, 3, generator=g) < 0.05
        pred = torch.where(over, 1.0 + 0.3 * torch.rand(H, W, 3, generator=g), pred)
        pred[2:5, 3:9] = gt[2:5, 3:9]  # exact matches: sign(0) = 0 in the L1 term
        out[f"{key}_pred"], out[f"{key}_gt"] = pred.numpy(), gt.numpy()
        for kind in ("ones", "zeros", "box", "frac"):
            out[f"{key}_mask_{kind}"] = make_mask(kind, key, g).numpy()
        if key != "s":  # some of the values above 1 must lie under a zero of the box
            assert int((over & (torch.from_numpy(out[f"{key}_mask_box"]) == 0)[..., None]).sum()) > 10
    for key, kind, clamp in CASES:
        loss, l1, ss, grad, unstable = reference(out[f"{key}_pred"], out[f"{key}_gt"], out[f"{key}_mask_{kind}"], clamp)
        assert unstable <= UNSTABLE_CAP, (key, kind, clamp, unstable)
        n = case_name(key, kind, clamp)
        out.update({f"{n}_loss": np.float64(loss), f"{n}_l1": np.float64(l1), f"{n}_ssim": np.float64(ss),
                    f"{n}_grad": grad.astype(np.float32)})
        print(n, SHAPES[key], f"loss {loss:.6f} l1 {l1:.6f} ssim {ss:.6f} unstable {unstable:.2e}")
    path = os.path.join(HERE, "masked_loss.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
