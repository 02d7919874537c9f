#!/usr/bin/env python3
"""Generate tests/golden/depth_reg.npz from the REFERENCE's own code for co-gs's depth regularisation.

Runs ONLY in the build container (it reads /root/reference).  As in make_golden_cogs.py the pieces are lifted out with
`ast` AT GENERATION TIME and executed unmodified on torch CPU float32 tensors:
  * utils/losses.py: the functions `l2_loss` and `nearMean_map`, and the module-level `with torch.no_grad():` block
    that builds `conv` (the plus-shaped 3x3 convolution) -- WITHOUT its single statement `conv = conv.cuda()`: the
    generating container has no device, and the statement moves the weights without changing a value;
  * models/depth_gs.py, `DepthGSModel.get_loss_dict`: the body of `if self.config.use_depth_regularization:`
    (lines 522-528), run with the case's `pred_depth` (requires_grad) and `canny_mask` as locals.
`torch.autograd` gives d loss / d pred.  Nothing of the reference's source is stored: the committed .npz holds the
inputs, the loss and the gradient that code produced.

The Canny masks among the cases come from tests/canny_reference.py (the non-edge mask, as the model passes it).

    python tests/golden/make_golden_depth_reg.py
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import canny_reference as CR  # noqa: E402
from make_golden_cogs import _guarded_blocks, _run  # noqa: E402

REF_LOSSES = "/root/reference/gs_toolkit/utils/losses.py"
REF_MODEL = "/root/reference/gs_toolkit/models/depth_gs.py"


def _losses_namespace():
    src = open(REF_LOSSES).read()
    tree = ast.parse(src)
    body, dropped = [], 0
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in ("l2_loss", "nearMean_map"):
            body.append(node)
        elif isinstance(node, ast.With) and "conv" in (ast.get_source_segment(src, node) or ""):
            keep = [s for s in node.body if (ast.get_source_segment(src, s) or "").strip() != "conv = conv.cuda()"]
            dropped += len(node.body) - len(keep)
            node.body = keep
            body.append(node)
    assert dropped == 1 and len(body) == 3, (dropped, len(body))
    ns = {"torch": torch, "np": np}
    _run(body, REF_LOSSES, ns)
    return ns


def main():
    L = _losses_namespace()
    block = _guarded_blocks(REF_MODEL, "get_loss_dict", ("use_depth_regularization",))["use_depth_regularization"]
    rng = np.random.default_rng(20241018)

    def pred_of(h, w, dead=0.1):
        p = rng.uniform(0.5, 4.0, (h, w))
        hole = rng.uniform(size=(h, w)) < dead
        return np.where(hole, np.where(rng.uniform(size=(h, w)) < 0.5, 0.0, -rng.uniform(0.1, 1.0, (h, w))), p).astype(np.float32)

    canny_mask = lambda h, w, seed: CR.image2canny(CR.smooth_random(h, w, seed), 50, 150, isEdge1=False)
    random_mask = lambda h, w: (rng.uniform(size=(h, w)) < 0.7).astype(np.float32)
    cases = [
        ("canny_24x40", pred_of(24, 40), canny_mask(24, 40, 1)),
        ("canny_11x13", pred_of(11, 13), canny_mask(11, 13, 2)),
        ("random_24x40", pred_of(24, 40), random_mask(24, 40)),
        ("random_11x13", pred_of(11, 13), random_mask(11, 13)),
        ("dead_11x13", -np.abs(pred_of(11, 13, 0.3)), random_mask(11, 13)),  # pred <= 0 everywhere: cnt = 0, loss 0
        ("nomask_24x40", pred_of(24, 40), np.zeros((24, 40), np.float32)),
    ]
    out = {"cases": np.array([c[0] for c in cases])}
    for name, pred, mask in cases:
        tp = torch.from_numpy(pred).requires_grad_(True)
        ns = dict(L, pred_depth=tp, canny_mask=torch.from_numpy(mask), loss_dict={})
        _run(block, REF_MODEL, ns)
        loss = ns["loss_dict"]["depth_reg_loss"]
        assert loss.dtype == torch.float32
        (grad,) = torch.autograd.grad(loss, tp)
        out[name + "_pred"], out[name + "_mask"] = pred, mask
        out[name + "_loss"] = np.float32(loss.item())
        out[name + "_grad"] = grad.numpy().astype(np.float32)
        print(f"{name}: mask mean {mask.mean():.3f}, pred <= 0: {(pred <= 0).mean():.3f}, loss {loss.item():.6g}, "
              f"max |grad| {np.abs(grad.numpy()).max():.3g}")
    path = os.path.join(HERE, "depth_reg.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
