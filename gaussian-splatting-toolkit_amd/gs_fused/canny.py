"""The Canny edge mask of an image, computed on the GPU: four HIP kernels, no host round trip.

Drop-in for `image2canny` of the reference (gs_toolkit/utils/losses.py:48-58):

    canny_mask = torch.from_numpy(cv2.Canny((image.detach().cpu().numpy() * 255.0).astype(np.uint8), thres1, thres2) / 255.0)
    if not isEdge1:
        canny_mask = 1.0 - canny_mask
    return canny_mask.float()

which copies the ground-truth image to the host, runs OpenCV there and copies a mask back on every training step of
the co-gs model with `use_depth_regularization`.  Here the image stays on the device.  The rule -- `cv::Canny` with its
defaults (aperture 3, L1 gradient), restated -- is the specification in `include/gsraster.h`; `tests/canny_reference.py`
restates it in NumPy + SciPy.  All arithmetic is integer: results are exact and the same on every run.
"""
from typing import Optional

import torch
from torch import Tensor

from rasterizer.cuda import _call, _check, _stream, _typed

_f32, _u8 = torch.float32, torch.uint8


def canny_workspace_bytes(height: int, width: int) -> int:
    """Bytes of scratch `canny` needs for an H x W image (6 per pixel; nothing in it has to be zeroed)."""
    return int(_typed().gsr_canny_workspace_bytes(int(height), int(width)))


def canny(image: Tensor, thres1: float = 50, thres2: float = 150, out: Optional[Tensor] = None,
          workspace: Optional[Tensor] = None) -> Tensor:
    """`cv2.Canny((image * 255.0).astype(uint8), thres1, thres2)` -> uint8 [H,W], 255 on edges and 0 elsewhere.
    `image`: float32 [H,W,3] on the GPU, values expected in [0,1] (out-of-range products saturate, NaN gives 0).
    `out` (uint8 [H,W], contiguous) and `workspace` (uint8, at least `canny_workspace_bytes(H, W)`, 256-byte aligned)
    are allocated when not given.  There is no CPU path: a CPU tensor raises RuntimeError."""
    if not isinstance(image, Tensor) or image.dim() != 3 or image.shape[-1] != 3:
        raise ValueError(f"expected an [H,W,3] image, got {tuple(getattr(image, 'shape', ()))}")
    image = _check(image.detach().contiguous(), "image", _f32)
    H, W = int(image.shape[0]), int(image.shape[1])
    dev = image.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((H, W), dtype=_u8, device=dev)
        else:
            _check(out, "out", _u8)
            if tuple(out.shape) != (H, W) or out.device != dev:
                raise ValueError(f"out must be uint8 [{H},{W}] on {dev}")
        if H * W == 0:
            return out
        need = canny_workspace_bytes(H, W)
        if need == 0:
            raise ValueError(f"canny: an image of {H} x {W} pixels is too large")
        if workspace is None:
            workspace = torch.empty((need,), dtype=_u8, device=dev)
        else:
            _check(workspace, "workspace", _u8)
        _call("gsr_canny", H, W, image, float(thres1), float(thres2), workspace, workspace.numel(), out, _stream(dev))
    return out


def image2canny(image: Tensor, thres1: float, thres2: float, isEdge1: bool = True) -> Tensor:
    """The reference's `image2canny` (utils/losses.py:48-58), signature and values: float32 [H,W], 1 on edges and 0
    elsewhere, or with ``isEdge1=False`` 1 on NON-edges -- the mask the co-gs depth regularisation multiplies with.
    The result is on the image's device (the reference returns a CPU tensor the model moves back)."""
    edges = canny(image, thres1, thres2).to(_f32) / 255.0
    return edges if isEdge1 else 1.0 - edges
