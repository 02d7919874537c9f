"""(1 - lambda) * L1 + lambda * (1 - SSIM) in two HIP kernels.

Drop-in for the loss of `GaussianSplattingModel.get_loss_dict`
(gs_toolkit/models/vanilla_gs.py:926-944):

    Ll1 = torch.abs(gt_img - pred_img).mean()
    simloss = 1 - self.ssim(gt_img.permute(2, 0, 1)[None], pred_img.permute(2, 0, 1)[None])
    main_loss = (1 - ssim_lambda) * Ll1 + ssim_lambda * simloss

with `self.ssim = pytorch_msssim.SSIM(data_range=1.0, size_average=True, channel=3)`.
`l1_ssim_loss(pred_img, gt_img, ssim_lambda)` returns the same scalar; its backward
writes d loss / d pred_img -- the cotangent the compositing backward consumes --
in one kernel.  Differentiable w.r.t. `pred` only (the ground truth is data).

Every head takes the per-view `mask` the models multiply into both images in front of the
loss (vanilla_gs.py:915-924, surface_gs.py:917-925, depth_gs.py:424-437):

    mask = self._downscale_if_required(batch["mask"]).to(self.device)
    gt_img, pred_img = gt_img * mask, pred_img * mask

`l1_ssim_loss(pred_img, gt_img, ssim_lambda, mask=mask)` computes the loss of those two
products inside the same two kernels: the mask is multiplied in, nothing is selected, and
the means stay over all pixels (the reference does not renormalise by the mask's area).
"""

import torch
from torch import Tensor
from torch.autograd import Function

from rasterizer.cuda import _call, _check, _stream

_f32 = torch.float32
WORKSPACE_DOUBLES = 2 * 64  # GSR_LOSS_WORKSPACE_DOUBLES (include/gsraster.h)


def _mask_arg(mask, H: int, W: int, ref: Tensor) -> Tensor:
    """A per-view mask as the masked kernels take it: contiguous float32 [H,W] on the images' device.  Accepts [H,W]
    or [H,W,1]; float32 as it is, bool / uint8 through `.to(float32)`."""
    if not isinstance(mask, Tensor):
        raise RuntimeError("mask must be a tensor")
    if tuple(mask.shape) not in ((H, W), (H, W, 1)):
        raise ValueError(f"expected a mask [{H},{W}] or [{H},{W},1] for these images, got {tuple(mask.shape)}")
    if mask.device != ref.device:
        raise RuntimeError(f"mask must be on the images' device {ref.device}, got {mask.device}")
    if mask.dtype in (torch.bool, torch.uint8):
        mask = mask.to(_f32)
    elif mask.dtype != _f32:
        raise ValueError(f"mask must be float32, bool or uint8, got {mask.dtype}")
    return _check(mask.detach().reshape(H, W).contiguous(), "mask", _f32)


class _L1SSIM(Function):
    @staticmethod
    def forward(ctx, pred: Tensor, gt: Tensor, ssim_lambda: float, clamp_pred: bool, mask=None):
        if pred.dim() != 3 or pred.shape[-1] != 3 or pred.shape != gt.shape:
            raise ValueError(f"expected two [H,W,3] images, got {tuple(pred.shape)} and {tuple(gt.shape)}")
        H, W = int(pred.shape[0]), int(pred.shape[1])
        if H <= 10 or W <= 10:
            raise ValueError("images must be larger than the 11x11 SSIM window")
        pred = _check(pred.contiguous(), "pred", _f32)
        gt = _check(gt.contiguous(), "gt", _f32)
        if mask is not None:
            mask = _mask_arg(mask, H, W, pred)
        dev = pred.device
        with torch.cuda.device(dev):
            maps = torch.empty((9, H - 10, W - 10), dtype=_f32, device=dev)
            work = torch.empty((WORKSPACE_DOUBLES,), dtype=torch.float64, device=dev)
            loss = torch.empty((), dtype=_f32, device=dev)
            terms = torch.empty((2,), dtype=_f32, device=dev)  # L1 mean, SSIM mean
            if mask is None:
                _call("gsr_l1_ssim_forward", H, W, ssim_lambda, 1 if clamp_pred else 0, pred, gt, maps, work, loss,
                      terms, _stream(dev))
            else:
                _call("gsr_l1_ssim_masked_forward", H, W, ssim_lambda, 1 if clamp_pred else 0, pred, gt, mask, maps,
                      work, loss, terms, _stream(dev))
        if mask is None:
            ctx.save_for_backward(pred, gt, maps)
        else:
            ctx.save_for_backward(pred, gt, maps, mask)
        ctx.ssim_lambda = float(ssim_lambda)
        ctx.clamp_pred = bool(clamp_pred)
        ctx.hw = (H, W)
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    def backward(ctx, v_loss, _v_terms):
        pred, gt, maps, *masks = ctx.saved_tensors
        H, W = ctx.hw
        dev = pred.device
        up = v_loss.to(_f32).reshape(1).contiguous()
        with torch.cuda.device(dev):
            v_pred = torch.empty_like(pred)
            if not masks:
                _call("gsr_l1_ssim_backward", H, W, ctx.ssim_lambda, 1 if ctx.clamp_pred else 0, up, pred, gt, maps,
                      v_pred, _stream(dev))
            else:
                _call("gsr_l1_ssim_masked_backward", H, W, ctx.ssim_lambda, 1 if ctx.clamp_pred else 0, up, pred, gt,
                      masks[0], maps, v_pred, _stream(dev))
        return v_pred, None, None, None, None


def l1_ssim_loss(pred: Tensor, gt: Tensor, ssim_lambda: float = 0.2, return_terms: bool = False,
                 clamp_pred: bool = False, mask=None):
    """Scalar loss (fp32, on device).  With `return_terms`, also the L1 mean and the
    SSIM value (detached diagnostics; gradients flow through the loss only).
    `clamp_pred`: compute the loss of `torch.clamp(pred, max=1.0)` (what the models
    feed it, vanilla_gs.py:857) without that op and its backward.
    `mask` ([H,W] or [H,W,1]; float32, bool or uint8; on the images' device): the loss of
    ``pred * mask`` and ``gt * mask`` (of ``torch.clamp(pred, max=1.0) * mask`` under
    `clamp_pred`), as the models form them (vanilla_gs.py:915-924), without the two
    multiplies and their backward.  Multiplied in, not selected: the means stay over all
    pixels, fractional values are allowed, and a non-finite `pred` under a zero is what
    ``pred * 0`` is.  The mask is a constant (no gradient); the gradient of `pred` is 0
    wherever the mask is 0."""
    loss, terms = _L1SSIM.apply(pred, gt, ssim_lambda, clamp_pred, mask)
    if return_terms:
        return loss, terms[0], terms[1]
    return loss


class L1SSIMLoss(torch.nn.Module):
    def __init__(self, ssim_lambda: float = 0.2, clamp_pred: bool = False):
        super().__init__()
        self.ssim_lambda = ssim_lambda
        self.clamp_pred = clamp_pred

    def forward(self, pred: Tensor, gt: Tensor, mask=None) -> Tensor:
        return l1_ssim_loss(pred, gt, self.ssim_lambda, clamp_pred=self.clamp_pred, mask=mask)


class _L1(Function):
    @staticmethod
    def forward(ctx, pred: Tensor, gt: Tensor, weight: float, clamp_pred: bool, mask=None):
        if pred.shape != gt.shape or pred.numel() == 0:
            raise ValueError(f"expected two images of one (non-empty) shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")
        if mask is not None and (pred.dim() != 3 or pred.shape[-1] != 3):
            raise ValueError(f"a mask needs two [H,W,3] images, got {tuple(pred.shape)}")
        pred = _check(pred.contiguous(), "pred", _f32)
        gt = _check(gt.contiguous(), "gt", _f32)
        if mask is not None:
            mask = _mask_arg(mask, int(pred.shape[0]), int(pred.shape[1]), pred)
        dev = pred.device
        with torch.cuda.device(dev):
            work = torch.empty((64,), dtype=torch.float64, device=dev)
            loss = torch.empty((), dtype=_f32, device=dev)
            if mask is None:
                _call("gsr_l1_forward", pred.numel(), weight, 1 if clamp_pred else 0, pred, gt, work, loss,
                      _stream(dev))
            else:
                _call("gsr_l1_masked_forward", pred.numel(), weight, 1 if clamp_pred else 0, pred, gt, mask, work, loss,
                      _stream(dev))
        if mask is None:
            ctx.save_for_backward(pred, gt)
        else:
            ctx.save_for_backward(pred, gt, mask)
        ctx.weight, ctx.clamp_pred = float(weight), bool(clamp_pred)
        return loss

    @staticmethod
    def backward(ctx, v_loss):
        pred, gt, *masks = ctx.saved_tensors
        dev = pred.device
        up = v_loss.to(_f32).reshape(1).contiguous()
        with torch.cuda.device(dev):
            v_pred = torch.empty_like(pred)
            if not masks:
                _call("gsr_l1_backward", pred.numel(), ctx.weight, 1 if ctx.clamp_pred else 0, up, pred, gt, v_pred,
                      _stream(dev))
            else:
                _call("gsr_l1_masked_backward", pred.numel(), ctx.weight, 1 if ctx.clamp_pred else 0, up, pred, gt,
                      masks[0], v_pred, _stream(dev))
        return v_pred, None, None, None, None


def l1_loss(pred: Tensor, gt: Tensor, weight: float = 1.0, clamp_pred: bool = False, mask=None) -> Tensor:
    """``weight * |gt - pred|.mean()`` in one streaming kernel each way -- the photometric loss of the co-gs
    model AS ITS SOURCE COMPUTES IT: `DepthGSModel.get_loss_dict` (depth_gs.py:445-448) writes
    ``loss_dict["main_loss"] = (1 - ssim_lambda) * Ll1`` and puts ``+ssim_lambda * simloss`` on a line of its own,
    an expression statement whose value is dropped, so ``weight = 1 - ssim_lambda`` and no SSIM term.
    `clamp_pred`: the loss of ``torch.clamp(pred, max=1.0)`` (depth_gs.py:343) without that op.
    `mask` ([H,W] or [H,W,1] for two [H,W,3] images; float32, bool or uint8): the loss of ``pred * mask`` and
    ``gt * mask`` (depth_gs.py:424-437), the mean still over all 3 H W values; see `l1_ssim_loss`."""
    return _L1.apply(pred, gt, weight, clamp_pred, mask)


class _DepthL1(Function):
    @staticmethod
    def forward(ctx, depth: Tensor, alpha: Tensor, gt: Tensor, mask=None):
        if depth.numel() != alpha.numel() or depth.numel() != gt.numel() or depth.numel() == 0:
            raise ValueError("depth, alpha and gt_depth must have the same (non-zero) number of pixels")
        if mask is not None and gt.dim() < 2:
            raise ValueError(f"a mask needs gt_depth as an image [H,W] (or [H,W,1]), got {tuple(gt.shape)}")
        d = _check(depth.contiguous(), "depth", _f32)
        a = _check(alpha.contiguous(), "alpha", _f32)
        g = _check(gt.contiguous(), "gt_depth", _f32)
        if mask is not None:
            mask = _mask_arg(mask, int(gt.shape[0]), int(gt.shape[1]), d)
        dev = d.device
        with torch.cuda.device(dev):
            far = d.detach().max().reshape(1)  # depth_im.detach().max() of the reference
            work = torch.empty((64,), dtype=torch.float64, device=dev)
            loss = torch.empty((), dtype=_f32, device=dev)
            if mask is None:
                _call("gsr_depth_l1_forward", d.numel(), d, a, g, far, work, loss, _stream(dev))
            else:
                _call("gsr_depth_l1_masked_forward", d.numel(), d, a, g, mask, far, work, loss, _stream(dev))
        if mask is None:
            ctx.save_for_backward(d, a, g, far)
        else:
            ctx.save_for_backward(d, a, g, far, mask)
        ctx.shapes = (depth.shape, alpha.shape)
        return loss

    @staticmethod
    def backward(ctx, v_loss):
        d, a, g, far, *masks = ctx.saved_tensors
        dev = d.device
        up = v_loss.to(_f32).reshape(1).contiguous()
        with torch.cuda.device(dev):
            v_d = torch.empty_like(d)
            v_a = torch.empty_like(a)
            if not masks:
                _call("gsr_depth_l1_backward", d.numel(), up, d, a, g, far, v_d, v_a, _stream(dev))
            else:
                _call("gsr_depth_l1_masked_backward", d.numel(), up, d, a, g, masks[0], far, v_d, v_a, _stream(dev))
        return v_d.view(ctx.shapes[0]), v_a.view(ctx.shapes[1]), None, None


def depth_l1_loss(depth_acc: Tensor, alpha: Tensor, gt_depth: Tensor, mask=None) -> Tensor:
    """Depth head of the co-gs model in two launches (+ one max): with
    ``pred = where(alpha > 0, depth_acc / alpha, depth_acc.detach().max())``
    (depth_gs.py:356-363) returns ``|gt * (gt > 0) - pred * (gt > 0)|.mean()``
    (depth_gs.py:531-538).  ``depth_acc`` is the raw output of the depth compositing
    pass, ``alpha`` the accumulated opacity of the RGB pass; differentiable w.r.t. both.
    `mask` ([H,W] or [H,W,1] like ``gt_depth``; float32, bool or uint8): both depth images are multiplied by it first
    (depth_gs.py:424-437): ``g = gt * mask``, ``p = pred * mask`` and the value is ``|g * (g > 0) - p * (g > 0)|.mean()``
    over all pixels; the cotangents of ``depth_acc`` and ``alpha`` are scaled by the mask."""
    return _DepthL1.apply(depth_acc, alpha, gt_depth, mask)


DEPTH_REG_WORKSPACE_DOUBLES = 1024  # GSR_DEPTH_REG_WORKSPACE_DOUBLES (include/gsraster.h)


class _DepthReg(Function):
    @staticmethod
    def forward(ctx, pred: Tensor, mask: Tensor):
        shape = pred.shape
        if pred.dim() == 3 and shape[-1] == 1:
            pred = pred[..., 0]
        if pred.dim() != 2 or pred.shape != mask.shape or pred.numel() == 0:
            raise ValueError(f"expected pred [H,W] (or [H,W,1]) and mask [H,W], non-empty, got {tuple(shape)} and "
                             f"{tuple(mask.shape)}")
        p = _check(pred.contiguous(), "pred_depth", _f32)
        m = _check(mask.contiguous(), "mask", _f32)
        H, W = int(p.shape[0]), int(p.shape[1])
        dev = p.device
        with torch.cuda.device(dev):
            scratch = torch.empty((2, H, W), dtype=_f32, device=dev)
            work = torch.empty((DEPTH_REG_WORKSPACE_DOUBLES,), dtype=torch.float64, device=dev)
            loss = torch.empty((), dtype=_f32, device=dev)
            _call("gsr_depth_reg_forward", H, W, p, m, scratch, work, loss, _stream(dev))
        ctx.save_for_backward(p, m, scratch)
        ctx.shape = shape
        return loss

    @staticmethod
    def backward(ctx, v_loss):
        p, m, scratch = ctx.saved_tensors
        H, W = int(p.shape[0]), int(p.shape[1])
        dev = p.device
        up = v_loss.to(_f32).reshape(1).contiguous()
        with torch.cuda.device(dev):
            v_pred = torch.empty_like(p)
            _call("gsr_depth_reg_backward", H, W, up, p, m, scratch, v_pred, _stream(dev))
        return v_pred.view(ctx.shape), None


def depth_reg_loss(pred_depth: Tensor, mask: Tensor) -> Tensor:
    """The depth regularisation of the co-gs model (depth_gs.py:521-528 with `nearMean_map` and `l2_loss`,
    utils/losses.py:8-9, 61-81) in two launches each way: with ``m = mask * (pred > 0)``, ``near`` = the plus-shaped
    five-tap sum (zero padding) of ``pred * m`` over that of ``m`` plus 1e-8, returns
    ``((near - pred * (pred > 0)) ** 2).mean()``.  ``pred_depth`` [H,W] or [H,W,1], ``mask`` [H,W] of any values (the
    model passes the non-edge mask, ``image2canny(gt_img, 50, 150, isEdge1=False)``).  Differentiable w.r.t.
    ``pred_depth`` only -- the mask and ``pred > 0`` are constants, as in the source.  The scalar is summed in float64
    in a fixed order: two runs are bit-equal."""
    return _DepthReg.apply(pred_depth, mask)
