"""The monocular-depth terms of the co-gs loss (`use_est_depth`, DepthGSModel.get_loss_dict, depth_gs.py:477-531) as
three fused heads on csrc/mono_depth.hip (the rule is stated in include/gsraster.h):

    local_pearson_loss(pred_depth, gt_depth, box_p, rows, cols, mask=None)          utils/losses.py:26-45
    log_depth_loss(pred_depth, gt_depth, gt_img, scale=1.0, shift=0.0, mask=None)   depth_gs.py:492-519
    tv_loss(pred_depth, mask=None)                                                  utils/losses.py:197-207

Conventions of `gs_fused.depth_reg_loss`: float32 in and out, float64 per-pixel arithmetic, float64 sums in a fixed
order without atomics (two runs are bit-equal, the local-Pearson gradient over overlapping patches included),
differentiable w.r.t. the predicted depth only, CUDA tensors only.  `mask` follows the other heads (`loss._mask_arg`):
``pred * mask`` and ``gt * mask`` are formed inside the kernels, nothing is selected, the means stay over all pixels
and the cotangent is scaled by the mask."""
import torch
from torch import Tensor
from torch.autograd import Function

from rasterizer.cuda import _call, _check, _stream

from .loss import _mask_arg

_f32 = torch.float32
WORKSPACE_DOUBLES = 2048  # GSR_MONO_DEPTH_WORKSPACE_DOUBLES (include/gsraster.h)


def _depth_arg(t, name: str) -> Tensor:
    """A depth image as the kernels take it: contiguous float32 [H,W] (from [H,W] or [H,W,1]) on the GPU."""
    if not isinstance(t, Tensor):
        raise RuntimeError(f"{name} must be a tensor")
    if t.dim() == 3 and t.shape[-1] == 1:
        t = t[..., 0]
    if t.dim() != 2 or t.numel() == 0:
        raise ValueError(f"expected {name} [H,W] (or [H,W,1]), non-empty, got {tuple(t.shape)}")
    return _check(t.contiguous(), name, _f32)


def _pair(pred, gt, mask):
    p = _depth_arg(pred, "pred_depth")
    g = _depth_arg(gt.detach() if isinstance(gt, Tensor) else gt, "gt_depth")
    if g.shape != p.shape:
        raise ValueError(f"pred_depth and gt_depth must have one shape, got {tuple(p.shape)} and {tuple(g.shape)}")
    if g.device != p.device:
        raise RuntimeError(f"gt_depth must be on pred_depth's device {p.device}, got {g.device}")
    H, W = int(p.shape[0]), int(p.shape[1])
    m = None if mask is None else _mask_arg(mask, H, W, p)
    return p, g, m, H, W


def _upstream(v_loss: Tensor) -> Tensor:
    return v_loss.to(_f32).reshape(1).contiguous()


class _LocalPearson(Function):
    @staticmethod
    def forward(ctx, pred: Tensor, gt: Tensor, box_p: int, rows: Tensor, cols: Tensor, mask=None):
        shape = pred.shape if isinstance(pred, Tensor) else None
        p, g, m, H, W = _pair(pred, gt, mask)
        box_p = int(box_p)
        if box_p < 1 or box_p > min(H, W):
            raise ValueError(f"box_p must be in [1, min(H, W) = {min(H, W)}], got {box_p}")
        for name, t in (("rows", rows), ("cols", cols)):
            if not isinstance(t, Tensor):
                raise RuntimeError(f"{name} must be a tensor")
            if t.dtype not in (torch.int64, torch.int32):
                raise ValueError(f"{name} must be int64 or int32, got {t.dtype}")
            if t.dim() != 1:
                raise ValueError(f"{name} must be one-dimensional, got {tuple(t.shape)}")
        if rows.dtype != cols.dtype or rows.shape != cols.shape:
            raise ValueError("rows and cols must have one dtype and one length")
        rows = _check(rows.contiguous(), "rows")
        cols = _check(cols.contiguous(), "cols")
        dev = p.device
        if rows.device != dev or cols.device != dev:
            raise RuntimeError(f"rows and cols must be on the images' device {dev}")
        n_corr = int(rows.numel())
        if n_corr >= 2 ** 31:
            raise ValueError("too many patches")
        i64 = 1 if rows.dtype == torch.int64 else 0
        with torch.cuda.device(dev):
            stats = torch.empty((max(n_corr, 1), 5), dtype=torch.float64, device=dev)
            loss = torch.empty((), dtype=_f32, device=dev)
            _call("gsr_local_pearson_forward", H, W, box_p, n_corr, p, g, m, rows, cols, i64, stats, loss, _stream(dev))
        saved = (p, g, rows, cols, stats) + (() if m is None else (m,))
        ctx.save_for_backward(*saved)
        ctx.args = (H, W, box_p, n_corr, i64)
        ctx.shape = shape
        return loss

    @staticmethod
    def backward(ctx, v_loss):
        p, g, rows, cols, stats, *masks = ctx.saved_tensors
        H, W, box_p, n_corr, i64 = ctx.args
        dev = p.device
        up = _upstream(v_loss)
        with torch.cuda.device(dev):
            v_pred = torch.empty_like(p)
            _call("gsr_local_pearson_backward", H, W, box_p, n_corr, up, p, g, masks[0] if masks else None, rows, cols,
                  i64, stats, v_pred, _stream(dev))
        return v_pred.view(ctx.shape), None, None, None, None, None


def local_pearson_loss(pred_depth: Tensor, gt_depth: Tensor, box_p: int, rows: Tensor, cols: Tensor,
                       mask=None) -> Tensor:
    """The mean over the given ``box_p x box_p`` patches of ``1 - cov / (std * std)`` between the two depth images
    (utils/losses.py:26-45: a biased covariance over unbiased deviations, as written), one workgroup per patch and a
    one-workgroup sum; the backward is one kernel, one thread per pixel, that adds the closed-form affine term of every
    patch covering the pixel in ascending patch index -- no index tensors, no atomics, bit-equal over two runs however
    the patches overlap.  ``rows`` / ``cols``: the patches' top-left corners, int64 (as `torch.randint` returns them)
    or int32, on the device; they are read there (`harness.cogs_losses.local_pearson_patches` draws them).
    ``pred_depth``, ``gt_depth`` [H,W] or [H,W,1].  A constant patch (in either image) or ``box_p == 1`` is 0 / 0: the
    loss is NaN and the gradient NaN on that patch's pixels only, as the source; a corner outside
    ``[0, H - box_p] x [0, W - box_p]`` is not read: NaN loss, no gradient from it; no patches: NaN.
    ``box_p`` outside ``[1, min(H, W)]`` raises ValueError."""
    return _LocalPearson.apply(pred_depth, gt_depth, box_p, rows, cols, mask)


_SCALE_SHIFT = {}  # (device, scale, shift) as Python floats -> the float32 [2] buffer (no upload per step)


def _scale_shift_arg(scale, shift, dev) -> Tensor:
    if not isinstance(scale, Tensor) and not isinstance(shift, Tensor):
        key = (dev, float(scale), float(shift))
        buf = _SCALE_SHIFT.get(key)
        if buf is None:
            if len(_SCALE_SHIFT) >= 64:
                _SCALE_SHIFT.clear()
            buf = _SCALE_SHIFT[key] = torch.tensor([key[1], key[2]], dtype=_f32, device=dev)
        return buf
    parts = []
    for name, v in (("scale", scale), ("shift", shift)):
        if isinstance(v, Tensor):
            if v.numel() != 1:
                raise ValueError(f"{name} must be a number or a tensor of one element, got {tuple(v.shape)}")
            if v.device != dev:
                raise RuntimeError(f"{name} must be on the images' device {dev}, got {v.device}")
            parts.append(v.detach().to(_f32).reshape(1))
        else:
            parts.append(torch.tensor([float(v)], dtype=_f32, device=dev))
    return torch.cat(parts)


class _LogDepth(Function):
    @staticmethod
    def forward(ctx, pred: Tensor, gt: Tensor, img: Tensor, scale, shift, mask=None):
        shape = pred.shape if isinstance(pred, Tensor) else None
        p, g, m, H, W = _pair(pred, gt, mask)
        if not isinstance(img, Tensor):
            raise RuntimeError("gt_img must be a tensor")
        if tuple(img.shape) != (H, W, 3):
            raise ValueError(f"expected gt_img [{H},{W},3], got {tuple(img.shape)}")
        img = _check(img.detach().contiguous(), "gt_img", _f32)
        dev = p.device
        if img.device != dev:
            raise RuntimeError(f"gt_img must be on pred_depth's device {dev}, got {img.device}")
        with torch.cuda.device(dev):
            ss = _scale_shift_arg(scale, shift, dev)
            work = torch.empty((WORKSPACE_DOUBLES,), dtype=torch.float64, device=dev)
            loss = torch.empty((), dtype=_f32, device=dev)
            _call("gsr_log_depth_forward", H, W, p, g, img, ss, m, work, loss, _stream(dev))
        ctx.save_for_backward(*((p, g, img, ss) + (() if m is None else (m,))))
        ctx.shape = shape
        return loss

    @staticmethod
    def backward(ctx, v_loss):
        p, g, img, ss, *masks = ctx.saved_tensors
        H, W = int(p.shape[0]), int(p.shape[1])
        dev = p.device
        up = _upstream(v_loss)
        with torch.cuda.device(dev):
            v_pred = torch.empty_like(p)
            _call("gsr_log_depth_backward", H, W, up, p, g, img, ss, masks[0] if masks else None, v_pred, _stream(dev))
        return v_pred.view(ctx.shape), None, None, None, None, None


def log_depth_loss(pred_depth: Tensor, gt_depth: Tensor, gt_img: Tensor, scale=1.0, shift=0.0, mask=None) -> Tensor:
    """The edge-aware scaled log-depth term (depth_gs.py:492-519): ``log(1 + |gt - (scale * pred + shift)|)`` weighted
    along x by ``exp(-mean_c |img[:, :-1] - img[:, 1:]|)`` and along y by the row analogue, the two weighted means
    added -- one streaming kernel each way, the backward recomputes (no scratch plane).  ``scale`` / ``shift``: Python
    numbers or one-element device tensors (the reference's ``batch["mono_depth_scale"]``); they reach the kernel as a
    float32 [2] device buffer, nothing is read back, and no gradient flows to them.  ``gt_img`` [H,W,3] is taken as the
    caller has it (under a mask: the masked target).  ``H == 1`` or ``W == 1``: NaN, the mean of an empty tensor."""
    return _LogDepth.apply(pred_depth, gt_depth, gt_img, scale, shift, mask)


class _TV(Function):
    @staticmethod
    def forward(ctx, pred: Tensor, mask=None):
        shape = pred.shape if isinstance(pred, Tensor) else None
        p = _depth_arg(pred, "pred_depth")
        H, W = int(p.shape[0]), int(p.shape[1])
        m = None if mask is None else _mask_arg(mask, H, W, p)
        dev = p.device
        with torch.cuda.device(dev):
            work = torch.empty((WORKSPACE_DOUBLES,), dtype=torch.float64, device=dev)
            loss = torch.empty((), dtype=_f32, device=dev)
            _call("gsr_tv_forward", H, W, p, m, work, loss, _stream(dev))
        ctx.save_for_backward(*((p,) + (() if m is None else (m,))))
        ctx.shape = shape
        return loss

    @staticmethod
    def backward(ctx, v_loss):
        p, *masks = ctx.saved_tensors
        H, W = int(p.shape[0]), int(p.shape[1])
        dev = p.device
        up = _upstream(v_loss)
        with torch.cuda.device(dev):
            v_pred = torch.empty_like(p)
            _call("gsr_tv_backward", H, W, up, p, masks[0] if masks else None, v_pred, _stream(dev))
        return v_pred.view(ctx.shape), None


def tv_loss(pred_depth: Tensor, mask=None) -> Tensor:
    """``|pred[:, :-1] - pred[:, 1:]|.mean() + |pred[:-1] - pred[1:]|.mean()`` of the [H,W] (or [H,W,1]) depth
    (utils/losses.py:197-207) in one streaming kernel each way; the backward gathers the signs of the four differences a
    pixel takes part in, ``sign(0) = 0``.  ``H == 1`` or ``W == 1``: NaN, the mean of an empty tensor."""
    return _TV.apply(pred_depth, mask)
