"""The 3D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024, section 4.1) on csrc/filter3d.hip (DESIGN.md section
4.22; the rule is stated in include/gsraster.h).

A Gaussian smaller than the finest sampling interval of any training view is unconstrained by the data: rendered closer
or at a higher resolution it shows as needles and holes.  The filter convolves every Gaussian with an isotropic
Gaussian of variance ``variance / nu^2``, ``nu`` the largest ``fx / z`` over the training cameras that see its centre:

    filter_cameras(cams, device)                               -> the camera table [V,20] of the sampling pass
    sampling_filter_3d(means, cameras, variance=0.2, ...)      -> filter [N]: sqrt(variance) / nu (one HIP pass)
    activate_gaussians(..., filter_3d=filter)                  -> the activations with the filter folded in (one launch
                                                                  each way; gs_fused.activations)
    apply_filter_3d(scales, opacities, filter)                 -> the same formula as differentiable torch ops
    bake_filter_3d(log_scales, opacity_logits, filter)         -> raw parameters whose plain activations ARE the
                                                                  filtered model (Mip-Splatting's fused PLY)

With ``s`` the activated scales, ``o`` the opacity and ``f`` the filter:

    s'_k = sqrt(s_k^2 + f^2)        c = prod_k s_k / s'_k        o' = o c

(the determinant ratio of the two covariances: the filtered Gaussian keeps its integral).  No gradient reaches ``f``.
``sampling_filter_3d`` and the filtered ``activate_gaussians`` take CUDA tensors only (no CPU fallback);
``apply_filter_3d`` and ``bake_filter_3d`` are plain torch and run anywhere.
"""
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor
from torch.autograd import Function

_f32 = torch.float32
CAMERA_STRIDE = 20  # floats per camera row: 12 view matrix, 6 intrinsics, 2 unread (rows stay 16-byte aligned)
WORKSPACE_BYTES = 16  # GSR_FILTER3D_WORKSPACE_BYTES


def _camera_row(cam) -> np.ndarray:
    vm = cam.viewmat
    vm = vm.detach().cpu().numpy() if isinstance(vm, Tensor) else np.asarray(vm)
    if vm.shape[-1] != 4 or vm.shape[0] < 3:
        raise ValueError(f"filter_cameras: viewmat must hold at least 3x4 values, got {tuple(vm.shape)}")
    row = np.zeros(CAMERA_STRIDE, np.float32)
    row[:12] = vm[:3, :].astype(np.float32).reshape(12)
    row[12:18] = [cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height]
    return row


def filter_cameras(cams: Sequence, device) -> Tensor:
    """-> float32 [V,20] on `device`, per row the top 3x4 of ``viewmat`` (row-major), ``fx, fy, cx, cy, width, height``
    and two unread words.  ``cams``: a sequence of `harness.pipeline.CameraTensors` or `harness.scene.Camera` (anything
    with those attributes).  Built on the host: a training run does it once per resolution."""
    cams = list(cams)
    table = np.stack([_camera_row(c) for c in cams]) if cams else np.zeros((0, CAMERA_STRIDE), np.float32)
    return torch.from_numpy(table).to(device)


def _require_cuda(t: Tensor, op: str, name: str) -> None:
    if not isinstance(t, Tensor):
        raise ValueError(f"{op}: {name} must be a tensor")
    if not t.is_cuda:
        raise ValueError(f"{op}: {name} is a CPU tensor; this op runs on CUDA tensors only (no CPU fallback)")


@torch.no_grad()
def sampling_filter_3d(means: Tensor, cameras: Union[Tensor, Sequence], *, variance: float = 0.2, near: float = 0.2,
                       margin: float = 0.15, out: Optional[Tensor] = None) -> Tensor:
    """-> filter float32 [N]: ``sqrt(variance) / nu_i`` with ``nu_i`` the largest ``fx / z`` over the cameras that see
    Gaussian i (``z > near``, the projected centre inside the image grown by ``margin`` of its size on every side); a
    Gaussian no camera sees takes the largest filter of any seen one; all zeros when nothing is seen.  float32, every
    operation rounded on its own (include/gsraster.h): bit-reproducible.  ``cameras``: the table of `filter_cameras`,
    or a sequence it accepts.  ``out``: an existing float32 [N] buffer on the device of ``means``, written in place and
    returned.  Three launches on the current stream, no read-back (``gsr_filter3d_sampling``).

    ValueError, before the library is entered: CPU tensors, wrong shapes or dtypes, no camera, ``variance <= 0``,
    ``near <= 0`` or ``margin < 0``."""
    op = "sampling_filter_3d"
    _require_cuda(means, op, "means")
    if not isinstance(cameras, Tensor):
        cameras = filter_cameras(cameras, means.device)
    _require_cuda(cameras, op, "cameras")
    if means.dim() != 2 or means.shape[1] != 3 or means.dtype != _f32:
        raise ValueError(f"{op}: means must be float32 [N,3], got {means.dtype} {tuple(means.shape)}")
    if cameras.dim() != 2 or cameras.shape[1] != CAMERA_STRIDE or cameras.dtype != _f32:
        raise ValueError(f"{op}: cameras must be float32 [V,{CAMERA_STRIDE}] (gs_fused.filter_cameras), got "
                         f"{cameras.dtype} {tuple(cameras.shape)}")
    if cameras.shape[0] < 1:
        raise ValueError(f"{op}: cameras holds no camera")
    if cameras.device != means.device:
        raise ValueError(f"{op}: cameras is on {cameras.device}, means on {means.device}")
    if not (float(variance) > 0.0 and float(near) > 0.0 and float(margin) >= 0.0):
        raise ValueError(f"{op}: need variance > 0, near > 0 and margin >= 0, got {variance}, {near}, {margin}")
    n, dev = means.shape[0], means.device
    if out is None:
        out = torch.empty(n, dtype=_f32, device=dev)
    elif (not isinstance(out, Tensor) or out.dtype != _f32 or tuple(out.shape) != (n,) or out.device != dev
          or not out.is_contiguous()):
        raise ValueError(f"{op}: out must be a contiguous float32 [{n}] tensor on {dev}")
    if n == 0:
        return out
    means, cameras = means.detach().contiguous(), cameras.contiguous()
    if cameras.data_ptr() % 16:
        cameras = cameras.clone()
    from rasterizer.cuda import _call, _stream

    k = float(np.float32(np.sqrt(np.float64(variance))))  # float32(sqrt(variance)), the constant of the rule
    with torch.cuda.device(dev):
        workspace = torch.empty(WORKSPACE_BYTES // 4, dtype=torch.int32, device=dev)
        _call("gsr_filter3d_sampling", n, means, cameras.shape[0], cameras, k, float(near), float(margin), out,
              workspace, _stream(dev))
    return out


class _ActivateFiltered(Function):
    """`gs_fused.activations._Activate` with the filter: the backward recomputes from the raw parameters (which are
    alive anyway), so the forward's outputs are not kept for it, only the unit quaternions."""

    @staticmethod
    def forward(ctx, means, log_scales, raw_quats, opacity_logits, campos, filter_3d):
        from rasterizer.cuda import _call, _check, _stream

        n = log_scales.shape[0]
        for t, nm in ((log_scales, "scales"), (raw_quats, "quats"), (opacity_logits, "opacities"),
                      (filter_3d, "filter_3d")):
            _check(t, nm, _f32)
        dev = log_scales.device
        want_dirs = campos is not None
        if want_dirs:
            _check(means, "means", _f32)
            _check(campos, "camera_position", _f32)
        with torch.cuda.device(dev):
            scales = torch.empty_like(log_scales)
            quats = torch.empty_like(raw_quats)
            opac = torch.empty_like(opacity_logits)
            dirs = torch.empty((n, 3), dtype=_f32, device=dev) if want_dirs else None
            _call("gsr_activate_filtered_forward", n, means if want_dirs else None, log_scales, raw_quats,
                  opacity_logits, campos if want_dirs else None, filter_3d, scales, quats, opac,
                  dirs if want_dirs else None, _stream(dev))
        ctx.save_for_backward(raw_quats, log_scales, quats, opacity_logits, filter_3d)
        ctx.set_materialize_grads(False)
        from rasterizer.ahead import announce_opacity

        announce_opacity(opac)  # the FILTERED opacity: what the projection that follows composites with
        if want_dirs:
            ctx.mark_non_differentiable(dirs)
            return scales, quats, opac, dirs
        return scales, quats, opac, None

    @staticmethod
    def backward(ctx, v_scales, v_quats, v_opac, _v_dirs):
        from rasterizer.cuda import _call, _check, _stream

        raw_quats, log_scales, quats, opacity_logits, filter_3d = ctx.saved_tensors
        n = log_scales.shape[0]
        dev = log_scales.device
        cot = [None if t is None else _check(t.contiguous(), nm, _f32)
               for t, nm in ((v_scales, "v_scales"), (v_quats, "v_quats"), (v_opac, "v_opacities"))]
        with torch.cuda.device(dev):
            g_s = torch.empty_like(log_scales)
            g_q = torch.empty_like(quats)
            g_o = torch.empty_like(opacity_logits)
            _call("gsr_activate_filtered_backward", n, raw_quats, log_scales, quats, opacity_logits, filter_3d, *cot,
                  g_s, g_q, g_o, _stream(dev))
        return None, g_s, g_q, g_o, None, None


def activate_gaussians_filtered(means: Optional[Tensor], log_scales: Tensor, raw_quats: Tensor,
                                opacity_logits: Tensor, camera_position: Optional[Tensor], filter_3d: Tensor
                                ) -> Tuple[Tensor, Tensor, Tensor, Optional[Tensor]]:
    """What `gs_fused.activate_gaussians` calls when it is given a filter (shapes are checked there)."""
    op = "activate_gaussians(filter_3d=...)"
    n = log_scales.shape[0]
    for t, nm in ((log_scales, "log_scales"), (raw_quats, "raw_quats"), (opacity_logits, "opacity_logits"),
                  (filter_3d, "filter_3d")):
        _require_cuda(t, op, nm)
    if filter_3d.dtype != _f32 or tuple(filter_3d.shape) != (n,):
        raise ValueError(f"{op}: filter_3d must be float32 [{n}], got {filter_3d.dtype} {tuple(filter_3d.shape)}")
    if filter_3d.device != log_scales.device:
        raise ValueError(f"{op}: filter_3d is on {filter_3d.device}, the parameters on {log_scales.device}")
    return _ActivateFiltered.apply(means.detach().contiguous() if camera_position is not None else None,
                                   log_scales.contiguous(), raw_quats.contiguous(), opacity_logits.contiguous(),
                                   camera_position.contiguous() if camera_position is not None else None,
                                   filter_3d.detach().contiguous())


def apply_filter_3d(scales: Tensor, opacities: Tensor, filter_3d: Tensor) -> Tuple[Tensor, Tensor]:
    """ACTIVATED scales [N,3] and opacities [N,1] or [N] -> (s', o') under the filter [N], as differentiable torch ops
    in the tensors' own dtype: ``s' = sqrt(s^2 + f^2)``, ``o' = o prod_k s_k / s'_k``.  No gradient reaches the
    filter.  For callers that keep their own activations (the toolkit's models do their own ``torch.exp``), and the
    statement of the rule the HIP kernels are held to.  Any device."""
    n = scales.shape[0]
    if scales.dim() != 2 or scales.shape[1] != 3 or opacities.numel() != n or tuple(filter_3d.shape) != (n,):
        raise ValueError(f"apply_filter_3d: expected scales [N,3], opacities [N,1] or [N] and filter_3d [N], got "
                         f"{tuple(scales.shape)}, {tuple(opacities.shape)}, {tuple(filter_3d.shape)}")
    f = filter_3d.detach().to(scales.dtype)[:, None]
    filtered = torch.sqrt(scales * scales + f * f)
    c = (scales / filtered).prod(dim=-1)
    return filtered, opacities * c.reshape(opacities.shape)


@torch.no_grad()
def bake_filter_3d(log_scales: Tensor, opacity_logits: Tensor, filter_3d: Tensor) -> Tuple[Tensor, Tensor]:
    """RAW log-scales [N,3] and opacity logits [N,1] or [N] -> ``(log s', logit(o c))``, computed in float64 and stored
    in the inputs' dtype: a model whose plain activations are the filtered activations of the given one (rendered
    without a filter it is the filtered model -- the interchange form, Mip-Splatting's fused PLY).  Any device."""
    n = log_scales.shape[0]
    if log_scales.dim() != 2 or log_scales.shape[1] != 3 or opacity_logits.numel() != n or \
            tuple(filter_3d.shape) != (n,):
        raise ValueError(f"bake_filter_3d: expected log_scales [N,3], opacity_logits [N,1] or [N] and filter_3d [N], "
                         f"got {tuple(log_scales.shape)}, {tuple(opacity_logits.shape)}, {tuple(filter_3d.shape)}")
    f64 = torch.float64
    l, a = log_scales.detach().to(f64), opacity_logits.detach().to(f64)
    f2 = (filter_3d.detach().to(device=l.device, dtype=f64) ** 2)[:, None]
    s2 = torch.exp(2.0 * l)
    log_filtered = 0.5 * torch.log(s2 + f2)
    # log c = sum_k (l_k - log s'_k);  logit(o c) = log(o c) - log(1 - o c), with log o = -softplus(-a)
    log_c = (l - log_filtered).sum(dim=-1).reshape(a.shape)
    log_oc = log_c - torch.nn.functional.softplus(-a)
    logit = log_oc - torch.log(-torch.expm1(log_oc))
    zero = (filter_3d.detach() == 0).to(l.device)
    log_filtered = torch.where(zero[:, None], l, log_filtered)
    logit = torch.where(zero.reshape(a.shape), a, logit)
    return log_filtered.to(log_scales.dtype), logit.to(opacity_logits.dtype)


__all__ = ["CAMERA_STRIDE", "filter_cameras", "sampling_filter_3d", "activate_gaussians_filtered", "apply_filter_3d",
           "bake_filter_3d"]
