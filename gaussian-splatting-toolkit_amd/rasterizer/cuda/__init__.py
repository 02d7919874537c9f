"""``rasterizer.cuda`` -- the native module of the rasterizer, MI355X edition.

The reference exposes an 11-function pybind module under this name
(``rasterizer/cuda/csrc/ext.cpp:6-17``; every Python module of the package does
``import rasterizer.cuda as _C``).  The module name is kept so that those
imports keep working; the implementation is hand-written HIP for gfx950 behind
the C ABI of ``include/gsraster.h``, bound here with ctypes.  Each function has
the reference's name, argument order, returned tuple order, dtypes, shapes and
error type (``RuntimeError`` for what ``TORCH_CHECK``/``AT_ERROR`` raise there).

PyTorch is used for device memory and streams only: outputs are allocated with
``torch.empty`` on the inputs' device (the kernels write every element, so the
reference's ``torch::zeros`` pre-fill is not needed) and kernels are enqueued
on the *current* HIP stream of that device.  There is no CPU path.
"""
import ctypes as C
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _tuning
from ._backend import lib as _lib, typed as _typed

_f32, _i32, _i64 = torch.float32, torch.int32, torch.int64


def _check(t: Tensor, name: str, dtype=None) -> Tensor:
    # CHECK_INPUT of the reference (bindings.h:10-15)
    if not isinstance(t, Tensor):
        raise RuntimeError(f"{name} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"{name} must have dtype {dtype}, got {t.dtype}")
    return t


def _ptr(t: Tensor) -> C.c_void_p:
    """(for callers of the raw handle `_backend.lib()`, which marshal for themselves; `_call` takes the tensor)"""
    return C.c_void_p(t.data_ptr())


class _Already:
    """(no-op context: the tensors' device is the current one already)"""

    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_ALREADY = _Already()


def _on(dev):
    """`torch.cuda.device(dev)` -- allocations and launches go to the inputs' device -- without the context
    manager's ~3 us when that device is current already (a dozen wrappers per view)."""
    idx = dev.index
    return _ALREADY if (idx is None or idx == torch.cuda.current_device()) else torch.cuda.device(dev)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(device) -> C.c_void_p:
    """The device's current stream as the C ABI takes it (the raw handle where torch hands it out directly: the
    `torch.cuda.Stream` object of `current_stream()` costs ~5 us, and every wrapper asks)."""
    idx = device.index
    if _raw_stream is not None and idx is not None:
        return C.c_void_p(_raw_stream(idx))
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _call(fn_name: str, *args) -> None:
    """One native entry through the typed handle (`_backend.typed`): `args` are the header's parameters as plain
    values -- a tensor, None or an address for a pointer, Python numbers for the scalars; values already wrapped in
    the parameter's own ctypes type pass as they are.  A wrong count or kind raises before the library is entered."""
    rc = getattr(_typed(), fn_name)(*args)
    if rc != 0:
        raise RuntimeError(f"{fn_name} failed ({rc}): {_lib().gsr_last_error().decode()}")


def _cf(v) -> C.c_float:
    """(as `_ptr`: for callers of the raw handle)"""
    return C.c_float(float(v))


def project_gaussians_forward(
    num_points: int, means3d: Tensor, scales: Optional[Tensor], glob_scale: float, quats: Optional[Tensor],
    viewmat: Tensor, projmat: Tensor, fx: float, fy: float, cx: float, cy: float,
    img_height: int, img_width: int, block_width: int, clip_thresh: float,
    cov3d_precomp: Optional[Tensor] = None,
) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (cov3d, xys, depths, radii, conics, compensation, num_tiles_hit);
    replaces ``project_gaussians_forward_tensor`` (bindings.cu:107-160).
    ``cov3d_precomp`` [N,6] (with ``scales`` = ``quats`` = None): covariances handed in
    instead of being built from scales and rotations; returned as ``cov3d``."""
    precomp = cov3d_precomp is not None
    if precomp != (scales is None) or precomp != (quats is None):
        raise RuntimeError("pass either scales and quats, or cov3d_precomp")
    for t, nm in ((means3d, "means3d"), (viewmat, "viewmat"), (projmat, "projmat")) + (
            ((cov3d_precomp, "cov3d_precomp"),) if precomp else ((scales, "scales"), (quats, "quats"))):
        _check(t, nm, _f32)
    n = int(num_points)
    if viewmat.numel() < 12 or projmat.numel() != 16:
        raise RuntimeError("viewmat must hold at least 3x4 and projmat 4x4 values")
    if means3d.numel() != 3 * n or (not precomp and (scales.numel() != 3 * n or quats.numel() != 4 * n)) \
            or (precomp and cov3d_precomp.numel() != 6 * n):
        raise RuntimeError("means3d/scales/quats do not match num_points")
    dev = means3d.device
    with _on(dev):
        # seven outputs, seven allocations (the caching allocator hands each out in ~1 us): in round 4 they were carved
        # out of ONE allocation, which made them views sharing a storage and a version counter (a caller's
        # in-place op on one invalidated the others that autograd had saved, and keeping `radii` alive pinned all 15
        # words per Gaussian); independent tensors over a shared storage (`set_`) cost 3 us apiece -- more than this
        e = lambda shape, dt=_f32: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
        xys, depths, conics, compensation = e((n, 2)), e((n,)), e((n, 3)), e((n,))
        radii, num_tiles_hit = e((n,), _i32), e((n,), _i32)
        cov3d = cov3d_precomp if precomp else e((n, 6))
        _call("gsr_project_forward", n, means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy,
              img_height, img_width, block_width, clip_thresh, cov3d, xys, depths, radii, conics, compensation,
              num_tiles_hit, _stream(dev))
    return cov3d, xys, depths, radii, conics, compensation, num_tiles_hit


def project_gaussians_backward(
    num_points: int, means3d: Tensor, scales: Tensor, glob_scale: float, quats: Tensor,
    viewmat: Tensor, projmat: Tensor, fx: float, fy: float, cx: float, cy: float,
    img_height: int, img_width: int, cov3d: Tensor, radii: Tensor, conics: Tensor,
    compensation: Tensor, v_xy: Tensor, v_depth: Tensor, v_conic: Tensor, v_compensation: Tensor,
    trusted: bool = False,
) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (v_cov2d, v_cov3d, v_mean3d, v_scale, v_quat);
    replaces ``project_gaussians_backward_tensor`` (bindings.cu:164-216).  ``trusted``: the first sixteen arguments
    are the tensors a forward call of this module validated and produced (what the autograd node passes back): only
    the cotangents are checked."""
    n = int(num_points)
    dev = means3d.device
    precomp = scales is None and quats is None  # covariances were handed in: the chain ends at v_cov3d
    if not trusted:
        for t, nm in ((means3d, "means3d"), (viewmat, "viewmat"),
                      (projmat, "projmat"), (cov3d, "cov3d"), (conics, "conics"),
                      (compensation, "compensation")) + (() if precomp else ((scales, "scales"), (quats, "quats"))):
            _check(t, nm, _f32)
        _check(radii, "radii", _i32)
    # cotangents may arrive non-contiguous / expanded from autograd; None = zero
    v_xy, v_depth, v_conic, v_compensation = (
        None if t is None else _check(t.contiguous(), nm, _f32)
        for t, nm in ((v_xy, "v_xy"), (v_depth, "v_depth"), (v_conic, "v_conic"),
                      (v_compensation, "v_compensation"))
    )
    with _on(dev):
        e = lambda shape: torch.empty(shape, dtype=_f32, device=dev)  # noqa: E731
        v_cov2d, v_cov3d, v_mean3d = e((n, 3)), e((n, 6)), e((n, 3))
        v_scale = None if precomp else e((n, 3))
        v_quat = None if precomp else e((n, 4))
        _call("gsr_project_backward", n, means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy,
              img_height, img_width, cov3d, radii, conics, compensation, v_xy, v_depth, v_conic, v_compensation,
              v_cov2d, v_cov3d, v_mean3d, v_scale, v_quat, _stream(dev))
    return v_cov2d, v_cov3d, v_mean3d, v_scale, v_quat


def project_gaussians_forward_aa(
    num_points: int, means3d: Tensor, scales: Tensor, glob_scale: float, quats: Tensor,
    viewmat: Tensor, projmat: Tensor, fx: float, fy: float, cx: float, cy: float,
    img_height: int, img_width: int, block_width: int, clip_thresh: float, opacities: Tensor,
) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (cov3d, xys, depths, radii, conics, compensation, num_tiles_hit, opacities_aa): ``project_gaussians_forward``
    plus ``opacities_aa = opacities * compensation`` (one float32 multiply in the projection kernel: the opacity the
    antialiased rasterize mode composites, vanilla_gs.py:815-816), in the shape of ``opacities`` ([N] or [N,1])."""
    for t, nm in ((means3d, "means3d"), (scales, "scales"), (quats, "quats"), (viewmat, "viewmat"),
                  (projmat, "projmat"), (opacities, "opacities")):
        _check(t, nm, _f32)
    n = int(num_points)
    if viewmat.numel() < 12 or projmat.numel() != 16:
        raise RuntimeError("viewmat must hold at least 3x4 and projmat 4x4 values")
    if means3d.numel() != 3 * n or scales.numel() != 3 * n or quats.numel() != 4 * n or opacities.numel() != n:
        raise RuntimeError("means3d/scales/quats/opacities do not match num_points")
    dev = means3d.device
    with _on(dev):
        e = lambda shape, dt=_f32: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
        xys, depths, conics, compensation, cov3d = e((n, 2)), e((n,)), e((n, 3)), e((n,)), e((n, 6))
        radii, num_tiles_hit = e((n,), _i32), e((n,), _i32)
        opacities_aa = e(tuple(opacities.shape))
        _call("gsr_project_forward_aa", n, means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy,
              img_height, img_width, block_width, clip_thresh, opacities, cov3d, xys, depths, radii, conics,
              compensation, num_tiles_hit, opacities_aa, _stream(dev))
    return cov3d, xys, depths, radii, conics, compensation, num_tiles_hit, opacities_aa


def _check_crop(crop: Tensor, dev) -> Tensor:
    _check(crop, "crop", _f32)
    if crop.numel() != 16 or crop.device != dev:
        raise RuntimeError("crop must hold 16 float32 values (gs_fused.CropBox.tensor) on the device of means3d")
    return crop


def project_gaussians_forward_crop(
    num_points: int, means3d: Tensor, scales: Tensor, glob_scale: float, quats: Tensor,
    viewmat: Tensor, projmat: Tensor, fx: float, fy: float, cx: float, cy: float,
    img_height: int, img_width: int, block_width: int, clip_thresh: float, crop: Tensor,
    opacities: Optional[Tensor] = None,
):
    """-> (cov3d, xys, depths, radii, conics, compensation, num_tiles_hit, opacities_aa or None):
    ``project_gaussians_forward`` (with ``opacities``: ``project_gaussians_forward_aa``) for the Gaussians whose
    centre is inside the oriented crop box ``crop`` (float32[16] on the device: the world->box matrix 3x4 and the
    half extents, include/gsraster.h); a Gaussian outside it comes back as a culled one, zeros everywhere."""
    for t, nm in ((means3d, "means3d"), (scales, "scales"), (quats, "quats"), (viewmat, "viewmat"),
                  (projmat, "projmat")) + (() if opacities is None else ((opacities, "opacities"),)):
        _check(t, nm, _f32)
    n = int(num_points)
    dev = means3d.device
    _check_crop(crop, dev)
    if viewmat.numel() < 12 or projmat.numel() != 16:
        raise RuntimeError("viewmat must hold at least 3x4 and projmat 4x4 values")
    if means3d.numel() != 3 * n or scales.numel() != 3 * n or quats.numel() != 4 * n \
            or (opacities is not None and opacities.numel() != n):
        raise RuntimeError("means3d/scales/quats/opacities do not match num_points")
    with _on(dev):
        e = lambda shape, dt=_f32: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
        xys, depths, conics, compensation, cov3d = e((n, 2)), e((n,)), e((n, 3)), e((n,)), e((n, 6))
        radii, num_tiles_hit = e((n,), _i32), e((n,), _i32)
        opacities_aa = None if opacities is None else e(tuple(opacities.shape))
        _call("gsr_project_forward_crop", n, means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy,
              img_height, img_width, block_width, clip_thresh, crop, opacities, cov3d, xys, depths, radii, conics,
              compensation, num_tiles_hit, opacities_aa, _stream(dev))
    return cov3d, xys, depths, radii, conics, compensation, num_tiles_hit, opacities_aa


def crop_mask(means3d: Tensor, crop: Tensor, want_count: bool = True) -> Tuple[Tensor, Optional[Tensor]]:
    """-> (mask uint8[N], count int32[1] on the device or None): which centres the crop box keeps, by the device
    function the cropped projection uses (``gsr_crop_mask``).  Nothing is read back."""
    _check(means3d, "means3d", _f32)
    if means3d.dim() != 2 or means3d.shape[1] != 3:
        raise RuntimeError("means3d [N,3] expected")
    dev = means3d.device
    _check_crop(crop, dev)
    n = means3d.shape[0]
    with _on(dev):
        mask = torch.empty((n,), dtype=torch.uint8, device=dev)
        count = torch.empty((1,), dtype=_i32, device=dev) if want_count else None
        _call("gsr_crop_mask", n, means3d, crop, mask, count, _stream(dev))
    return mask, count


def project_gaussians_backward_aa(
    num_points: int, means3d: Tensor, scales: Tensor, glob_scale: float, quats: Tensor,
    viewmat: Tensor, projmat: Tensor, fx: float, fy: float, cx: float, cy: float,
    img_height: int, img_width: int, cov3d: Tensor, radii: Tensor, conics: Tensor,
    compensation: Tensor, opacities: Tensor, v_xy: Optional[Tensor], v_depth: Optional[Tensor],
    v_conic: Optional[Tensor], v_compensation: Optional[Tensor], v_opacities_aa: Optional[Tensor],
    in_place: bool = False, want_v_compensation: bool = False, trusted: bool = False,
):
    """-> (v_cov2d, v_cov3d, v_mean3d, v_scale, v_quat, v_opacities, v_compensation_out or None):
    ``project_gaussians_backward`` plus the product's two cotangents.  ``v_opacities = v_opacities_aa * compensation``
    (``in_place``: written over ``v_opacities_aa``, which is returned); the compensation's cotangent inside the chain
    is ``v_compensation + v_opacities_aa * opacities`` (float32), returned when ``want_v_compensation`` -- what
    ``project_gaussians_backward_pose`` takes as its ``v_compensation``.  A cotangent that is None is zero."""
    n = int(num_points)
    dev = means3d.device
    if not trusted:
        for t, nm in ((means3d, "means3d"), (scales, "scales"), (quats, "quats"), (viewmat, "viewmat"),
                      (projmat, "projmat"), (cov3d, "cov3d"), (conics, "conics"), (compensation, "compensation"),
                      (opacities, "opacities")):
            _check(t, nm, _f32)
        _check(radii, "radii", _i32)
        if opacities.numel() != n or compensation.numel() != n:
            raise RuntimeError("opacities/compensation do not match num_points")
    v_xy, v_depth, v_conic, v_compensation = (
        None if t is None else _check(t.contiguous(), nm, _f32)
        for t, nm in ((v_xy, "v_xy"), (v_depth, "v_depth"), (v_conic, "v_conic"),
                      (v_compensation, "v_compensation"))
    )
    with _on(dev):
        e = lambda shape: torch.empty(shape, dtype=_f32, device=dev)  # noqa: E731
        if v_opacities_aa is None:
            v_opacities_aa = torch.zeros(tuple(opacities.shape), dtype=_f32, device=dev)
            in_place = True
        elif in_place:
            _check(v_opacities_aa, "v_opacities_aa", _f32)
        else:
            v_opacities_aa = _check(v_opacities_aa.contiguous(), "v_opacities_aa", _f32)
        if v_opacities_aa.numel() != n:
            raise RuntimeError("v_opacities_aa does not match num_points")
        v_cov2d, v_cov3d, v_mean3d, v_scale, v_quat = e((n, 3)), e((n, 6)), e((n, 3)), e((n, 3)), e((n, 4))
        v_opacities = v_opacities_aa if in_place else e(tuple(opacities.shape))
        v_comp_out = e((n,)) if want_v_compensation else None
        _call("gsr_project_backward_aa", n, means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy,
              img_height, img_width, cov3d, radii, conics, compensation, opacities, v_xy, v_depth, v_conic,
              v_compensation, v_opacities_aa, v_cov2d, v_cov3d, v_mean3d, v_scale, v_quat, v_opacities, v_comp_out,
              _stream(dev))
    return v_cov2d, v_cov3d, v_mean3d, v_scale, v_quat, v_opacities, v_comp_out


def project_gaussians_forward_fisheye(
    num_points: int, means3d: Tensor, scales: Optional[Tensor], glob_scale: float, quats: Optional[Tensor],
    viewmat: Tensor, projmat: Tensor, fx: float, fy: float, cx: float, cy: float,
    img_height: int, img_width: int, block_width: int, clip_thresh: float,
    opacities: Optional[Tensor] = None, cov3d_precomp: Optional[Tensor] = None,
):
    """-> (cov3d, xys, depths, radii, conics, compensation, num_tiles_hit, opacities_aa or None): the outputs of
    ``project_gaussians_forward`` (with ``opacities``: of ``project_gaussians_forward_aa``) through the equidistant
    fisheye camera (``gsr_project_forward_fisheye``, include/gsraster.h).  ``projmat`` is checked like the
    pinhole entry's and not read."""
    precomp = cov3d_precomp is not None
    if precomp != (scales is None) or precomp != (quats is None):
        raise RuntimeError("pass either scales and quats, or cov3d_precomp")
    for t, nm in ((means3d, "means3d"), (viewmat, "viewmat"), (projmat, "projmat")) + (
            ((cov3d_precomp, "cov3d_precomp"),) if precomp else ((scales, "scales"), (quats, "quats"))) + (
            () if opacities is None else ((opacities, "opacities"),)):
        _check(t, nm, _f32)
    n = int(num_points)
    if viewmat.numel() < 12 or projmat.numel() != 16:
        raise RuntimeError("viewmat must hold at least 3x4 and projmat 4x4 values")
    if means3d.numel() != 3 * n or (not precomp and (scales.numel() != 3 * n or quats.numel() != 4 * n)) \
            or (precomp and cov3d_precomp.numel() != 6 * n) or (opacities is not None and opacities.numel() != n):
        raise RuntimeError("means3d/scales/quats/opacities do not match num_points")
    dev = means3d.device
    with _on(dev):
        e = lambda shape, dt=_f32: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
        xys, depths, conics, compensation = e((n, 2)), e((n,)), e((n, 3)), e((n,))
        radii, num_tiles_hit = e((n,), _i32), e((n,), _i32)
        cov3d = cov3d_precomp if precomp else e((n, 6))
        opacities_aa = None if opacities is None else e(tuple(opacities.shape))
        _call("gsr_project_forward_fisheye", n, means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy,
              img_height, img_width, block_width, clip_thresh, opacities, cov3d, xys, depths, radii, conics,
              compensation, num_tiles_hit, opacities_aa, _stream(dev))
    return cov3d, xys, depths, radii, conics, compensation, num_tiles_hit, opacities_aa


def project_gaussians_backward_fisheye(
    num_points: int, means3d: Tensor, scales: Optional[Tensor], glob_scale: float, quats: Optional[Tensor],
    viewmat: Tensor, projmat: Tensor, fx: float, fy: float, cx: float, cy: float,
    img_height: int, img_width: int, cov3d: Tensor, radii: Tensor, conics: Tensor,
    compensation: Tensor, opacities: Optional[Tensor], v_xy: Optional[Tensor], v_depth: Optional[Tensor],
    v_conic: Optional[Tensor], v_compensation: Optional[Tensor], v_opacities_aa: Optional[Tensor] = None,
    trusted: bool = False,
):
    """-> (v_cov2d, v_cov3d, v_mean3d, v_scale, v_quat, v_opacities or None): ``project_gaussians_backward`` (with
    ``opacities``: ``project_gaussians_backward_aa``) through the equidistant fisheye camera.  A cotangent that is
    None is zero; ``scales`` = ``quats`` = None: the covariances were handed in and the chain ends at v_cov3d."""
    n = int(num_points)
    dev = means3d.device
    precomp = scales is None and quats is None
    if not trusted:
        for t, nm in ((means3d, "means3d"), (viewmat, "viewmat"), (projmat, "projmat"), (cov3d, "cov3d"),
                      (conics, "conics"), (compensation, "compensation")) + (
                () if precomp else ((scales, "scales"), (quats, "quats"))) + (
                () if opacities is None else ((opacities, "opacities"),)):
            _check(t, nm, _f32)
        _check(radii, "radii", _i32)
        if compensation.numel() != n or (opacities is not None and opacities.numel() != n):
            raise RuntimeError("opacities/compensation do not match num_points")
    v_xy, v_depth, v_conic, v_compensation = (
        None if t is None else _check(t.contiguous(), nm, _f32)
        for t, nm in ((v_xy, "v_xy"), (v_depth, "v_depth"), (v_conic, "v_conic"),
                      (v_compensation, "v_compensation"))
    )
    with _on(dev):
        e = lambda shape: torch.empty(shape, dtype=_f32, device=dev)  # noqa: E731
        v_opacities = None
        if opacities is None:
            if v_opacities_aa is not None:
                raise RuntimeError("v_opacities_aa without opacities")
        else:
            if v_opacities_aa is None:
                v_opacities_aa = torch.zeros(tuple(opacities.shape), dtype=_f32, device=dev)
            else:
                v_opacities_aa = _check(v_opacities_aa.contiguous(), "v_opacities_aa", _f32)
            if v_opacities_aa.numel() != n:
                raise RuntimeError("v_opacities_aa does not match num_points")
            v_opacities = e(tuple(opacities.shape))
        v_cov2d, v_cov3d, v_mean3d = e((n, 3)), e((n, 6)), e((n, 3))
        v_scale = None if precomp else e((n, 3))
        v_quat = None if precomp else e((n, 4))
        _call("gsr_project_backward_fisheye", n, means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy,
              img_height, img_width, cov3d, radii, conics, compensation, opacities, v_xy, v_depth, v_conic,
              v_compensation, v_opacities_aa, v_cov2d, v_cov3d, v_mean3d, v_scale, v_quat, v_opacities, None,
              _stream(dev))
    return v_cov2d, v_cov3d, v_mean3d, v_scale, v_quat, v_opacities


def project_gaussians_backward_pose(
    num_points: int, means3d: Tensor, viewmat: Tensor, projmat: Tensor, fx: float, fy: float,
    img_height: int, img_width: int, cov3d: Tensor, radii: Tensor, conics: Tensor, compensation: Tensor,
    v_xy: Optional[Tensor], v_depth: Optional[Tensor], v_conic: Optional[Tensor], v_compensation: Optional[Tensor],
    trusted: bool = False,
) -> Tuple[Tensor, Tensor]:
    """-> (v_viewmat [3,4], v_projmat [4,4]): the camera's gradient through the projection, which the reference does
    not have (its backward returns None for both matrices, project_gaussians.py:156-232).  The sums over the visible
    Gaussians of the terms ``project_gaussians_backward`` forms per Gaussian, under its conventions: no fov clamp (so
    outside the 1.3x guard band this is not the forward's derivative, as for ``v_mean3d``), the compensation's
    cotangent scaled by ``0.5 / (compensation + 1e-6)``, a cotangent that is None is zero.  Row 2 of ``v_projmat`` is
    exactly zero.  The colour's view dependence contributes nothing: the SH op has no gradient with respect to
    ``viewdirs``, in the reference or here.  Reads ``cov3d``, never scales or quats.  Float64 sums in a fixed order:
    two calls give the same bits.  ``trusted`` as in ``project_gaussians_backward``."""
    n = int(num_points)
    dev = means3d.device
    if not trusted:
        for t, nm in ((means3d, "means3d"), (viewmat, "viewmat"), (projmat, "projmat"), (cov3d, "cov3d"),
                      (conics, "conics"), (compensation, "compensation")):
            _check(t, nm, _f32)
        _check(radii, "radii", _i32)
        if viewmat.numel() < 12 or projmat.numel() != 16:
            raise RuntimeError("viewmat must hold at least 3x4 and projmat 4x4 values")
        if means3d.numel() != 3 * n or cov3d.numel() != 6 * n or radii.numel() != n or conics.numel() != 3 * n \
                or compensation.numel() != n:
            raise RuntimeError("means3d/cov3d/radii/conics/compensation do not match num_points")
    cots = []
    for t, nm, width in ((v_xy, "v_xy", 2), (v_depth, "v_depth", 1), (v_conic, "v_conic", 3),
                         (v_compensation, "v_compensation", 1)):
        if t is not None:
            t = _check(t.contiguous(), nm, _f32)
            if t.numel() != width * n:
                raise RuntimeError(f"{nm} does not match num_points")
        cots.append(t)
    with _on(dev):
        nbytes = int(_typed().gsr_project_backward_pose_workspace(n))
        workspace = torch.empty((max(nbytes, 8) // 8,), dtype=torch.float64, device=dev)
        v_viewmat = torch.empty((3, 4), dtype=_f32, device=dev)
        v_projmat = torch.empty((4, 4), dtype=_f32, device=dev)
        _call("gsr_project_backward_pose", n, means3d, viewmat, projmat, fx, fy, img_height, img_width, cov3d, radii,
              conics, compensation, *cots, workspace, nbytes, v_viewmat, v_projmat, _stream(dev))
    return v_viewmat, v_projmat


def _num_sh_bases(degree: int) -> int:
    return {0: 1, 1: 4, 2: 9, 3: 16}.get(int(degree), 25)


SH_SHARE_CU, SH_NARROW = 1, 2  # GSR_SH_SHARE_CU, GSR_SH_NARROW (include/gsraster.h)


def compute_sh_forward(num_points: int, degree: int, degrees_to_use: int, viewdirs: Tensor,
                       coeffs: Tensor, flags: int = 0) -> Tensor:
    """-> colors [N,3]; replaces ``compute_sh_forward_tensor`` (bindings.cu:58-77).  ``flags``: ``SH_SHARE_CU`` [``|
    SH_NARROW``], the kernel that runs beside kernels of another stream (include/gsraster.h): the same bits."""
    n = int(num_points)
    if coeffs.dim() != 3 or coeffs.size(0) != n or coeffs.size(1) != _num_sh_bases(degree) \
            or coeffs.size(2) != 3:
        raise RuntimeError("coeffs must have dimensions (N, D, 3)")
    _check(viewdirs, "viewdirs", _f32)
    _check(coeffs, "coeffs", _f32)
    dev = coeffs.device
    with _on(dev):
        colors = torch.empty((n, 3), dtype=_f32, device=dev)
        if flags:
            _call("gsr_sh_forward_flags", n, degree, degrees_to_use, viewdirs, coeffs, colors, int(flags), _stream(dev))
        else:
            _call("gsr_sh_forward", n, degree, degrees_to_use, viewdirs, coeffs, colors, _stream(dev))
    return colors


def compute_sh_backward(num_points: int, degree: int, degrees_to_use: int, viewdirs: Tensor,
                        v_colors: Tensor, trusted: bool = False) -> Tensor:
    """-> v_coeffs [N,K,3]; replaces ``compute_sh_backward_tensor`` (bindings.cu:79-103)."""
    n = int(num_points)
    if viewdirs.dim() != 2 or viewdirs.size(0) != n or viewdirs.size(1) != 3:
        raise RuntimeError("viewdirs must have dimensions (N, 3)")
    if v_colors.dim() != 2 or v_colors.size(0) != n or v_colors.size(1) != 3:
        raise RuntimeError("v_colors must have dimensions (N, 3)")
    if not trusted:  # (trusted: `viewdirs` is the tensor the forward call validated)
        _check(viewdirs, "viewdirs", _f32)
    v_colors = _check(v_colors.contiguous(), "v_colors", _f32)
    dev = viewdirs.device
    with _on(dev):
        v_coeffs = torch.empty((n, _num_sh_bases(degree), 3), dtype=_f32, device=dev)
        _call("gsr_sh_backward", n, degree, degrees_to_use, viewdirs, v_colors, v_coeffs, _stream(dev))
    return v_coeffs


def cumsum_tiles(num_tiles_hit: Tensor) -> Tensor:
    """Inclusive int32 scan (not part of the reference's native module, which
    uses ``torch.cumsum``; exported for ``utils.compute_cumulative_intersects``)."""
    _check(num_tiles_hit, "num_tiles_hit", _i32)
    n = num_tiles_hit.numel()
    dev = num_tiles_hit.device
    with _on(dev):
        cum = torch.empty_like(num_tiles_hit)
        nbytes = int(_typed().gsr_cumsum_workspace_bytes(n))
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
        _call("gsr_cumsum_tiles", n, num_tiles_hit, cum, ws, nbytes, _stream(dev))
    return cum


def map_gaussian_to_intersects(
    num_points: int, num_intersects: int, xys: Tensor, depths: Tensor, radii: Tensor,
    cum_tiles_hit: Tensor, tile_bounds: Tuple[int, int, int], block_width: int,
) -> Tuple[Tensor, Tensor]:
    """-> (isect_ids i64[I], gaussian_ids i32[I]);
    replaces ``map_gaussian_to_intersects_tensor`` (bindings.cu:218-251)."""
    _check(xys, "xys", _f32)
    _check(depths, "depths", _f32)
    _check(radii, "radii", _i32)
    _check(cum_tiles_hit, "cum_tiles_hit", _i32)
    dev = xys.device
    I = int(num_intersects)
    with _on(dev):
        # zero-filled like the reference: slots not claimed by any splat stay 0
        isect_ids = torch.zeros((I,), dtype=_i64, device=dev)
        gaussian_ids = torch.zeros((I,), dtype=_i32, device=dev)
        _call("gsr_map_intersects", int(num_points), I, xys, depths, radii, cum_tiles_hit, tile_bounds[0],
              tile_bounds[1], block_width, isect_ids, gaussian_ids, _stream(dev))
    return isect_ids, gaussian_ids


def sort_intersects(isect_ids: Tensor, gaussian_ids: Tensor, num_tiles: int) -> Tuple[Tensor, Tensor]:
    """Stable radix sort of the (tile|depth) keys with their Gaussian ids (the
    reference's ``torch.sort`` + ``torch.gather``, utils.py:179-180)."""
    _check(isect_ids, "isect_ids", _i64)
    _check(gaussian_ids, "gaussian_ids", _i32)
    I = isect_ids.numel()
    dev = isect_ids.device
    with _on(dev):
        keys = torch.empty_like(isect_ids)
        vals = torch.empty_like(gaussian_ids)
        nbytes = int(_typed().gsr_sort_workspace_bytes(I))
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
        _call("gsr_sort_intersects", I, max(int(num_tiles), 1), isect_ids, gaussian_ids, keys, vals, ws, nbytes,
              _stream(dev))
    return keys, vals


def get_tile_bin_edges(num_intersects: int, isect_ids_sorted: Tensor,
                       tile_bounds: Tuple[int, int, int]) -> Tensor:
    """-> tile_bins i32[T,2]; replaces ``get_tile_bin_edges_tensor`` (bindings.cu:253-267)."""
    _check(isect_ids_sorted, "isect_ids_sorted", _i64)
    dev = isect_ids_sorted.device
    nt = int(tile_bounds[0]) * int(tile_bounds[1])
    with _on(dev):
        tile_bins = alloc_tile_bins(tile_bounds, dev)
        _call("gsr_tile_bin_edges", int(num_intersects), isect_ids_sorted, nt, tile_bins, _stream(dev))
    return tile_bins


def depth_order(depths: Tensor, radii: Tensor, num_tiles_hit: Optional[Tensor]) -> Tuple[Tensor, Optional[Tensor]]:
    """First half of the fused binning pipeline (``gsr_depth_order``):
    -> (order i32[N], cum_sorted i32[B*N]); ``cum_sorted[-1]`` is the number of
    intersections.  ``num_tiles_hit`` is [N], or the band-major [B*N] counts of
    :func:`count_reach` on a tile grid of B = :func:`tile_bands` bands, or None: the
    order only, ``cum_sorted`` is None (lists without counts, :func:`lists_need_counts`)."""
    _check(depths, "depths", _f32)
    _check(radii, "radii", _i32)
    n = depths.numel()
    bands = 1
    if num_tiles_hit is not None:
        _check(num_tiles_hit, "num_tiles_hit", _i32)
        bands = num_tiles_hit.numel() // n if n else 1
        if n and (num_tiles_hit.numel() != bands * n or bands < 1):
            raise RuntimeError("depth_order: num_tiles_hit must hold N (or bands * N) counts")
    dev = depths.device
    with _on(dev):
        order = torch.empty((n,), dtype=_i32, device=dev)
        cum = torch.empty((bands * n,), dtype=_i32, device=dev) if num_tiles_hit is not None else None
        nbytes = int(_typed().gsr_depth_order_workspace_bytes(n, bands))
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
        _call("gsr_depth_order", n, depths, radii, num_tiles_hit, bands, order, cum, ws, nbytes, _stream(dev))
    return order, cum


def lists_need_counts(num_points: int, num_intersects: int, tile_bounds: Tuple[int, int, int],
                      device_sized: bool = True, want_slots: bool = False) -> bool:
    """``gsr_bin_sorted_needs_counts``: False when :func:`bin_sorted` (exact lists, one
    band) will take the two-level partition for these sizes -- the caller may then skip
    the counts: ``count_reach(..., counts=False)``, ``depth_order(depths, radii, None)``,
    ``bin_sorted(..., cum_sorted=None)``."""
    return bool(_typed().gsr_bin_sorted_needs_counts(int(num_points), int(num_intersects), tile_bounds[0], tile_bounds[1],
                                                   1 if device_sized else 0, 1 if want_slots else 0))


def tile_bands(tile_bounds: Tuple[int, int, int]) -> int:
    """``gsr_tile_bands``: 1 up to 16384 tiles; above, the number of tile-row bands the
    fused binning works in (4K at 16 px: 4)."""
    return int(_typed().gsr_tile_bands(tile_bounds[0], tile_bounds[1]))


def publish_int32(src: Tensor, dst: Tensor) -> None:
    """``gsr_publish_int32``: ``dst[0] = src[0]`` by a one-thread kernel in stream order;
    ``dst`` may be pinned host memory (int32)."""
    _check(src, "src", _i32)
    if dst.dtype != _i32 or dst.numel() < 1:
        raise RuntimeError("publish_int32: dst must be int32")
    dev = src.device
    with _on(dev):
        _call("gsr_publish_int32", src, dst, _stream(dev))


def count_reach(xys: Tensor, radii: Tensor, conics: Tensor, opacities: Tensor,
                tile_bounds: Tuple[int, int, int], bands: int = 1, counts: bool = True,
                extra_rows: int = 0) -> Tuple[Optional[Tensor], Tensor]:
    """``gsr_count_reach``: per Gaussian, the number of 16x16 tiles of its bounding
    box in which it can reach alpha >= 1/255 -> (counts i32[bands*N], band-major, summing to
    <= num_tiles_hit per Gaussian; opaque per-Gaussian records for :func:`bin_sorted`).
    ``bands``: 1 (default: one count per Gaussian; large grids then take the two-level
    partition) or :func:`tile_bands` (tile-row bands: needed for ``want_slots``).
    ``counts=False``: the records only (-> (None, records)), see :func:`lists_need_counts`."""
    _check(xys, "xys", _f32)
    _check(radii, "radii", _i32)
    _check(conics, "conics", _f32)
    _check(opacities, "opacities", _f32)
    n = radii.numel()
    if xys.numel() != 2 * n or conics.numel() != 3 * n or opacities.numel() != n:
        raise RuntimeError("count_reach: xys [N,2], conics [N,3], opacities [N,1] expected")
    dev = xys.device
    with _on(dev):
        cnt = torch.empty((int(bands) * n,), dtype=_i32, device=dev) if counts else None
        recs = torch.empty((n + int(extra_rows), int(_typed().gsr_reach_record_bytes())), dtype=torch.uint8, device=dev)
        if extra_rows:
            recs[n:].zero_()  # all-zero records are culled ones (empty tile box): `saturation_filter`'s dummy
        _call("gsr_count_reach", n, xys, radii, conics, opacities, tile_bounds[0], tile_bounds[1], int(bands), cnt,
              recs, _stream(dev))
    return cnt, recs


def reach_records_depth_order(xys: Tensor, radii: Tensor, conics: Tensor, opacities: Tensor, depths: Tensor,
                              tile_bounds: Tuple[int, int, int], extra_rows: int = 0) -> Tuple[Tensor, Tensor]:
    """``gsr_reach_records_depth_order``: ``count_reach(..., counts=False)`` and ``depth_order(depths, radii, None)``
    as one call -> (records, order), the same values (lists without counts, :func:`lists_need_counts`)."""
    _check(xys, "xys", _f32)
    _check(radii, "radii", _i32)
    _check(conics, "conics", _f32)
    _check(opacities, "opacities", _f32)
    _check(depths, "depths", _f32)
    n = radii.numel()
    if xys.numel() != 2 * n or conics.numel() != 3 * n or opacities.numel() != n or depths.numel() != n:
        raise RuntimeError("reach_records_depth_order: xys [N,2], conics [N,3], opacities [N,1], depths [N] expected")
    dev = xys.device
    with _on(dev):
        recs = torch.empty((n + int(extra_rows), int(_typed().gsr_reach_record_bytes())), dtype=torch.uint8, device=dev)
        if extra_rows:
            recs[n:].zero_()  # (as in count_reach: the dummy culled record)
        order = torch.empty((n,), dtype=_i32, device=dev)
        nbytes = int(_typed().gsr_depth_order_workspace_bytes(n, 1))
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
        _call("gsr_reach_records_depth_order", n, xys, radii, conics, opacities, depths, tile_bounds[0], tile_bounds[1],
              recs, order, ws, nbytes, _stream(dev))
    return recs, order


MAX_SCATTER_TILES = 16384  # tile grids the device-sized path supports without reach records (tile_scatter.hip)


def bin_sorted(num_points: int, num_intersects: int, order: Tensor, cum_sorted: Optional[Tensor], xys: Tensor,
               radii: Tensor, tile_bounds: Tuple[int, int, int], block_width: int,
               reach_records: Optional[Tensor] = None, device_sized: bool = False,
               count_out: Optional[Tensor] = None, want_slots: bool = False, job_orders=None):
    """Second half (``gsr_bin_sorted``): -> (gaussian_ids_sorted i32[I],
    tile_bins i32[T,2]), identical to what ``bin_and_sort_gaussians`` returns.
    With the records (and counts) of :func:`count_reach`: the same lists without
    the pairs that cannot reach alpha >= 1/255 anywhere in their tile.
    ``device_sized``: ``num_intersects`` is only a capacity; the length is read on
    the device from ``cum_sorted[-1]`` and the lists are cut at the capacity
    (``gsr_bin_sorted_dev``) -- the caller checks ``cum_sorted[-1] <= capacity``
    later, off the critical path; ``count_out`` (int32[1], pinned host memory or
    device) receives that count.  ``cum_sorted=None``: only where :func:`lists_need_counts`
    is False.  ``want_slots``: also return ``slot_of_entry`` i32[I]
    (the inverse of the scatter, for :func:`rasterize_backward_det`).
    ``job_orders`` (device-sized lists with records): the (forward, backward) `deep_arg` words of the two job orders
    the list build leaves behind ``tile_bins`` where its last launch can carry them (``gsr_bin_sorted_dev_jobs``);
    default: the words :func:`forward_orders` will compute for these lists, ``(0, 0)``: none."""
    _check(order, "order", _i32)
    if cum_sorted is not None:
        _check(cum_sorted, "cum_sorted", _i32)
    _check(xys, "xys", _f32)
    _check(radii, "radii", _i32)
    if reach_records is not None:
        _check(reach_records, "reach_records", torch.uint8)
        if reach_records.numel() != int(num_points) * int(_typed().gsr_reach_record_bytes()):
            raise RuntimeError("bin_sorted: reach_records has the wrong size")
    I = int(num_intersects)
    nt = int(tile_bounds[0]) * int(tile_bounds[1])
    dev = xys.device
    with _on(dev):
        ids = torch.empty((I,), dtype=_i32, device=dev)
        tile_bins = alloc_tile_bins(tile_bounds, dev)
        nbytes = int(_typed().gsr_bin_sorted_workspace_bytes(int(num_points), I, tile_bounds[0], tile_bounds[1]))
        bands = cum_sorted.numel() // max(int(num_points), 1) if int(num_points) and cum_sorted is not None else 1
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
        slots = torch.empty((I,), dtype=_i32, device=dev) if want_slots else None
        head = (int(num_points), I, order, cum_sorted, xys, radii, reach_records, tile_bounds[0], tile_bounds[1],
                block_width, bands, ids, tile_bins)
        tail = (slots, ws, nbytes, _stream(dev))
        if device_sized:
            # the two job orders of the compositing launches that will walk these lists ride in the list build's last
            # launch where it can carry them (the two-level partition): the words `forward_orders` would compute
            fwd, second = (0, 0) if reach_records is None or want_slots else (
                _list_build_orders(tile_bins, I, nt, tile_bounds) if job_orders is None else job_orders)
            if fwd:
                built = C.c_int(0)
                _call("gsr_bin_sorted_dev_jobs", *head, count_out, *tail[:-1], fwd, second, C.byref(built), tail[-1])
                if built.value and second:  # (as view.hip and rasterize_gaussians_forward leave them)
                    tile_bins._gsr_jobs_bwd, tile_bins._gsr_jobs_fwd = second, fwd
                    tile_bins._gsr_jobs_by_list_build = True
            else:
                _call("gsr_bin_sorted_dev", *head, count_out, *tail)
        else:
            _call("gsr_bin_sorted", *head, *tail)
    if want_slots:
        return ids, tile_bins, slots
    return ids, tile_bins


# ---- two-round lists (include/gsraster.h "two-round lists for deep scenes") -----------------------------
def tile_lists_subrange(order_sub: Tensor, capacity: int, reach_records: Tensor, tile_bounds, ids_out: Tensor,
                        count_out: Optional[Tensor] = None) -> Tensor:
    """``gsr_tile_lists_subrange``: the two-level partition over ``order_sub`` (a contiguous slice of the depth
    order) into ``ids_out`` (int32[capacity], e.g. a slice of the combined array) -> tile_bins i32[T,2] relative
    to ``ids_out``; ``count_out`` (int32[1], device or pinned) receives the uncut length."""
    _check(order_sub, "order", _i32)
    _check(ids_out, "ids_out", _i32)
    if ids_out.numel() < int(capacity):
        raise RuntimeError("tile_lists_subrange: ids_out is smaller than the capacity")
    n = order_sub.numel()
    nt = int(tile_bounds[0]) * int(tile_bounds[1])
    dev = ids_out.device
    with _on(dev):
        bins = alloc_tile_bins(tile_bounds, dev)
        nbytes = int(_typed().gsr_tile_lists_subrange_workspace_bytes(n, int(capacity), tile_bounds[0], tile_bounds[1]))
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
        _call("gsr_tile_lists_subrange", n, int(capacity), order_sub, reach_records, tile_bounds[0], tile_bounds[1],
              ids_out, bins, count_out, ws, nbytes, _stream(dev))
    return bins


def saturation_filter(order_sub: Tensor, reach_records: Tensor, dummy_index: int, tile_flags: Tensor, tile_bounds,
                      stats_out: Optional[Tensor] = None) -> Tensor:
    """``gsr_saturation_filter``: -> a copy of ``order_sub`` in which every Gaussian whose tile box holds no flagged
    tile is replaced by ``dummy_index`` (the row of a culled record, see ``count_reach(extra_rows=1)``).
    ``tile_flags`` int32[T]; ``stats_out`` int32[2] on the device: flagged tiles, Gaussians kept."""
    _check(order_sub, "order", _i32)
    _check(tile_flags, "tile_flags", _i32)
    dev = tile_flags.device
    with _on(dev):
        out = torch.empty_like(order_sub)
        nbytes = int(_typed().gsr_saturation_filter_workspace_bytes(tile_bounds[0], tile_bounds[1]))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        _call("gsr_saturation_filter", order_sub.numel(), order_sub, reach_records, int(dummy_index), tile_flags,
              tile_bounds[0], tile_bounds[1], out, ws, nbytes, stats_out, _stream(dev))
    return out


def rasterize_forward_round(rnd: int, tile_bounds, img_size, gaussian_ids_sorted, tile_bins, idx_base: int, xys, conics,
                            colors, extra, opacities, background, extra_background: float, out_img, out_extra, final_Ts,
                            final_idx, tile_flags, out_alpha=None, zero=None) -> None:
    """``gsr_rasterize_forward_round``: round 1 composites the prefix lists into RAW state (``final_Ts`` signed,
    ``out_img`` / ``out_extra`` without background) and flags the tiles with a live pixel; round 2 resumes over the
    second lists (``tile_bins`` relative to ``idx_base``) and finalises.  All outputs are caller-owned tensors;
    ``tile_flags`` (int32[T], zeroed before round 1) and ``out_alpha`` go to BOTH rounds."""
    W, H = int(img_size[0]), int(img_size[1])
    dev = xys.device
    nt = tile_bounds[0] * tile_bounds[1]
    with _on(dev):
        _call("gsr_rasterize_forward_round", int(rnd), tile_bounds[0], tile_bounds[1], W, H, gaussian_ids_sorted,
              tile_bins, int(idx_base), xys, conics, colors, extra, opacities, background, extra_background, out_img,
              out_extra, final_Ts, final_idx, tile_flags, deep_tile_threshold(tile_bins.shape[0] * 400, nt), out_alpha,
              zero, zero.numel() * 4 if zero is not None else 0, _stream(dev))


def rasterize_backward_two(img_height, img_width, gaussian_ids_sorted, tile_bins, tile_bins2, idx_base2: int, xys,
                           conics, colors, extra, opacities, background, extra_background: float, final_Ts, final_idx,
                           v_output, v_output_extra, v_output_alpha, accumulators: Optional[Tensor] = None,
                           v_xy_abs: Optional[Tensor] = None):
    """``gsr_rasterize_backward_two``: the backward over two-round lists -> (v_xy, v_conic, v_colors, v_opacity)
    or, with ``extra``, (v_xy, v_conic, v_colors, v_extra, v_opacity).  ``v_xy_abs`` ([N,2], optional): overwritten
    with the absgrad (``gsr_rasterize_backward_two_abs``)."""
    v_output = _check(v_output.contiguous(), "v_output", _f32)
    if v_output_alpha is not None:
        v_output_alpha = _check(v_output_alpha.contiguous(), "v_output_alpha", _f32)
    if extra is not None:
        v_output_extra = _check(v_output_extra.contiguous(), "v_output_extra", _f32)
    n = xys.size(0)
    dev = xys.device
    with _on(dev):
        zeroed = accumulators is not None
        v_xy, v_conic, v_colors, v_opacity, v_extra = _carve_accumulators(accumulators, n, 3, extra is not None, dev)
        nt = ((img_width + 15) // 16) * ((img_height + 15) // 16)
        v_xy_abs = _check_absgrad(v_xy_abs, n, dev)
        _call("gsr_rasterize_backward_two" if v_xy_abs is None else "gsr_rasterize_backward_two_abs", img_height,
              img_width, n, gaussian_ids_sorted, tile_bins, tile_bins2, int(idx_base2), xys, conics, colors, extra,
              opacities, background, extra_background, final_Ts, final_idx, v_output,
              v_output_extra if extra is not None else None, v_output_alpha, v_xy, v_conic, v_colors, v_extra,
              v_opacity, deep_tile_threshold(tile_bins.shape[0] * 400, nt, backward=True), 1 if zeroed else 0,
              *(() if v_xy_abs is None else (v_xy_abs,)), _stream(dev))
    if extra is not None:
        return v_xy, v_conic, v_colors, v_extra, v_opacity
    return v_xy, v_conic, v_colors, v_opacity


def _check_absgrad(v_xy_abs: Optional[Tensor], n: int, dev) -> Optional[Tensor]:
    """``v_xy_abs``: None, or the caller's [n,2] float32 output of the ``gsr_rasterize_backward_*abs`` entries (a
    contiguous view of a larger allocation will do: exactly 2 n floats are written)."""
    if v_xy_abs is None:
        return None
    _check(v_xy_abs, "v_xy_abs", _f32)
    if tuple(v_xy_abs.shape) != (n, 2) or v_xy_abs.device != dev:
        raise RuntimeError("v_xy_abs must have dimensions (num_points, 2) on the inputs' device")
    return v_xy_abs


def _raster_inputs(gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background):
    _check(gaussian_ids_sorted, "gaussian_ids_sorted", _i32)
    _check(tile_bins, "tile_bins", _i32)
    for t, nm in ((xys, "xys"), (conics, "conics"), (colors, "colors"), (opacities, "opacities"),
                  (background, "background")):
        _check(t, nm, _f32)
    if xys.dim() != 2 or xys.size(1) != 2:
        raise RuntimeError("xys must have dimensions (num_points, 2)")
    if colors.dim() != 2:
        raise RuntimeError("colors must have 2 dimensions")
    if background.numel() != colors.size(1):
        raise RuntimeError("background must have one value per channel")


def depth_segments(list_entries: int, num_tiles: int):
    """-> (segments, minimum entries) for ``gsr_rasterize_forward_seg`` / ``gsr_rasterize_backward_seg``: into how many
    runs the lists of the tiles that are split over four waves are cut, each run walked by its own waves (DESIGN.md
    4.3; docs/history/DESIGN_r01-r05.md 4.16).  Only tile grids that cannot fill the chip gain: 16 runs (`depth_segments` in _tuning.py; 1 = off) on grids of up to
    `depth_segments_grid` = 1 100 tiles (the grids on which forward and backward split every tile), for lists of more
    than `depth_segments_min` = 512 entries.  Measured (tools/exp/seg_ab.py, profiles/r04_depth_segments.txt):
    300 k Gaussians of the trainer's object scene at 480 x 270, compositing backward 436 -> 263 us with 8 runs
    (pre-pass 75 + walk 188), forward 338 -> 295 us with 4; config 3 (whose first 2 000 iterations run on this grid)
    818 / 825 -> 871 (8 runs) -> 885 iterations/s (16).  On larger grids the kernels are bound by their total work,
    which the pre-passes raise: 960 x 540 unchanged, the long-tail 1080p scene 0.62 -> 0.67 ms (backward), the default
    0.427 -> 0.448 ms (the empty workgroups of the segment grid) -- off there."""
    segs, grid, least = _segment_knobs()[:3]
    _, _, small_grid, _, small_grid_bwd = _deep_knobs()[:5]
    # (only where EVERY tile above the small-grid floor is split, forward and backward alike: which tiles are cut, and
    #  where, is then a function of the tile's list alone and every route to the kernels rounds the same way)
    if segs < 2 or num_tiles <= 0 or num_tiles > min(grid, small_grid, small_grid_bwd):
        return 1, 0
    return segs, least


def _forward_segments(list_entries: int, num_tiles: int, H: int, W: int, dev):
    """-> (segments, minimum entries, workspace or None) of ``gsr_rasterize_forward_seg`` for this tile grid."""
    segs, seg_min = depth_segments(list_entries, num_tiles)
    cap = _segment_knobs()[3]
    if segs > 1 and cap > 0:
        # `depth_segments_fwd` (_tuning.py): until round 6 the forward walked every list twice (a transmittance pre-pass
        # from T = 1 to each run's own saturation, then the runs) and a saturating scene paid for many runs (300 k opaque
        # Gaussians at 480 x 270: 338 us single, 295 with 4 runs, 432 with 16) while a translucent one gained all the way
        # (the model config 3 ends with: 0.54 / 0.39 / 0.31 ms with 4 / 8 / 16).  The forward now walks every run once
        # (csrc/raster_fwd.hip) and re-walks only the runs in which pixels cross the stop rule's threshold.
        segs = min(segs, cap)
    if segs < 2:
        return 0, 0, None
    nbytes = int(_typed().gsr_rasterize_forward_seg_workspace_bytes(H, W, segs))
    return segs, seg_min, torch.empty((nbytes,), dtype=torch.uint8, device=dev)


_segment_cache = {}


def _segment_knobs():
    if not _segment_cache:
        # (the C entries take at most 16 runs -- GSR_REQUIRE(segments <= 16) -- and the backward calls them from inside
        #  autograd: a larger value in the table's overrides is clamped here instead of raising there)
        _segment_cache["v"] = (min(16, max(1, int(_tuning.get("depth_segments")))), int(_tuning.get("depth_segments_grid")),
                               int(_tuning.get("depth_segments_min")), min(16, max(0, int(_tuning.get("depth_segments_fwd")))))
    return _segment_cache["v"]


def deep_tile_threshold(list_entries: int, num_tiles: int, backward: bool = False) -> int:
    """List length above which a 16x16 tile is composited by four waves (one per 8x8
    sub-tile) instead of one (include/gsraster.h, ``deep_tile_threshold``): `deep_factor`
    (default 1.2; 0 = off) times the mean list length, not below `deep_min` (256; 1024 until round 5).
    `list_entries` is normally the capacity of device-sized lists (~1.25x the real count), so
    the default splits tiles above ~1.5x the mean.  Measured on the long-tail bench scene
    (10 % of the tiles ~10x deeper): forward 357 -> 320 us, backward 664 -> 625 us; factors
    0.8-1.5 within 3 % of each other, 0.3 (nearly every tile split) 1.7x slower; no effect
    on the uniform scene (nothing above the threshold; the idle workgroups cost < 1 %).
    Backward: `deep_factor_bwd` (2.0, quoted on a 1080p grid) scaled by tiles / 8 160 on grids above
    `small_grid_bwd` -- i.e. a tile is split when its list exceeds total entries / 4 096, the share of one of
    the backward's resident wave slots (`deep_factor_bwd_scaled`=0: the fixed factor)."""
    factor, floor, small_grid, small_floor, small_grid_bwd = _deep_knobs()[:5]
    if backward and _deep_knobs()[5] > 0:
        # `deep_factor_bwd` (2.0; 0 = the forward's factor): with the longest jobs first, the backward gains from
        # splitting only its longest tiles (four sub-tile waves run four butterflies): trained model 0.405 (1.2) ->
        # 0.348 ms (2.0) -> 0.40 (3.0+); long-tail scene 0.588 -> 0.559 -> 0.504 (6.0)
        factor = _deep_knobs()[5]
        if _deep_knobs()[6] and num_tiles > small_grid_bwd:
            # ... at 1080p.  The best factor follows the grid (trained model rendered at five sizes, job order on,
            # profiles/r05_midgrid_factors.txt): 2 040 tiles 0.5-0.7, 3 600 0.7-1.0, 4 590 1.4, 8 160 2.0, 14 400 3.0+
            # -- one per 4 096 tiles, the backward's resident waves (4 per SIMD): a tile is split when its list is
            # longer than the share of the launch's entries one wave slot would get.  960 x 540, the middle stage of
            # the reference's coarse-to-fine schedule: backward 0.637 -> 0.352 ms, config 3 879 -> 930+ iterations/s.
            factor *= num_tiles / _BWD_FACTOR_GRID
    if factor <= 0 or num_tiles <= 0:
        return 0
    if num_tiles <= (small_grid_bwd if backward else small_grid):
        # A small tile grid cannot fill the chip with one wave per tile (480 x 270 -- the first 2 000 iterations of
        # the reference's coarse-to-fine schedule -- is 510 tiles for 1 024 SIMDs) and every tile's list is long: the
        # walk is a serial chain of ~100 instructions per splat on a SIMD that has nothing else to issue.  Every
        # tile with more than a chunk or two of entries is split over four waves (one per 8x8 sub-tile).  Measured
        # (profiles/r04_small_grids.txt): 300 k Gaussians at 480 x 270, forward 0.32 -> 0.17 ms, backward 0.45 ->
        # 0.26 ms; 450 k at 960 x 540 (2 040 tiles), forward 0.19 -> 0.15 ms but backward 0.28 -> 0.35 ms (four
        # waves per tile also issue four times the atomics): the backward splits every tile only on grids of up to
        # `small_grid_bwd` tiles.  1080p with every tile split: 1.57 ms instead of 1.00.
        return small_floor
    return max(floor, int(factor * list_entries / num_tiles))


GSR_DEEP_ORDERED, GSR_DEEP_PREBUILT, GSR_DEEP_SECOND = 1 << 30, 1 << 29, 1 << 28  # include/gsraster.h
_DEEP_TAIL_SHIFT, _DEEP_THRESHOLD_MASK = 22, 0x3FFFFF


def tile_jobs_ints(tile_bounds) -> int:
    return int(_typed().gsr_tile_jobs_ints(int(tile_bounds[0]), int(tile_bounds[1])))


_jobs_ints_cache = {}


def alloc_tile_bins(tile_bounds, dev) -> Tensor:
    """tile_bins [tiles, 2] int32 with room behind it for the launch's job order (include/gsraster.h,
    GSR_DEEP_ORDERED): one allocation; the returned tensor is the leading [tiles, 2] view."""
    key = (int(tile_bounds[0]), int(tile_bounds[1]))
    ints = _jobs_ints_cache.get(key)
    if ints is None:
        ints = _jobs_ints_cache[key] = tile_jobs_ints(key)
    nt = key[0] * key[1]
    bins = torch.empty((2 * nt + ints,), dtype=_i32, device=dev)[:2 * nt].view(nt, 2)
    bins._gsr_job_tail = ints > 0
    return bins


def deep_arg(tile_bins: Optional[Tensor], list_entries: int, num_tiles: int, backward: bool = False, tile_bounds=None) -> int:
    """The `deep_tile_threshold` argument of a compositing entry: the threshold (`deep_tile_threshold`), with
    GSR_DEEP_ORDERED set when `tile_bins` came from `alloc_tile_bins` (so the job order fits behind it), the grid
    is not a small one and `deep_order` is not 0 -- the entry then runs the launch's jobs longest first (DESIGN.md
    section 4.1; docs/history/DESIGN_r01-r05.md section 4.18)."""
    deep = deep_tile_threshold(list_entries, num_tiles, backward) if backward else deep_tile_threshold(list_entries, num_tiles)
    if deep <= 0 or tile_bins is None or tile_bounds is None or not _order_knob():
        return deep
    # small grids (every tile split, depth segments): the launch is a few hundred short jobs per run -- nothing to
    # order, and the step is bound by the host, where one more launch costs what it costs
    if num_tiles <= (_order_cache["grid"] if _order_cache["grid"] >= 0 else _deep_knobs()[4]):
        return deep
    key = (int(tile_bounds[0]), int(tile_bounds[1]))
    ints = _jobs_ints_cache.get(key)
    if ints is None:
        ints = _jobs_ints_cache[key] = tile_jobs_ints(key)
    if ints == 0:
        return deep  # (a grid beyond the order kernel's tables -- above 3840 x 2160: the static order)
    ok = getattr(tile_bins, "_gsr_job_tail", None)  # (decided once per tensor object)
    if ok is None:
        # A tensor that does not carry the attribute (unpacked from autograd's saved tensors: a new Python object over
        # the same storage; or a caller's own bins) owns a job tail only if `alloc_tile_bins` made its storage: the
        # whole storage is exactly  2 tiles + ints  int32 and the tensor starts at its beginning.  Room behind a slice
        # of some larger live buffer is NOT a tail -- the order kernel would write over whatever follows.
        ok = (tile_bins.dtype == _i32 and tile_bins.is_contiguous() and tile_bins.storage_offset() == 0
              and tile_bins.numel() == 2 * num_tiles
              and tile_bins.untyped_storage().nbytes() == 4 * (2 * num_tiles + ints))
        try:
            tile_bins._gsr_job_tail = ok
        except AttributeError:
            pass
    if not ok:
        return deep
    # (the forward's order lives in the first of the two arrays behind tile_bins, the backward's in the second)
    return (min(deep, _DEEP_THRESHOLD_MASK) | GSR_DEEP_ORDERED | (GSR_DEEP_SECOND if backward else 0)
            | (_order_cache["tail_bwd" if backward else "tail"] << _DEEP_TAIL_SHIFT))


def _list_build_orders(tile_bins: Tensor, list_entries: int, num_tiles: int, tile_bounds):
    """-> (fwd, bwd) `deep_arg` words for the call that builds these lists, as `forward_orders` will compute them for the
    compositing forward over them; (0, 0) where it would build no pair of orders."""
    fwd = deep_arg(tile_bins, list_entries, num_tiles, tile_bounds=tile_bounds)
    if not (fwd & GSR_DEEP_ORDERED):
        return 0, 0
    bwd = deep_arg(tile_bins, list_entries, num_tiles, backward=True, tile_bounds=tile_bounds)
    if not (bwd & GSR_DEEP_ORDERED):
        return 0, 0
    return fwd, bwd


def forward_orders(tile_bins: Optional[Tensor], list_entries: int, num_tiles: int, tile_bounds, dev) -> int:
    """`deep_arg` for a compositing FORWARD, with both job orders -- this launch's and the coming backward's -- written
    by ONE small launch (`gsr_tile_jobs_build`) in front of it: the backward then finds its order ready
    (`backward_order`) and launches nothing."""
    fwd = deep_arg(tile_bins, list_entries, num_tiles, tile_bounds=tile_bounds)
    if not (fwd & GSR_DEEP_ORDERED):
        return fwd
    bwd = deep_arg(tile_bins, list_entries, num_tiles, backward=True, tile_bounds=tile_bounds)
    second = bwd if (bwd & GSR_DEEP_ORDERED) else 0
    if second and getattr(tile_bins, "_gsr_jobs_fwd", 0) == fwd and getattr(tile_bins, "_gsr_jobs_bwd", 0) == second:
        return fwd | GSR_DEEP_PREBUILT  # (the call that built these lists has written both orders behind them)
    if getattr(tile_bins, "_gsr_jobs_by_list_build", False):
        # the list build wrote orders for other words (another list count, a changed tuning row): build them again
        order_counters["orders_prebuilt_fallbacks"] += 1
        tile_bins._gsr_jobs_by_list_build = False
    _call("gsr_tile_jobs_build", int(tile_bounds[0]), int(tile_bounds[1]), tile_bins, fwd, second, _stream(dev))
    try:
        tile_bins._gsr_jobs_bwd, tile_bins._gsr_jobs_fwd = second, (fwd if second else 0)
    except AttributeError:
        pass
    return fwd | GSR_DEEP_PREBUILT


def backward_order(tile_bins: Optional[Tensor], list_entries: int, num_tiles: int, tile_bounds) -> int:
    """`deep_arg` for a compositing BACKWARD: with GSR_DEEP_PREBUILT when the forward of these very lists has already
    written this order (`forward_orders` left the argument it built for on the tensor), else the entry builds it."""
    arg = deep_arg(tile_bins, list_entries, num_tiles, backward=True, tile_bounds=tile_bounds)
    if (arg & GSR_DEEP_ORDERED) and getattr(tile_bins, "_gsr_jobs_bwd", 0) == arg:
        arg |= GSR_DEEP_PREBUILT
    return arg


_order_cache = {}
order_counters = {"orders_prebuilt_fallbacks": 0}  # (rasterizer.rasterize puts its `counters` here)


def _order_knob() -> bool:
    if not _order_cache:
        _order_cache["v"] = bool(int(_tuning.get("deep_order")))
        # the share (in 1/64ths) of a launch's whole-tile jobs that run last as four sub-tile jobs each (csrc/raster_common.h)
        _order_cache["tail"] = min(63, max(0, int(_tuning.get("deep_tail"))))
        _order_cache["tail_bwd"] = min(63, max(0, int(_tuning.get("deep_tail_bwd"))))
        # grids of up to this many tiles run in the static order (-1: small_grid_bwd, the grids on which both
        # directions split every tile and cut the lists into depth segments)
        _order_cache["grid"] = int(_tuning.get("deep_order_grid"))
    return _order_cache["v"]


_deep_cache = {}
_BWD_FACTOR_GRID = 8160.0  # (the grid `deep_factor_bwd` is quoted on: 1920 x 1080)


def _deep_knobs():
    # (read once: table look-ups per compositing call are measurable on small scenes)
    if not _deep_cache:
        g = _tuning.get
        _deep_cache["v"] = (float(g("deep_factor")), int(g("deep_min")), int(g("small_grid")), int(g("small_grid_min")),
                            int(g("small_grid_bwd")), float(g("deep_factor_bwd")), bool(int(g("deep_factor_bwd_scaled"))))
    return _deep_cache["v"]


@_tuning.on_change
def _drop_tuning_caches():
    _segment_cache.clear()
    _order_cache.clear()
    _deep_cache.clear()


class _RasterDesc(C.Structure):  # gsr_raster_desc (include/gsraster.h)
    _fields_ = ([(k, C.c_int) for k in ("num_points", "img_height", "img_width", "capacity", "deep_tile_threshold")]
                + [("extra_background", C.c_float)]
                + [(k, C.c_void_p) for k in ("xys", "depths", "radii", "conics", "colors", "extra", "opac", "background",
                                             "order_ready", "reach_records", "counts", "order", "cum", "ids",
                                             "tile_bins", "count_out", "sort_ws")]
                + [("sort_ws_bytes", C.c_size_t), ("bin_ws", C.c_void_p), ("bin_ws_bytes", C.c_size_t)]
                + [(k, C.c_void_p) for k in ("out_img", "out_extra", "final_Ts", "final_idx", "out_alpha", "zero_ptr")]
                + [("zero_bytes", C.c_size_t), ("segments", C.c_int), ("segment_min_entries", C.c_int),
                   ("seg_ws", C.c_void_p), ("seg_ws_bytes", C.c_size_t), ("deep_tile_threshold_backward", C.c_int)])


_raster_plan_cache = {}


def _raster_plan(n: int, capacity: int, tb, have_order: bool):
    """Byte offsets of the scratch regions of one `rasterize_gaussians_forward` call inside ONE allocation
    (records | order | counts | cum | sort workspace | partition workspace, each 256-byte aligned)."""
    key = (n, capacity, tb[0], tb[1], have_order)
    plan = _raster_plan_cache.get(key)
    if plan is None:
        lib = _typed()
        lean = not lists_need_counts(n, capacity, tb, device_sized=True)
        al = lambda b: (int(b) + 255) & ~255
        rec_b = al(n * int(lib.gsr_reach_record_bytes()))
        sort_b = 0 if (have_order and lean) else int(lib.gsr_depth_order_workspace_bytes(n, 1))
        bin_b = int(lib.gsr_bin_sorted_workspace_bytes(n, capacity, tb[0], tb[1]))
        off, o = {}, 0
        for name, size in (("records", rec_b), ("order", 0 if (have_order and lean) else al(4 * n)),
                           ("counts", 0 if lean else al(4 * n)), ("cum", 0 if lean else al(4 * n)),
                           ("sort_ws", al(sort_b)), ("bin_ws", al(bin_b))):
            off[name] = (o, size)
            o += size
        plan = (lean, off, max(o, 256), sort_b, bin_b)
        if len(_raster_plan_cache) > 64:
            _raster_plan_cache.clear()
        _raster_plan_cache[key] = plan
    return plan


def rasterize_gaussians_forward(xys, depths, radii, conics, colors, opacities, background, img_height: int,
                                img_width: int, capacity: int, count_out: Tensor, want_alpha: bool = False, zero=None,
                                order_ready: Optional[Tensor] = None, extra: Optional[Tensor] = None,
                                extra_background: float = 0.0, composite: bool = True, checked: bool = False):
    """``gsr_rasterize_gaussians_forward``: reach records + depth order + device-sized tile lists + compositing of
    16x16 tiles / 3 channels in ONE native call (what ``_RasterizeGaussians.forward`` runs on the device,
    rasterize.py:89-170 of the reference) -> (gaussian_ids_sorted i32[capacity], tile_bins i32[T,2], out_img,
    final_Ts, final_idx, alpha or None[, out_extra]).  ``count_out`` (int32[1], pinned or device) receives the number
    of list entries the view needs: above ``capacity`` the lists were cut and the caller builds them again.
    ``order_ready``: the depth order of these depths / radii if the caller already has it (the sort is skipped).
    ``composite=False``: the lists only -> (gaussian_ids_sorted, tile_bins); ``colors`` / ``background`` unused."""
    n = xys.size(0)
    dev = xys.device
    for t, dt, width in () if checked else ((xys, _f32, 2), (depths, _f32, 1), (radii, _i32, 1), (conics, _f32, 3), (opacities, _f32, 1)) + (
            ((colors, _f32, 3), (background, _f32, None)) if composite else ()):
        if t.dtype != dt or t.device != dev or not t.is_contiguous() or (width is not None and t.numel() != n * width):
            raise RuntimeError("rasterize_gaussians_forward: float32 / int32 contiguous tensors of one device with N rows "
                               "expected (xys [N,2], depths [N], radii [N], conics [N,3], colors [N,3], opacities [N,1])")
    if (composite and background.numel() != 3) or n < 1 or capacity < 1:
        raise RuntimeError("rasterize_gaussians_forward: background [3], N >= 1 and capacity >= 1 expected")
    tb = ((img_width + 15) // 16, (img_height + 15) // 16, 1)
    if order_ready is not None and lists_need_counts(n, capacity, tb, device_sized=True):
        order_ready = None  # lists with counts sort the counts along: the ready-made order is of no use
    lean, off, total, sort_b, bin_b = _raster_plan(n, capacity, tb, order_ready is not None)
    H, W = int(img_height), int(img_width)
    with _on(dev):
        ws = torch.empty((total,), dtype=torch.uint8, device=dev)
        ids = torch.empty((capacity,), dtype=_i32, device=dev)
        bins = alloc_tile_bins(tb, dev)
        img = Ts = idx = alpha = out_extra = None
        if composite:
            img = torch.empty((H, W, 3), dtype=_f32, device=dev)
            # final_Ts | final_idx | alpha [| extra]: one allocation, three (four) [H,W] planes
            planes = torch.empty((2 + int(want_alpha) + int(extra is not None), H, W), dtype=_f32, device=dev)
            Ts, idx = planes[0], planes[1].view(_i32)
            alpha = planes[2] if want_alpha else None
            out_extra = planes[2 + int(want_alpha)] if extra is not None else None
        base = ws.data_ptr()
        at = lambda name: (base + off[name][0]) if off[name][1] else None
        p = lambda t: None if t is None else t.data_ptr()
        zero_bytes = 0
        if zero is not None:
            zero_bytes = zero.numel() * 4
            if zero_bytes == 0:
                zero = None
        segs, seg_min, seg_ws = _forward_segments(capacity, tb[0] * tb[1], H, W, dev) if composite else (0, 0, None)
        desc = _RasterDesc(n, H, W, int(capacity), deep_arg(bins, capacity, tb[0] * tb[1], tile_bounds=tb), float(extra_background),
                           xys.data_ptr(), depths.data_ptr(), radii.data_ptr(), conics.data_ptr(),
                           p(colors) if composite else None, p(extra), opacities.data_ptr(),
                           p(background) if composite else None, p(order_ready), at("records"),
                           at("counts"), at("order"), at("cum"), ids.data_ptr(), bins.data_ptr(), count_out.data_ptr(),
                           at("sort_ws"), sort_b, at("bin_ws"), bin_b, p(img), p(out_extra), p(Ts),
                           p(idx), p(alpha), p(zero), zero_bytes, segs, seg_min, p(seg_ws),
                           seg_ws.numel() if seg_ws is not None else 0, 0)
        if desc.deep_tile_threshold & GSR_DEEP_ORDERED:
            # both job orders -- this forward's (or, for lists built ahead, the later compositing call's) and the
            # coming backward's -- ride in one launch behind the lists (include/gsraster.h)
            bwd = deep_arg(bins, capacity, tb[0] * tb[1], backward=True, tile_bounds=tb)
            if bwd & GSR_DEEP_ORDERED:
                desc.deep_tile_threshold_backward = bwd
                bins._gsr_jobs_bwd = bwd
                bins._gsr_jobs_fwd = int(desc.deep_tile_threshold)
        _call("gsr_rasterize_gaussians_forward", C.byref(desc), _stream(dev))
    if not composite:
        return ids, bins
    if extra is not None:
        return ids, bins, img, Ts, idx, alpha, out_extra
    return ids, bins, img, Ts, idx, alpha


def _composite16_forward(tile_bounds, W: int, H: int, gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities,
                         background, out_img, final_Ts, final_idx, dev, *, extra=None, extra_background: float = 0.0,
                         out_extra=None, alpha=None, zero=None, deep: Optional[int] = None) -> None:
    """The one call of ``gsr_rasterize_forward_seg`` -- the 16-px, 3-channel compositing forward, with or without the
    ``extra`` channel, into the caller's outputs.  The entry cuts the deep lists into the runs of
    :func:`_forward_segments` where that gives any, and is ``gsr_rasterize_forward_ex`` / ``_rgbd`` where not.
    ``deep``: the deep argument (default: :func:`forward_orders`); ``zero``: a float32 tensor the launch clears."""
    entries, tiles = gaussian_ids_sorted.numel(), tile_bounds[0] * tile_bounds[1]
    if deep is None:
        deep = forward_orders(tile_bins, entries, tiles, tile_bounds, dev)
    segs, seg_min, seg_ws = _forward_segments(entries, tiles, H, W, dev)
    zero_bytes = zero.numel() * 4 if zero is not None else 0
    _call("gsr_rasterize_forward_seg", tile_bounds[0], tile_bounds[1], W, H, gaussian_ids_sorted, tile_bins, xys,
          conics, colors, extra, opacities, background, extra_background, out_img, out_extra, final_Ts, final_idx, deep,
          alpha, zero if zero_bytes else None, zero_bytes, segs, seg_min, seg_ws,
          seg_ws.numel() if seg_ws is not None else 0, _stream(dev))


def composite_prepared(tile_bounds, img_width: int, img_height: int, gaussian_ids_sorted, tile_bins, xys, conics, colors,
                       opacities, background, out_img, planes, want_alpha: bool, zero=None):
    """The 16-px compositing forward into caller-owned outputs, for callers that have validated their tensors and
    allocated ``out_img`` [H,W,3] and ``planes`` [3,H,W] (final_Ts | final_idx as int32 | alpha) ahead of time: the
    shortest host path to the compositing launch (rasterize.py, "lists built ahead of time")
    -> (out_img, final_Ts, final_idx, alpha or None)."""
    dev = xys.device
    Ts, idx = planes[0], planes[1].view(_i32)
    alpha = planes[2] if want_alpha else None
    with _on(dev):
        _composite16_forward(tile_bounds, int(img_width), int(img_height), gaussian_ids_sorted, tile_bins, xys, conics,
                             colors, opacities, background, out_img, Ts, idx, dev, alpha=alpha, zero=zero)
    return out_img, Ts, idx, alpha


def rasterize_forward_ex(tile_bounds, block, img_size, gaussian_ids_sorted, tile_bins, xys, conics,
                         colors, opacities, background, want_alpha=False, zero=None):
    """``gsr_rasterize_forward_ex`` (16x16 tiles, 3 channels): -> (out_img, final_Ts, final_idx, alpha or None);
    ``alpha = 1 - final_Ts`` written by the kernel; ``zero``: a float32 tensor the launch clears (the
    accumulators of the coming :func:`rasterize_backward` -- see ``accumulators``)."""
    return _rasterize_forward(tile_bounds, block, img_size, gaussian_ids_sorted, tile_bins, xys,
                              conics, colors, opacities, background, nd=False, want_alpha=want_alpha, zero=zero,
                              ex=True)


def _rasterize_forward(tile_bounds, block, img_size, gaussian_ids_sorted, tile_bins, xys, conics,
                       colors, opacities, background, nd: bool, want_alpha: bool = False, zero=None, ex: bool = False):
    _raster_inputs(gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background)
    channels = colors.size(1)
    W, H = int(img_size[0]), int(img_size[1])
    dev = xys.device
    with _on(dev):
        out_img = torch.empty((H, W, channels), dtype=_f32, device=dev)
        final_Ts = torch.empty((H, W), dtype=_f32, device=dev)
        final_idx = torch.empty((H, W), dtype=_i32, device=dev)
        if not nd and channels != 3:
            raise RuntimeError("rasterize_forward expects 3 channels; use nd_rasterize_forward")
        alpha = None
        if ex:
            if zero is not None and _check(zero, "zero", _f32).numel() == 0:
                zero = None
            alpha = torch.empty((H, W), dtype=_f32, device=dev) if want_alpha else None
        if not nd and block[0] == 16:
            _composite16_forward(tile_bounds, W, H, gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities,
                                 background, out_img, final_Ts, final_idx, dev, alpha=alpha, zero=zero if ex else None)
        else:
            if alpha is not None or (ex and zero is not None):  # (the generic kernel writes neither)
                raise RuntimeError("rasterize_forward_ex: out_alpha / zero_ptr need block_width 16")
            sizes = (tile_bounds[0], tile_bounds[1], block[0], W, H)
            args = (gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background, out_img, final_Ts,
                    final_idx)
            if nd:
                _call("gsr_rasterize_forward_nd", *sizes, channels, *args, _stream(dev))
            else:
                deep = deep_tile_threshold(gaussian_ids_sorted.numel(), tile_bounds[0] * tile_bounds[1])
                _call("gsr_rasterize_forward", *sizes, *args, deep, _stream(dev))
    return (out_img, final_Ts, final_idx, alpha) if ex else (out_img, final_Ts, final_idx)


def rasterize_forward(tile_bounds, block, img_size, gaussian_ids_sorted, tile_bins, xys, conics,
                      colors, opacities, background):
    """-> (out_img [H,W,3], final_Ts [H,W], final_idx i32[H,W]);
    replaces ``rasterize_forward_tensor`` (bindings.cu:269-328)."""
    return _rasterize_forward(tile_bounds, block, img_size, gaussian_ids_sorted, tile_bins, xys,
                              conics, colors, opacities, background, nd=False)


def rasterize_forward_scan(tile_bounds, img_size, gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities,
                           background):
    """`rasterize_forward` through the scan mapping (``gsr_rasterize_forward_scan``; measurement variant,
    16x16 tiles): lanes over splats, wave prefix product for the transmittance."""
    _raster_inputs(gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background)
    W, H = int(img_size[0]), int(img_size[1])
    dev = xys.device
    with _on(dev):
        img = torch.empty((H, W, 3), dtype=_f32, device=dev)
        Ts = torch.empty((H, W), dtype=_f32, device=dev)
        idx = torch.empty((H, W), dtype=_i32, device=dev)
        _call("gsr_rasterize_forward_scan", tile_bounds[0], tile_bounds[1], W, H, gaussian_ids_sorted, tile_bins, xys,
              conics, colors, opacities, background, img, Ts, idx, _stream(dev))
    return img, Ts, idx


def nd_rasterize_forward(tile_bounds, block, img_size, gaussian_ids_sorted, tile_bins, xys, conics,
                         colors, opacities, background):
    """Generic channel count; replaces ``nd_rasterize_forward_tensor``
    (bindings.cu:330-399).  Accumulates in fp32 (the reference uses fp16)."""
    return _rasterize_forward(tile_bounds, block, img_size, gaussian_ids_sorted, tile_bins, xys,
                              conics, colors, opacities, background, nd=True)


def rasterize_forward_rgbd(tile_bounds, img_size, gaussian_ids_sorted, tile_bins, xys, conics, colors, extra,
                           opacities, background, extra_background: float, want_alpha: bool = False, zero=None):
    """RGB + one extra channel in one pass (``gsr_rasterize_forward_rgbd``, 16x16 tiles):
    -> (out_img [H,W,3], out_extra [H,W], final_Ts [H,W], final_idx i32[H,W]) [+ alpha = 1 - final_Ts
    when ``want_alpha``].  ``zero``: a float32 tensor the launch clears (``backward_accumulators(n, 4, dev)``
    for the coming :func:`rasterize_backward_rgbd`)."""
    _raster_inputs(gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background)
    _check(extra, "extra", _f32)
    if colors.size(1) != 3 or extra.numel() != xys.size(0):
        raise RuntimeError("rasterize_forward_rgbd expects colors [N,3] and extra [N]")
    W, H = int(img_size[0]), int(img_size[1])
    dev = xys.device
    with _on(dev):
        img = torch.empty((H, W, 3), dtype=_f32, device=dev)
        ext = torch.empty((H, W), dtype=_f32, device=dev)
        Ts = torch.empty((H, W), dtype=_f32, device=dev)
        idx = torch.empty((H, W), dtype=_i32, device=dev)
        alpha = torch.empty((H, W), dtype=_f32, device=dev) if want_alpha else None
        if zero is not None:
            _check(zero, "zero", _f32)
        _composite16_forward(tile_bounds, W, H, gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background,
                             img, Ts, idx, dev, extra=extra, extra_background=extra_background, out_extra=ext, alpha=alpha,
                             zero=zero)
    if want_alpha:
        return img, ext, Ts, idx, alpha
    return img, ext, Ts, idx


def rasterize_backward_rgbd(img_height, img_width, gaussian_ids_sorted, tile_bins, xys, conics, colors, extra,
                            opacities, background, extra_background, final_Ts, final_idx, v_output,
                            v_output_extra, v_output_alpha, accumulators: Optional[Tensor] = None,
                            v_xy_abs: Optional[Tensor] = None):
    """-> (v_xy, v_conic, v_colors, v_extra [N], v_opacity [N,1]); ``gsr_rasterize_backward_rgbd``.
    ``accumulators``: ``backward_accumulators(n, 4, dev)`` already cleared by the forward launch.
    ``v_xy_abs`` ([N,2], optional): overwritten with the absgrad."""
    _raster_inputs(gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background)
    _check(extra, "extra", _f32)
    v_output = _check(v_output.contiguous(), "v_output", _f32)
    v_output_extra = _check(v_output_extra.contiguous(), "v_output_extra", _f32)
    if v_output_alpha is not None:
        v_output_alpha = _check(v_output_alpha.contiguous(), "v_output_alpha", _f32)
    n = xys.size(0)
    dev = xys.device
    with _on(dev):
        v_xy, v_conic, v_colors, v_opacity, v_extra = _carve_accumulators(accumulators, n, 3, True, dev)
        _composite16_backward(img_height, img_width, n, gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities,
                              background, final_Ts, final_idx, v_output, v_output_alpha, v_xy, v_conic, v_colors,
                              v_opacity, accumulators is not None, dev, extra=extra, extra_background=extra_background,
                              v_output_extra=v_output_extra, v_extra=v_extra, v_xy_abs=v_xy_abs)
    return v_xy, v_conic, v_colors, v_extra, v_opacity


def rasterize_backward_det(img_height, img_width, gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities,
                           background, final_Ts, final_idx, v_output, v_output_alpha, order, cum_sorted, slot_of_entry,
                           extra=None, extra_background: float = 0.0, v_output_extra=None,
                           v_xy_abs: Optional[Tensor] = None):
    """``gsr_rasterize_backward_det``: the compositing backward with a fixed summation order
    (bit-identical gradients from run to run) -> (v_xy, v_conic, v_colors, v_opacity [N,1]) or,
    with ``extra`` / ``v_output_extra``, (v_xy, v_conic, v_colors, v_extra [N], v_opacity).
    ``v_xy_abs`` ([N,2], optional): overwritten with the absgrad, bit-reproducible as well
    (``gsr_rasterize_backward_det_abs``)."""
    _raster_inputs(gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background)
    for t, nm in ((order, "order"), (cum_sorted, "cum_sorted"), (slot_of_entry, "slot_of_entry")):
        _check(t, nm, _i32)
    v_output = _check(v_output.contiguous(), "v_output", _f32)
    if v_output_alpha is not None:
        v_output_alpha = _check(v_output_alpha.contiguous(), "v_output_alpha", _f32)
    rgbd = extra is not None
    if rgbd:
        _check(extra, "extra", _f32)
        v_output_extra = _check(v_output_extra.contiguous(), "v_output_extra", _f32)
    n = xys.size(0)
    L = gaussian_ids_sorted.numel()
    if slot_of_entry.numel() != L or order.numel() != n or cum_sorted.numel() % max(n, 1):
        raise RuntimeError("rasterize_backward_det: order / cum_sorted / slot_of_entry do not match the lists")
    bands = cum_sorted.numel() // n if n else 1
    dev = xys.device
    with _on(dev):
        v_xy = torch.empty((n, 2), dtype=_f32, device=dev)
        v_conic = torch.empty((n, 3), dtype=_f32, device=dev)
        v_colors = torch.empty((n, 3), dtype=_f32, device=dev)
        v_opacity = torch.empty((n, 1), dtype=_f32, device=dev)
        v_extra = torch.empty((n,), dtype=_f32, device=dev) if rgbd else None
        nbytes = int(_typed().gsr_rasterize_backward_det_workspace_bytes(L))
        ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)
        v_xy_abs = _check_absgrad(v_xy_abs, n, dev)
        _call("gsr_rasterize_backward_det" if v_xy_abs is None else "gsr_rasterize_backward_det_abs", img_height,
              img_width, n, L, gaussian_ids_sorted, tile_bins, xys, conics, colors, extra, opacities, background,
              extra_background, final_Ts, final_idx, v_output, v_output_extra, v_output_alpha, order, cum_sorted, bands,
              slot_of_entry, ws, nbytes, v_xy, v_conic, v_colors, v_extra, v_opacity,
              *(() if v_xy_abs is None else (v_xy_abs,)), _stream(dev))
    if rgbd:
        return v_xy, v_conic, v_colors, v_extra, v_opacity
    return v_xy, v_conic, v_colors, v_opacity


def backward_accumulators(n: int, channels: int, device) -> Tensor:
    """The flat float32 buffer :func:`rasterize_backward` carves ``v_xy | v_conic | v_colors | v_opacity``
    out of.  Cleared by ``rasterize_forward_ex(zero=...)`` and handed back as ``accumulators`` it spares
    the backward its own zero fill."""
    with torch.cuda.device(device):
        return torch.empty((n * (6 + channels),), dtype=_f32, device=device)


def _carve_accumulators(flat: Optional[Tensor], n: int, channels: int, with_extra: bool, dev):
    """-> (v_xy [n,2], v_conic [n,3], v_colors [n,channels], v_opacity [n,1], v_extra [n] or None): views of ONE
    allocation, back to back (the library clears them with one fill) -- of ``flat``, a :func:`backward_accumulators`
    buffer the forward launch has already cleared, or of a new one."""
    k = 6 + channels + (1 if with_extra else 0)
    if flat is None:
        flat = torch.empty((n * k,), dtype=_f32, device=dev)
    elif flat.numel() != n * k or flat.dtype != _f32 or not flat.is_contiguous():
        raise RuntimeError(f"accumulators must be backward_accumulators(n, {k - 6}, device)")
    v_opacity = flat[(5 + channels) * n: (6 + channels) * n].view(n, 1)
    return (flat[: 2 * n].view(n, 2), flat[2 * n: 5 * n].view(n, 3), flat[5 * n: (5 + channels) * n].view(n, channels),
            v_opacity, flat[(6 + channels) * n:] if with_extra else None)


def _composite16_backward(img_height, img_width, n: int, gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities,
                          background, final_Ts, final_idx, v_output, v_output_alpha, v_xy, v_conic, v_colors, v_opacity,
                          zeroed: bool, dev, *, extra=None, extra_background: float = 0.0, v_output_extra=None,
                          v_extra=None, v_xy_abs: Optional[Tensor] = None) -> None:
    """The one call of ``gsr_rasterize_backward_seg`` -- the 16-px, 3-channel compositing backward, with or without
    the ``extra`` channel.  The entry cuts the deep lists into the runs of :func:`depth_segments` where that gives any,
    and is ``gsr_rasterize_backward_ex`` / ``_rgbd`` where not.  ``zeroed``: the accumulators are cleared already.
    ``v_xy_abs`` ([n,2]): ``gsr_rasterize_backward_abs`` instead -- the same call, which also overwrites it with the
    absgrad."""
    tb = ((int(img_width) + 15) // 16, (int(img_height) + 15) // 16)
    entries, tiles = gaussian_ids_sorted.numel(), tb[0] * tb[1]
    segs, seg_min = depth_segments(entries, tiles)
    ws = torch.empty(((segs - 1) * int(img_height) * int(img_width), 2), dtype=_f32, device=dev) if segs > 1 else None
    v_xy_abs = _check_absgrad(v_xy_abs, n, dev)
    _call("gsr_rasterize_backward_seg" if v_xy_abs is None else "gsr_rasterize_backward_abs", img_height, img_width, n,
          gaussian_ids_sorted, tile_bins, xys, conics, colors, extra, opacities, background, extra_background, final_Ts,
          final_idx, v_output, v_output_extra, v_output_alpha, v_xy, v_conic, v_colors, v_extra, v_opacity,
          backward_order(tile_bins, entries, tiles, tb), 1 if zeroed else 0, segs if ws is not None else 0, seg_min, ws,
          ws.numel() * 4 if ws is not None else 0, *(() if v_xy_abs is None else (v_xy_abs,)), _stream(dev))


def _rasterize_backward(img_height, img_width, block_width, gaussian_ids_sorted, tile_bins, xys,
                        conics, colors, opacities, background, final_Ts, final_idx, v_output,
                        v_output_alpha, nd: bool, accumulators: Optional[Tensor] = None, trusted: bool = False,
                        v_xy_abs: Optional[Tensor] = None):
    if v_xy_abs is not None and (nd or block_width != 16 or colors.size(1) != 3):
        raise ValueError("absgrad (v_xy_abs) needs block_width 16 and 3 colour channels: the generic kernels do not "
                         "compute it")
    if not trusted:  # (trusted: everything but the two cotangents went through the forward's checks)
        _raster_inputs(gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background)
        if not nd and colors.size(1) != 3:
            raise RuntimeError("colors must have 2 dimensions")  # message of bindings.cu:494-496
        _check(final_Ts, "final_Ts", _f32)
        _check(final_idx, "final_idx", _i32)
    v_output = _check(v_output.contiguous(), "v_output", _f32)
    if v_output_alpha is not None:  # None = zero cotangent for the alpha output
        v_output_alpha = _check(v_output_alpha.contiguous(), "v_output_alpha", _f32)
    n, channels = xys.size(0), colors.size(1)
    dev = xys.device
    with _on(dev):
        tile16 = not nd and block_width == 16
        zeroed = accumulators is not None and tile16  # (the generic kernels' entries clear for themselves)
        v_xy, v_conic, v_colors, v_opacity, _ = _carve_accumulators(accumulators if zeroed else None, n, channels, False, dev)
        if tile16:
            _composite16_backward(img_height, img_width, n, gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities,
                                  background, final_Ts, final_idx, v_output, v_output_alpha, v_xy, v_conic, v_colors,
                                  v_opacity, zeroed, dev, v_xy_abs=v_xy_abs)
        else:
            sizes = (img_height, img_width, block_width)
            args = (n, gaussian_ids_sorted, tile_bins, xys, conics, colors, opacities, background, final_Ts, final_idx,
                    v_output, v_output_alpha, v_xy, v_conic, v_colors, v_opacity)
            if nd:
                _call("gsr_rasterize_backward_nd", *sizes, channels, *args, _stream(dev))
            else:
                tiles = ((img_width + block_width - 1) // block_width) * ((img_height + block_width - 1) // block_width)
                deep = deep_tile_threshold(gaussian_ids_sorted.numel(), tiles, backward=True)
                _call("gsr_rasterize_backward", *sizes, *args, deep, _stream(dev))
    return v_xy, v_conic, v_colors, v_opacity


def rasterize_backward(img_height, img_width, block_width, gaussian_ids_sorted, tile_bins, xys,
                       conics, colors, opacities, background, final_Ts, final_idx, v_output,
                       v_output_alpha, accumulators: Optional[Tensor] = None, trusted: bool = False,
                       v_xy_abs: Optional[Tensor] = None):
    """-> (v_xy, v_conic, v_colors, v_opacity [N,1]);
    replaces ``rasterize_backward_tensor`` (bindings.cu:476-528).  ``accumulators``: a
    :func:`backward_accumulators` buffer already cleared by :func:`rasterize_forward_ex`.
    ``v_xy_abs`` ([N,2], optional; block_width 16): overwritten with the absgrad (``gsr_rasterize_backward_abs``)."""
    return _rasterize_backward(img_height, img_width, block_width, gaussian_ids_sorted, tile_bins,
                               xys, conics, colors, opacities, background, final_Ts, final_idx,
                               v_output, v_output_alpha, nd=False, accumulators=accumulators, trusted=trusted,
                               v_xy_abs=v_xy_abs)


def nd_rasterize_backward(img_height, img_width, block_width, gaussian_ids_sorted, tile_bins, xys,
                          conics, colors, opacities, background, final_Ts, final_idx, v_output,
                          v_output_alpha):
    """Generic channel count; replaces ``nd_rasterize_backward_tensor`` (bindings.cu:406-469)."""
    return _rasterize_backward(img_height, img_width, block_width, gaussian_ids_sorted, tile_bins,
                               xys, conics, colors, opacities, background, final_Ts, final_idx,
                               v_output, v_output_alpha, nd=True)


def compute_cov2d_bounds(num_pts: int, cov2d: Tensor) -> Tuple[Tensor, Tensor]:
    """-> (conics [N,3], radii [N,1] f32); replaces ``compute_cov2d_bounds_tensor``
    (bindings.cu:39-56)."""
    _check(cov2d, "cov2d", _f32)
    n = int(num_pts)
    dev = cov2d.device
    with _on(dev):
        conics = torch.empty((n, cov2d.size(1)), dtype=_f32, device=dev)
        radii = torch.empty((n, 1), dtype=_f32, device=dev)
        _call("gsr_cov2d_bounds", n, cov2d, conics, radii, _stream(dev))
    return conics, radii


def _distortion_inputs(gaussian_ids_sorted, tile_bins, xys, conics, opacities, values):
    _check(gaussian_ids_sorted, "gaussian_ids_sorted", _i32)
    _check(tile_bins, "tile_bins", _i32)
    for t, nm in ((xys, "xys"), (conics, "conics"), (opacities, "opacities"), (values, "values")):
        _check(t, nm, _f32)
    n = xys.size(0)
    if xys.dim() != 2 or xys.size(1) != 2:
        raise RuntimeError("xys must have dimensions (num_points, 2)")
    if tuple(conics.shape) != (n, 3) or opacities.numel() != n or values.numel() != n:
        raise RuntimeError("conics, opacities and values must hold 3, 1 and 1 value per point of xys")
    for t, nm in ((gaussian_ids_sorted, "gaussian_ids_sorted"), (tile_bins, "tile_bins"), (conics, "conics"),
                  (opacities, "opacities"), (values, "values")):
        if t.device != xys.device:
            raise RuntimeError(f"{nm} must be on the device of xys")


def distortion_forward(tile_bounds, img_size, gaussian_ids_sorted, tile_bins, xys, conics, opacities, values):
    """The depth-distortion walk on given single-segment lists of 16 x 16 tiles (``gsr_distortion_forward``)
    -> (distortion, median, vsum, final_Ts [H,W] float32, final_idx [H,W] int32).  ``values`` [N]: one scalar per
    Gaussian.  A view without list entries launches nothing: zeros, final_Ts = 1, final_idx = -1."""
    W, H = int(img_size[0]), int(img_size[1])
    if W < 1 or H < 1:
        raise RuntimeError("distortion_forward: empty image")
    if tuple(int(v) for v in tile_bounds[:2]) != ((W + 15) // 16, (H + 15) // 16):
        raise RuntimeError(f"distortion_forward: tile bounds {tuple(tile_bounds)} are not those of a {W} x {H} image in "
                           f"16 x 16 tiles")
    dev = xys.device
    if gaussian_ids_sorted is None or gaussian_ids_sorted.numel() == 0:
        with _on(dev):
            z = torch.zeros((3, H, W), dtype=_f32, device=dev)
            return (z[0], z[1], z[2], torch.ones((H, W), dtype=_f32, device=dev),
                    torch.full((H, W), -1, dtype=_i32, device=dev))
    _distortion_inputs(gaussian_ids_sorted, tile_bins, xys, conics, opacities, values)
    if tile_bins.numel() < 2 * tile_bounds[0] * tile_bounds[1]:
        raise RuntimeError("tile_bins must hold one (start, end) pair per tile")
    with _on(dev):
        planes = torch.empty((4, H, W), dtype=_f32, device=dev)
        final_idx = torch.empty((H, W), dtype=_i32, device=dev)
        _call("gsr_distortion_forward", tile_bounds[0], tile_bounds[1], W, H, gaussian_ids_sorted, tile_bins, xys, conics,
              opacities, values, planes[0], planes[1], planes[2], planes[3], final_idx, _stream(dev))
    return planes[0], planes[1], planes[2], planes[3], final_idx


def distortion_backward(img_height, img_width, gaussian_ids_sorted, tile_bins, xys, conics, opacities, values, vsum,
                        final_Ts, final_idx, v_distortion):
    """-> (v_xy [N,2], v_conic [N,3], v_opacity [N], v_values [N]) of `distortion_forward` (``gsr_distortion_backward``;
    float atomics).  A view without list entries launches nothing: zeros."""
    H, W = int(img_height), int(img_width)
    n, dev = xys.size(0), xys.device
    with _on(dev):
        if gaussian_ids_sorted is None or gaussian_ids_sorted.numel() == 0 or n == 0:
            flat = torch.zeros((7 * n,), dtype=_f32, device=dev)
        else:
            _distortion_inputs(gaussian_ids_sorted, tile_bins, xys, conics, opacities, values)
            for t, nm, dt in ((vsum, "vsum", _f32), (final_Ts, "final_Ts", _f32), (final_idx, "final_idx", _i32)):
                if tuple(_check(t, nm, dt).shape) != (H, W) or t.device != dev:
                    raise RuntimeError(f"{nm} must have dimensions ({H}, {W}) on the device of xys")
            v_distortion = _check(v_distortion.contiguous(), "v_distortion", _f32)
            if v_distortion.numel() != H * W or v_distortion.device != dev:
                raise RuntimeError(f"v_distortion must hold {H} x {W} values on the device of xys")
            if tile_bins.numel() < 2 * ((W + 15) // 16) * ((H + 15) // 16):
                raise RuntimeError("tile_bins must hold one (start, end) pair per tile")
            flat = torch.empty((7 * n,), dtype=_f32, device=dev)  # (cleared by the entry: one fill)
            _call("gsr_distortion_backward", H, W, n, gaussian_ids_sorted, tile_bins, xys, conics, opacities, values,
                  vsum, final_Ts, final_idx, v_distortion, flat[:2 * n], flat[2 * n:5 * n], flat[5 * n:6 * n],
                  flat[6 * n:], _stream(dev))
    return flat[:2 * n].view(n, 2), flat[2 * n:5 * n].view(n, 3), flat[5 * n:6 * n], flat[6 * n:]


def contribution_accumulate(tile_bounds, img_size, gaussian_ids_sorted, tile_bins, xys, conics, opacities, max_w, sum_q,
                            hits, dominant) -> None:
    """The contribution walk on given single-segment lists of 16 x 16 tiles (``gsr_contribution_accumulate``): ADDS the
    view's blend-weight statistics to the caller's ``max_w`` float32 [N], ``sum_q``, ``hits`` and ``dominant`` int64
    [N], in place.  A view without list entries launches nothing and changes nothing."""
    W, H = int(img_size[0]), int(img_size[1])
    if W < 1 or H < 1:
        raise RuntimeError("contribution_accumulate: empty image")
    if tuple(int(v) for v in tile_bounds[:2]) != ((W + 15) // 16, (H + 15) // 16):
        raise RuntimeError(f"contribution_accumulate: tile bounds {tuple(tile_bounds)} are not those of a {W} x {H} "
                           f"image in 16 x 16 tiles")
    n, dev = xys.size(0), xys.device
    for t, nm, dt in ((max_w, "max_w", _f32), (sum_q, "sum_q", torch.int64), (hits, "hits", torch.int64),
                      (dominant, "dominant", torch.int64)):
        if tuple(_check(t, nm, dt).shape) != (n,) or t.device != dev:
            raise RuntimeError(f"{nm} must have dimensions ({n},) on the device of xys")
    if gaussian_ids_sorted is None or gaussian_ids_sorted.numel() == 0 or n == 0:
        return
    _distortion_inputs(gaussian_ids_sorted, tile_bins, xys, conics, opacities, opacities)
    if tile_bins.numel() < 2 * tile_bounds[0] * tile_bounds[1]:
        raise RuntimeError("tile_bins must hold one (start, end) pair per tile")
    with _on(dev):
        _call("gsr_contribution_accumulate", tile_bounds[0], tile_bounds[1], W, H, n, gaussian_ids_sorted, tile_bins, xys,
              conics, opacities, max_w, sum_q, hits, dominant, _stream(dev))
