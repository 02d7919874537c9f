"""Normal maps and the depth-normal consistency loss of surface-oriented training, on csrc/normals.hip (DESIGN.md
section 4.19; the rule is stated in include/gsraster.h).  What 2DGS, GOF, RaDe-GS, PGSR and gsplat's `normal_lambda`
share: every Gaussian gets a normal, the normals are composited into an image, a second normal image is derived from
the rendered depth, and their disagreement is penalised.

    gaussian_normals(quats, scales, means, viewmat)                 [N,3]; gradients to quats
    depth_to_normal(depth, alpha, fx, fy, cx, cy)                   [H,W,3]; no gradient
    normal_consistency_loss(normals_img, depth, alpha, fx, fy, cx, cy, mask=None)
                                                                    scalar; gradients to normals_img and depth

Camera space is the projection's (x right, y down, z forward); the centre of pixel (row i, column j) is
(j + 0.5, i + 0.5).  float32 in and out, float64 per-element arithmetic, the loss a float64 sum in a fixed order without
atomics: two runs are bit-equal.  CUDA tensors only; no CPU fallback."""
import torch
from torch import Tensor
from torch.autograd import Function

from rasterizer.cuda import _call, _check, _stream

_f32 = torch.float32
TILE = 16  # GSR_NORMAL_TILE (include/gsraster.h)


def workspace_doubles(H: int, W: int) -> int:
    """GSR_NORMAL_WORKSPACE_DOUBLES."""
    return ((H + TILE - 1) // TILE) * ((W + TILE - 1) // TILE)


def _tensors(**named) -> None:
    for name, t in named.items():
        if not isinstance(t, Tensor):
            raise RuntimeError(f"{name} must be a tensor")


def _plane(t: Tensor, name: str) -> Tensor:
    """[H,W] from [H,W] or [H,W,1] (a view); ValueError for anything else or an empty image."""
    if t.dim() == 3 and t.shape[-1] == 1:
        t = t[..., 0]
    if t.dim() != 2 or t.numel() == 0:
        raise ValueError(f"expected {name} [H,W] (or [H,W,1]), non-empty, got {tuple(t.shape)}")
    return t


def _same_plane(t: Tensor, name: str, H: int, W: int) -> Tensor:
    if tuple(t.shape) not in ((H, W), (H, W, 1)):
        raise ValueError(f"expected {name} [{H},{W}] or [{H},{W},1], got {tuple(t.shape)}")
    return t.reshape(H, W)


def _intrinsics(fx, fy, cx, cy):
    try:
        k = tuple(float(v) for v in (fx, fy, cx, cy))
    except (TypeError, ValueError):
        raise ValueError(f"fx, fy, cx, cy must be numbers, got {(fx, fy, cx, cy)!r}") from None
    if not (k[0] != 0.0 and k[1] != 0.0) or any(v != v for v in k):
        raise ValueError(f"fx and fy must be non-zero and no intrinsic may be NaN, got {k}")
    return k


def _on_device(t: Tensor, name: str, dev) -> Tensor:
    t = _check(t.contiguous(), name, _f32)
    if dev is not None and t.device != dev:
        raise RuntimeError(f"{name} must be on the device of the first argument, {dev}, got {t.device}")
    return t


class _GaussianNormals(Function):
    @staticmethod
    def forward(ctx, quats: Tensor, scales: Tensor, means: Tensor, viewmat: Tensor):
        _tensors(quats=quats, scales=scales, means=means, viewmat=viewmat)
        if quats.dim() != 2 or quats.shape[1] != 4:
            raise ValueError(f"expected quats [N,4], got {tuple(quats.shape)}")
        n = int(quats.shape[0])
        for name, t in (("scales", scales), ("means", means)):
            if tuple(t.shape) != (n, 3):
                raise ValueError(f"expected {name} [{n},3], got {tuple(t.shape)}")
        if viewmat.dim() != 2 or viewmat.shape[1] != 4 or viewmat.shape[0] not in (3, 4):
            raise ValueError(f"expected viewmat [3,4] (or [4,4], of which the top three rows are read), got "
                             f"{tuple(viewmat.shape)}")
        if 4 * n >= 2 ** 31:
            raise ValueError("quats must hold fewer than 2^31 elements")
        q = _on_device(quats.detach(), "quats", None)
        dev = q.device
        s = _on_device(scales.detach(), "scales", dev)
        m = _on_device(means.detach(), "means", dev)
        vm = _on_device(viewmat.detach()[:3], "viewmat", dev)
        with torch.cuda.device(dev):
            normals = torch.empty((n, 3), dtype=_f32, device=dev)
            axis = torch.empty((n,), dtype=torch.int32, device=dev)
            sign = torch.empty((n,), dtype=_f32, device=dev)
            _call("gsr_gaussian_normals_forward", n, q, s, m, vm, normals, axis, sign, _stream(dev))
        ctx.save_for_backward(q, vm, axis, sign)
        ctx.mark_non_differentiable(axis)
        return normals, axis

    @staticmethod
    def backward(ctx, v_normals, _v_axis):
        q, vm, axis, sign = ctx.saved_tensors
        n, dev = int(q.shape[0]), q.device
        v_normals = _check(v_normals.contiguous(), "v_normals", _f32)
        with torch.cuda.device(dev):
            v_quats = torch.empty_like(q)
            _call("gsr_gaussian_normals_backward", n, q, vm, axis, sign, v_normals, v_quats, _stream(dev))
        return v_quats, None, None, None


def gaussian_normals(quats: Tensor, scales: Tensor, means: Tensor, viewmat: Tensor, return_axis: bool = False):
    """The camera-facing normal of every Gaussian, [N,3]: the column of ``R(q / |q|)`` that belongs to the smallest of
    its three scales (a tie goes to the lowest axis index), rotated into camera space by ``viewmat`` (row-major [3,4],
    or [4,4] of which the top three rows are read) and negated where ``n . p_cam > 0``.  ``quats`` [N,4] are
    (w,x,y,z), raw: they are normalised inside the kernel.  Only the order of ``scales`` [N,3] is used, so log-scales
    and exp'd scales give the same result.  Differentiable w.r.t. ``quats`` only, through the normalisation and the
    rotation column: the choice of axis and the facing sign are piecewise constant, so ``scales``, ``means`` and
    ``viewmat`` get no gradient.  ``return_axis=True`` also returns the chosen axis, int32 [N]."""
    normals, axis = _GaussianNormals.apply(quats, scales, means, viewmat)
    return (normals, axis) if return_axis else normals


def _depth_alpha(depth, alpha):
    """-> (depth, alpha) as [H,W] views, shapes checked (no device or dtype check yet)."""
    d = _plane(depth, "depth")
    H, W = int(d.shape[0]), int(d.shape[1])
    a = _same_plane(alpha, "alpha", H, W)
    if 3 * H * W >= 2 ** 31:
        raise ValueError("the images must hold fewer than 2^31 elements")
    return d, a, H, W


@torch.no_grad()
def depth_to_normal(depth: Tensor, alpha: Tensor, fx: float, fy: float, cx: float, cy: float) -> Tensor:
    """The normal map of a rendered depth image, [H,W,3], for visualisation and export (no gradient; the loss forms
    the same normals inside its kernels).  With ``P(i,j) = ((j + 0.5 - cx) / fx * D, (i + 0.5 - cy) / fy * D, D)``:
    ``normalise((P(i+1,j) - P(i-1,j)) x (P(i,j+1) - P(i,j-1)))``, which is (0,0,-1) for a fronto-parallel plane -- it
    faces the camera like `gaussian_normals`.  An exact zero where the pixel is on the one-pixel border, where it or one
    of its four neighbours has ``alpha <= 0`` or a non-finite depth (the test is on alpha: the models fill
    ``alpha == 0`` pixels with ``depth.max()``), or where the cross product has zero or non-finite length.
    ``depth`` and ``alpha`` are [H,W] or [H,W,1]."""
    _tensors(depth=depth, alpha=alpha)
    d, a, H, W = _depth_alpha(depth, alpha)
    k = _intrinsics(fx, fy, cx, cy)
    d = _on_device(d, "depth", None)
    dev = d.device
    a = _on_device(a, "alpha", dev)
    with torch.cuda.device(dev):
        out = torch.empty((H, W, 3), dtype=_f32, device=dev)
        _call("gsr_depth_normals", H, W, k[0], k[1], k[2], k[3], d, a, out, _stream(dev))
    return out


class _Consistency(Function):
    @staticmethod
    def forward(ctx, normals_img: Tensor, depth: Tensor, alpha: Tensor, k, mask=None):
        _tensors(normals_img=normals_img, depth=depth, alpha=alpha)
        if mask is not None:
            _tensors(mask=mask)
        d_shape = depth.shape
        d, a, H, W = _depth_alpha(depth, alpha)
        if tuple(normals_img.shape) != (H, W, 3):
            raise ValueError(f"expected normals_img [{H},{W},3], got {tuple(normals_img.shape)}")
        if mask is not None and tuple(mask.shape) not in ((H, W), (H, W, 1)):
            raise ValueError(f"expected a mask [{H},{W}] or [{H},{W},1] for these images, got {tuple(mask.shape)}")
        k = _intrinsics(*k)
        nimg = _on_device(normals_img.detach(), "normals_img", None)
        dev = nimg.device
        d = _on_device(d.detach(), "depth", dev)
        a = _on_device(a.detach(), "alpha", dev)
        from .loss import _mask_arg

        m = None if mask is None else _mask_arg(mask, H, W, nimg)
        with torch.cuda.device(dev):
            work = torch.empty((workspace_doubles(H, W),), dtype=torch.float64, device=dev)
            loss = torch.empty((), dtype=_f32, device=dev)
            _call("gsr_normal_consistency_forward", H, W, k[0], k[1], k[2], k[3], nimg, d, a, m, work, loss, _stream(dev))
        ctx.save_for_backward(*((nimg, d, a) + (() if m is None else (m,))))
        ctx.k, ctx.d_shape = k, d_shape
        return loss

    @staticmethod
    def backward(ctx, v_loss):
        nimg, d, a, *masks = ctx.saved_tensors
        H, W = int(d.shape[0]), int(d.shape[1])
        dev, k = nimg.device, ctx.k
        up = v_loss.to(_f32).reshape(1).contiguous()
        with torch.cuda.device(dev):
            v_nimg = torch.empty_like(nimg)
            v_depth = torch.empty_like(d)
            _call("gsr_normal_consistency_backward", H, W, k[0], k[1], k[2], k[3], up, nimg, d, a,
                  masks[0] if masks else None, v_nimg, v_depth, _stream(dev))
        return v_nimg, v_depth.view(ctx.d_shape), None, None, None


def normal_consistency_loss(normals_img: Tensor, depth: Tensor, alpha: Tensor, fx: float, fy: float, cx: float,
                            cy: float, mask=None) -> Tensor:
    """``mean over ALL H W pixels of m (1 - alpha <normals_img, n_d>)`` with ``n_d`` the depth normal of
    `depth_to_normal` -- 2DGS / gsplat's ``1 - (normals * normals_from_depth * alpha.detach()).sum(-1)``, as a mean.
    ``normals_img`` [H,W,3] is the alpha-blended, un-normalised rendered normal image; ``depth`` and ``alpha`` are
    [H,W] or [H,W,1].  ``mask`` ([H,W] or [H,W,1]; float32, bool or uint8) is multiplied in and the mean stays over all
    pixels, as in the other heads; a pixel without a depth normal contributes ``m``.  One forward kernel that stages
    depth and alpha in LDS tiles with a one-pixel halo (the depth normal is never written) and a one-workgroup sum; the
    backward is one kernel that returns the gradients w.r.t. ``normals_img`` and ``depth``, the latter as a gather over
    a pixel's four neighbours' normals recomputed from a two-pixel halo (an exact zero where none of them is valid).
    ``alpha`` is a weight and gets no gradient."""
    return _Consistency.apply(normals_img, depth, alpha, (fx, fy, cx, cy), mask)
