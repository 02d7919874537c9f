"""Per-view bilateral grids: appearance compensation between the render and the loss heads, on csrc/bilagrid.hip
(the rule is stated in include/gsraster.h).  What `use_bilateral_grid` of gsplat / splatfacto
does with `lib_bilagrid`: every training view owns a small 3-D grid of 3x4 affine colour maps, a rendered pixel is
mapped by the grid's value at (its position, its brightness), and a total-variation term keeps the grids smooth.

    bilagrid_slice(grids, rgb, view)      the mapped image; gradients to the grids and to rgb
    bilagrid_tv_loss(grids)               sum over the three grid axes of mean(squared forward difference)
    BilateralGrids(num_views, ...)        the nn.Module that owns the parameter

`grids` is [V,L,Gh,Gw,12] float32, channel last (gsplat stores [V,12,L,Gh,Gw]: `to_gsplat` / `from_gsplat`).  float32
per-pixel arithmetic, float64 sums over pixels in a fixed order without atomics: two runs are bit-equal.  CUDA tensors
only; no CPU fallback."""

import torch
from torch import Tensor
from torch.autograd import Function

from rasterizer.cuda import _call, _check, _stream

_f32 = torch.float32
CHANNELS = 12               # GSR_BILAGRID_CHANNELS (include/gsraster.h)
MAX_XY, MAX_L = 64, 16      # GSR_BILAGRID_MAX_XY, GSR_BILAGRID_MAX_L
TV_WORKSPACE_DOUBLES = 3072  # GSR_BILAGRID_TV_WORKSPACE_DOUBLES
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def strips(grid_w: int, grid_h: int) -> int:
    """GSR_BILAGRID_STRIPS."""
    n = grid_w * grid_h
    return 1 if n >= 2048 else (64 if n <= 32 else 2048 // n)


def workspace_doubles(grid_w: int, grid_h: int, grid_l: int) -> int:
    """GSR_BILAGRID_WORKSPACE_DOUBLES."""
    return strips(grid_w, grid_h) * grid_w * grid_h * grid_l * CHANNELS


def check_grid_shape(grid_w: int, grid_h: int, grid_l: int) -> None:
    """ValueError naming the argument for a grid dimension below 2, `grid_w` / `grid_h` above 64 or `grid_l` above 16."""
    for name, v, hi in (("grid_w", grid_w, MAX_XY), ("grid_h", grid_h, MAX_XY), ("grid_l", grid_l, MAX_L)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{name} must be an integer, got {v!r}")
        if v < 2 or v > hi:
            raise ValueError(f"{name} must be in [2, {hi}], got {v}")


def _grids_arg(grids, check_device: bool = True) -> Tensor:
    """The argument checks in the order ValueError (shape) before RuntimeError (device, dtype)."""
    if not isinstance(grids, Tensor):
        raise RuntimeError("grids must be a tensor")
    if grids.dim() != 5 or grids.shape[-1] != CHANNELS or grids.shape[0] < 1:
        raise ValueError(f"expected grids [V,L,Gh,Gw,{CHANNELS}], got {tuple(grids.shape)}")
    check_grid_shape(int(grids.shape[3]), int(grids.shape[2]), int(grids.shape[1]))
    if grids.numel() >= 2 ** 31:
        raise ValueError("grids must hold fewer than 2^31 elements")
    return _check(grids.contiguous(), "grids", _f32) if check_device else grids


def _dims(g: Tensor):
    return int(g.shape[0]), int(g.shape[3]), int(g.shape[2]), int(g.shape[1])  # V, Gw, Gh, L


class _Slice(Function):
    @staticmethod
    def forward(ctx, grids: Tensor, rgb: Tensor, view: int):
        if not isinstance(rgb, Tensor):
            raise RuntimeError("rgb must be a tensor")
        if rgb.dim() != 3 or rgb.shape[-1] != 3 or rgb.numel() == 0:
            raise ValueError(f"expected rgb [H,W,3], non-empty, got {tuple(rgb.shape)}")
        V, gw, gh, gl = _dims(_grids_arg(grids, check_device=False))
        if isinstance(view, bool) or not isinstance(view, int):
            raise ValueError(f"view must be a host integer, got {view!r}")
        if view < 0 or view >= V:
            raise ValueError(f"view must be in [0, {V}), got {view}")
        g = _grids_arg(grids)
        x = _check(rgb.contiguous(), "rgb", _f32)
        if x.device != g.device:
            raise RuntimeError(f"rgb must be on the grids' device {g.device}, got {x.device}")
        H, W = int(x.shape[0]), int(x.shape[1])
        if 3 * H * W >= 2 ** 31:
            raise ValueError("rgb must hold fewer than 2^31 elements")
        dev = g.device
        with torch.cuda.device(dev):
            out = torch.empty_like(x)
            _call("gsr_bilagrid_slice_forward", H, W, V, view, gw, gh, gl, g, x, out, _stream(dev))
        ctx.save_for_backward(g, x)
        ctx.view = view
        return out

    @staticmethod
    def backward(ctx, v_out):
        g, x = ctx.saved_tensors
        V, gw, gh, gl = _dims(g)
        H, W = int(x.shape[0]), int(x.shape[1])
        dev = g.device
        v_out = _check(v_out.contiguous(), "v_out", _f32)
        with torch.cuda.device(dev):
            work = torch.empty((workspace_doubles(gw, gh, gl),), dtype=torch.float64, device=dev)
            v_rgb = torch.empty_like(x)
            v_grids = torch.empty_like(g)
            _call("gsr_bilagrid_slice_backward", H, W, V, ctx.view, gw, gh, gl, g, x, v_out, work, v_rgb, v_grids,
                  _stream(dev))
        return v_grids, v_rgb, None


def bilagrid_slice(grids: Tensor, rgb: Tensor, view: int) -> Tensor:
    """``rgb`` [H,W,3] mapped by view ``view``'s grid: per pixel the 3x4 affine map interpolated trilinearly at
    ``((px + 0.5) / W, (py + 0.5) / H, clamp(0.299 r + 0.587 g + 0.114 b, 0, 1))`` -- `F.grid_sample(..., "bilinear",
    align_corners=True, padding_mode="border")` + the affine map, one kernel.  The backward writes the whole grid
    gradient (exact zeros for the other views and for vertices no pixel reaches) from a per-vertex gather with float64
    sums in pixel order, and the ``rgb`` gradient including the path through the guide (zero where the guide is
    clamped).  ``view`` is a host integer; outside ``[0, V)`` raises ValueError."""
    return _Slice.apply(grids, rgb, view)


class _TV(Function):
    @staticmethod
    def forward(ctx, grids: Tensor):
        g = _grids_arg(grids)
        V, gw, gh, gl = _dims(g)
        dev = g.device
        with torch.cuda.device(dev):
            work = torch.empty((TV_WORKSPACE_DOUBLES,), dtype=torch.float64, device=dev)
            loss = torch.empty((), dtype=_f32, device=dev)
            _call("gsr_bilagrid_tv_forward", V, gw, gh, gl, g, work, loss, _stream(dev))
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, v_loss):
        (g,) = ctx.saved_tensors
        V, gw, gh, gl = _dims(g)
        dev = g.device
        up = v_loss.to(_f32).reshape(1).contiguous()
        with torch.cuda.device(dev):
            v_grids = torch.empty_like(g)
            _call("gsr_bilagrid_tv_backward", V, gw, gh, gl, up, g, v_grids, _stream(dev))
        return v_grids


def bilagrid_tv_loss(grids: Tensor) -> Tensor:
    """``sum over the axes L, Gh, Gw of mean((A[.. i+1 ..] - A[.. i ..])^2)``, each mean over all difference elements of
    that axis across views and channels (gsplat's `total_variation_loss`): one streaming kernel each way over all
    views, float64 sums in a fixed order."""
    return _TV.apply(grids)


def lr_schedule(step: int, lr0: float, max_steps: int) -> float:
    """gsplat's schedule for the grids: a linear warm-up from 1 % over 1000 steps, chained with an exponential decay to
    1 % at ``max_steps``: ``lr0 * min(1, 0.01 + 0.99 * step / 1000) * 0.01 ** (step / max_steps)``."""
    return lr0 * min(1.0, 0.01 + 0.99 * step / 1000.0) * 0.01 ** (step / max(max_steps, 1))


def identity_grids(num_views: int, grid_w: int = 16, grid_h: int = 16, grid_l: int = 8, device=None) -> Tensor:
    """[V,L,Gh,Gw,12] with the identity map at every vertex."""
    if isinstance(num_views, bool) or not isinstance(num_views, int) or num_views < 1:
        raise ValueError(f"num_views must be a positive integer, got {num_views!r}")
    check_grid_shape(grid_w, grid_h, grid_l)
    eye = torch.tensor(IDENTITY, dtype=_f32, device=device)
    return eye.repeat(num_views, grid_l, grid_h, grid_w, 1).contiguous()


class BilateralGrids(torch.nn.Module):
    """One grid per training view, as ONE parameter ``grids`` [V,L,Gh,Gw,12] initialised to the identity map."""

    def __init__(self, num_views: int, grid_w: int = 16, grid_h: int = 16, grid_l: int = 8, device=None):
        super().__init__()
        self.grids = torch.nn.Parameter(identity_grids(num_views, grid_w, grid_h, grid_l, device))

    @property
    def num_views(self) -> int:
        return int(self.grids.shape[0])

    @property
    def shape(self):
        """(grid_w, grid_h, grid_l)"""
        return int(self.grids.shape[3]), int(self.grids.shape[2]), int(self.grids.shape[1])

    def slice(self, rgb: Tensor, view: int) -> Tensor:
        return bilagrid_slice(self.grids, rgb, view)

    def tv_loss(self) -> Tensor:
        return bilagrid_tv_loss(self.grids)

    def to_gsplat(self) -> Tensor:
        """The grids in the layout of gsplat's `BilateralGrid.grids`: [V,12,L,Gh,Gw] (a contiguous copy)."""
        return self.grids.detach().permute(0, 4, 1, 2, 3).contiguous()

    @torch.no_grad()
    def from_gsplat(self, grids: Tensor) -> "BilateralGrids":
        """Take the values of a [V,12,L,Gh,Gw] tensor (a gsplat checkpoint's `grids`) of this module's shape."""
        want = (self.grids.shape[0], CHANNELS) + tuple(self.grids.shape[1:4])
        if not isinstance(grids, Tensor) or tuple(grids.shape) != want:
            raise ValueError(f"expected grids {want}, got {tuple(grids.shape) if isinstance(grids, Tensor) else grids!r}")
        self.grids.copy_(grids.permute(0, 2, 3, 4, 1).to(self.grids.dtype))
        return self
