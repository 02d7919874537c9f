"""A training step's ground truth from an integer image cache.  The toolkit's datamanager
keeps every image as float32 on the device (12-16 B per pixel) and `get_gt_img` (vanilla_gs.py:859-881) converts,
resizes and composites it every step; here the images stay uint8 (3-4 B per pixel) and one HIP kernel
(csrc/target.hip, `gsr_target_from_u8` / `gsr_plane_from_int`; the rule is stated in include/gsraster.h) forms the
step's target from them.  torch for memory and streams only; no CPU path; nothing is differentiated.
"""
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from rasterizer.cuda import _call, _on, _stream

_f32, _u8 = torch.float32, torch.uint8
_u16 = getattr(torch, "uint16", None)
# 16-bit planes: torch.uint16 where this torch has it, and int16 holding the same bits (what a tensor of an older
# torch, or one that was indexed, can be): the kernel reads the 16 bits as unsigned either way
_PLANE_DTYPES = {_u8: 1, torch.int16: 2, **({} if _u16 is None else {_u16: 2})}


def _source(t, name: str, dims: int) -> Tensor:
    if not isinstance(t, Tensor):
        raise ValueError(f"{name} must be a tensor")
    if not t.is_cuda:
        raise ValueError(f"{name} must be on the GPU (got a {t.device.type} tensor): there is no CPU path")
    if t.dim() != dims:
        raise ValueError(f"{name} must have {dims} dimensions, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def _out_hw(out_hw, H: int, W: int) -> Tuple[int, int]:
    try:
        h, w = (int(v) for v in out_hw)
    except (TypeError, ValueError):
        raise ValueError(f"out_hw must be (h, w), got {out_hw!r}") from None
    if not (1 <= h <= H and 1 <= w <= W):
        raise ValueError(f"out_hw {(h, w)} must be at least (1, 1) and at most the source's {(H, W)}")
    return h, w


def _out(out: Optional[Tensor], shape: Tuple[int, ...], dev) -> Tensor:
    if out is None:
        return torch.empty(shape, dtype=_f32, device=dev)
    if not isinstance(out, Tensor) or out.dtype != _f32 or out.device != dev or tuple(out.shape) != shape:
        raise ValueError(f"out must be a float32 tensor of shape {shape} on {dev}")
    if not out.is_contiguous():
        raise ValueError("out must be contiguous (a slice of a larger tensor is not written into)")
    return out


def target_from_u8(image_u8: Tensor, background: Optional[Tensor], out_hw: Sequence[int],
                   out: Optional[Tensor] = None) -> Tensor:
    """uint8 [H,W,C], C in (3, 4) -> float32 [h,w,3]: `u8 / 255`, bilinear resize to `out_hw` = (h, w) (no
    antialiasing, align_corners=False, alpha included), and for C = 4 `alpha * rgb + (1 - alpha) * background` from the
    resized RGBA -- `get_gt_img` in one launch on the current stream.  `background`: float32 [3] on the image's device
    (never read back); may be None for C = 3.  `out`: written in place and returned (a HIP graph's static target)."""
    img = _source(image_u8, "image_u8", 3)
    if img.dtype != _u8:
        raise ValueError(f"image_u8 must have dtype torch.uint8, got {img.dtype}")
    H, W, Cn = img.shape
    if Cn not in (3, 4):
        raise ValueError(f"image_u8 must have 3 or 4 channels, got {Cn}")
    dev = img.device
    if background is None:
        if Cn == 4:
            raise ValueError("background is needed for an image with an alpha channel")
    else:
        if not isinstance(background, Tensor) or background.dtype != _f32 or tuple(background.shape) != (3,) \
                or not background.is_contiguous():
            raise ValueError("background must be a contiguous float32 tensor of shape (3,)")
        if background.device != dev:
            raise ValueError(f"background must be on the image's device {dev}, got {background.device}")
    h, w = _out_hw(out_hw, H, W)
    with _on(dev):
        out = _out(out, (h, w, 3), dev)
        _call("gsr_target_from_u8", img, H, W, Cn, background, h, w, out, _stream(dev))
    return out


def plane_from_int(plane: Tensor, unit: float, out_hw: Sequence[int], out: Optional[Tensor] = None) -> Tensor:
    """uint8 or uint16 [H,W] -> float32 [h,w]: `float32(value) * float32(unit)`, then `target_from_u8`'s resize.
    Masks (uint8 0/1, unit 1), sensor depth (uint16 millimetres, unit 1e-3), monocular depth (uint8, unit 1/255);
    zeros are interpolated like any other value."""
    p = _source(plane, "plane", 2)
    size = _PLANE_DTYPES.get(p.dtype)
    if size is None:
        raise ValueError(f"plane must have dtype torch.uint8 or torch.uint16, got {p.dtype}")
    H, W = p.shape
    h, w = _out_hw(out_hw, H, W)
    dev = p.device
    with _on(dev):
        out = _out(out, (h, w), dev)
        _call("gsr_plane_from_int", p, size, H, W, float(unit), h, w, out, _stream(dev))
    return out


class DeferredTarget:
    """A target that is written straight into its destination: `shape`, and `write(out)` fills a float32 tensor of
    that shape.  `gs_fused.render.ViewGraph` calls it on its static target instead of copying one in."""

    def __init__(self, shape: Tuple[int, ...], write):
        self.shape, self.write = torch.Size(shape), write


def _upload(host, device, dtype=None) -> Tensor:
    """One `copy_` from pinned memory, in the file's integer dtype: no float copy on either side."""
    t = host if isinstance(host, Tensor) else torch.from_numpy(host)
    if dtype is not None and t.dtype != dtype:
        t = t.view(dtype)
    if t.device == device:
        return t.contiguous()
    dst = torch.empty(t.shape, dtype=t.dtype, device=device)
    if device.type == "cuda":
        t = t.contiguous().pin_memory()
    dst.copy_(t, non_blocking=False)
    return dst


class ImageCache:
    """The per-view store of a dataset on the device: uint8 images [H,W,3|4], optional uint8 0/1 masks [H,W] and
    optional integer depth [H,W] (uint16 with `depth_unit` 1e-3: millimetres; uint8 with 1/255: monocular), as the
    files hold them.  `target` forms a step's ground truth from them; only what does not depend on the step and is small
    is cached as floats: the resized mask and depth per (view, factor)."""

    def __init__(self, images: Sequence, masks: Optional[Sequence] = None, depths: Optional[Sequence] = None,
                 depth_unit=1e-3, device=None):
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self.images: List[Tensor] = [_upload(i, device) for i in images]
        if not self.images:
            raise ValueError("an ImageCache needs at least one image")
        for i, t in enumerate(self.images):
            if t.dtype != _u8 or t.dim() != 3 or t.shape[2] not in (3, 4):
                raise ValueError(f"image {i} must be uint8 [H,W,3|4], got {t.dtype} {tuple(t.shape)}")
            if t.shape != self.images[0].shape:
                raise ValueError(f"image {i} is {tuple(t.shape)}, image 0 is {tuple(self.images[0].shape)}")
        self.height, self.width, self.channels = (int(v) for v in self.images[0].shape)
        self.masks = self._planes(masks, "mask", (_u8,))
        self.depths = self._planes(depths, "depth", tuple(_PLANE_DTYPES))
        n = len(self.images)
        units = [float(depth_unit)] * n if isinstance(depth_unit, (int, float)) else [float(u) for u in depth_unit]
        if len(units) != n:
            raise ValueError(f"depth_unit must be one number or one per view ({n}), got {len(units)}")
        self.depth_units = units
        self._mask_cache: Dict[Tuple[int, int], Tensor] = {}
        self._depth_cache: Dict[Tuple[int, int], Tensor] = {}

    def _planes(self, planes, name: str, dtypes) -> Optional[List[Tensor]]:
        if planes is None:
            return None
        planes = [_upload(p, self.device) for p in planes]
        if len(planes) != len(self.images):
            raise ValueError(f"{len(planes)} {name}s for {len(self.images)} images")
        for i, t in enumerate(planes):
            if t.dtype not in dtypes or tuple(t.shape) != (self.height, self.width):
                raise ValueError(f"{name} {i} must be an integer plane {(self.height, self.width)}, got {t.dtype} "
                                 f"{tuple(t.shape)}")
        return planes

    def __len__(self) -> int:
        return len(self.images)

    @property
    def nbytes(self) -> int:
        """Bytes of the integer store (the resized float planes of `mask` / `depth` are not counted)."""
        every = self.images + (self.masks or []) + (self.depths or [])
        return sum(t.numel() * t.element_size() for t in every)

    def size(self, d: int) -> Tuple[int, int]:
        return self.height // d, self.width // d

    def target(self, view: int, d: int, background: Optional[Tensor], out: Optional[Tensor] = None) -> Tensor:
        """float32 [H // d, W // d, 3]: view `view` at downscale factor `d` over `background` (one launch)."""
        return target_from_u8(self.images[view], background, self.size(d), out=out)

    def deferred_target(self, view: int, d: int, background: Optional[Tensor]) -> DeferredTarget:
        h, w = self.size(d)
        return DeferredTarget((h, w, 3), lambda out: self.target(view, d, background, out=out))

    def mask(self, view: int, d: int) -> Optional[Tensor]:
        """float32 [H // d, W // d, 1] (fractional along the edges for d > 1, as the reference's resize leaves it)."""
        if self.masks is None:
            return None
        m = self._mask_cache.get((view, d))
        if m is None:
            m = self._mask_cache[(view, d)] = plane_from_int(self.masks[view], 1.0, self.size(d))[..., None]
        return m

    def depth(self, view: int, d: int) -> Optional[Tensor]:
        """float32 [H // d, W // d] in the dataset's units; 0 = no measurement (interpolated like any value)."""
        if self.depths is None:
            return None
        z = self._depth_cache.get((view, d))
        if z is None:
            z = self._depth_cache[(view, d)] = plane_from_int(self.depths[view], self.depth_units[view], self.size(d))
        return z
