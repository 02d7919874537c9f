"""NumPy restatements of gs_fused.target_from_u8 / plane_from_int (include/gsraster.h, "targets from an integer image
cache"): a float32 one that performs the kernel's operations in the kernel's order, every one rounded on its own
(NumPy float32 arithmetic is correctly rounded, division included), and a float64 one of the same rule."""
import numpy as np

f32 = np.float32


def axis_taps(n_in: int, n_out: int, dtype=f32):
    """-> (i0, i1, l0, l1) per output index: s = max(scale * (dst + 0.5) - 0.5, 0), scale = float(in) / float(out)."""
    t = dtype
    scale = t(n_in) / t(n_out)
    dst = np.arange(n_out).astype(t)
    s = scale * (dst + t(0.5)) - t(0.5)
    s = np.where(s < t(0), t(0), s).astype(t)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (s - i0.astype(t)).astype(t)
    l0 = (t(1) - l1).astype(t)
    return i0, i1, l0, l1


def resize(v: np.ndarray, out_hw, dtype=f32) -> np.ndarray:
    """v [H,W] or [H,W,C] of `dtype` -> [h,w(,C)]: ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
    out == in: v itself (one tap)."""
    H, W = v.shape[:2]
    h, w = out_hw
    assert v.dtype == dtype
    if (h, w) == (H, W):
        return v.copy()
    y0, y1, ly0, ly1 = axis_taps(H, h, dtype)
    x0, x1, lx0, lx1 = axis_taps(W, w, dtype)
    tail = (1,) * (v.ndim - 2)
    lx0, lx1 = lx0.reshape((1, w) + tail), lx1.reshape((1, w) + tail)
    ly0, ly1 = ly0.reshape((h, 1) + tail), ly1.reshape((h, 1) + tail)
    r0, r1 = v[y0], v[y1]
    top = lx0 * r0[:, x0] + lx1 * r0[:, x1]
    bot = lx0 * r1[:, x0] + lx1 * r1[:, x1]
    out = ly0 * top + ly1 * bot
    assert out.dtype == dtype
    return out


def target_from_u8(image_u8: np.ndarray, background, out_hw, dtype=f32) -> np.ndarray:
    assert image_u8.dtype == np.uint8 and image_u8.ndim == 3 and image_u8.shape[2] in (3, 4)
    v = image_u8.astype(dtype) / dtype(255)
    v = resize(v, out_hw, dtype)
    if v.shape[2] == 3:
        return v
    bg = np.asarray(background, dtype).reshape(1, 1, 3)
    a = v[..., 3:4]
    na = dtype(1) - a
    out = a * v[..., :3] + na * bg
    assert out.dtype == dtype
    return out


def plane_from_int(plane: np.ndarray, unit, out_hw, dtype=f32) -> np.ndarray:
    """`unit` is taken as a float32 first in both precisions: that is the number the kernel is given."""
    assert plane.dtype in (np.uint8, np.uint16) and plane.ndim == 2
    return resize(plane.astype(dtype) * dtype(f32(unit)), out_hw, dtype)
