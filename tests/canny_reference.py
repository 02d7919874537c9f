"""NumPy + SciPy restatement of the Canny rule of include/gsraster.h -- the oracle of
tests/test_canny_host.py and tests/test_gpu_canny.py.  Padded array slices for the stencils and
`scipy.ndimage.label` for the hysteresis: no sort, no union-find, no tiles -- nothing it shares with the kernels.

The rule restates OpenCV's `cv::Canny(img8, thres1, thres2)` (aperture 3, L1 gradient).  OpenCV is not available
where these tests run, so nothing here is pinned against OpenCV itself: this file checks the kernels against the
written rule, and the written rule against hand-worked cases.
"""
import numpy as np
from scipy import ndimage


def to_u8(image: np.ndarray) -> np.ndarray:
    """(uint8)trunc(x * 255.0f), the product in float32; out-of-range products saturate, NaN gives 0."""
    t = np.asarray(image, np.float32) * np.float32(255.0)
    t = np.where(np.isnan(t), np.float32(0), np.clip(t, np.float32(0), np.float32(255)))
    return np.trunc(t).astype(np.uint8)


def thresholds(thres1, thres2):
    low, high = int(np.floor(thres1)), int(np.floor(thres2))
    return (high, low) if low > high else (low, high)


def gradient(u8: np.ndarray):
    """-> (mag, dx, dy) int32 [H,W]: 3x3 Sobel with a replicate border per channel, then per pixel the channel with
    the largest |dx| + |dy| (the lowest index on ties)."""
    p = np.pad(u8.astype(np.int32), ((1, 1), (1, 1), (0, 0)), mode="edge")
    dx = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    dy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    norm = np.abs(dx) + np.abs(dy)
    k = np.argmax(norm, axis=-1)[..., None]  # (the first maximum)
    take = lambda a: np.take_along_axis(a, k, axis=-1)[..., 0]
    return take(norm), take(dx), take(dy)


def candidates(mag: np.ndarray, dx: np.ndarray, dy: np.ndarray, low: int, high: int):
    """Non-maximum suppression -> (candidate map, strong map), bool [H,W]."""
    mp = np.pad(mag, 1)  # mag outside the image is 0
    left, right = mp[1:-1, :-2], mp[1:-1, 2:]
    above, below = mp[:-2, 1:-1], mp[2:, 1:-1]
    x, y = np.abs(dx).astype(np.int64), np.abs(dy).astype(np.int64) << 15
    t22 = x * 13573
    t67 = t22 + (x << 16)
    horizontal = (mag > left) & (mag >= right)
    vertical = (mag > above) & (mag >= below)
    same_sign = (mag > mp[:-2, :-2]) & (mag > mp[2:, 2:])      # s = +1: (row-1, col-1), (row+1, col+1)
    opposite = (mag > mp[:-2, 2:]) & (mag > mp[2:, :-2])       # s = -1: (row-1, col+1), (row+1, col-1)
    diagonal = np.where(np.bitwise_xor(dx, dy) < 0, opposite, same_sign)
    cand = (mag > low) & np.where(y < t22, horizontal, np.where(y > t67, vertical, diagonal))
    return cand, cand & (mag > high)


def canny_maps(image: np.ndarray, thres1=50, thres2=150):
    """-> (edges uint8 [H,W] 255 / 0, candidate map bool, strong map bool) of a float [H,W,3] image."""
    image = np.asarray(image)
    assert image.ndim == 3 and image.shape[-1] == 3, image.shape
    H, W = image.shape[:2]
    if H * W == 0:
        e = np.zeros((H, W), bool)
        return e.astype(np.uint8), e, e.copy()
    low, high = thresholds(thres1, thres2)
    cand, strong = candidates(*gradient(to_u8(image)), low, high)
    labels, n = ndimage.label(cand, structure=np.ones((3, 3), np.int32))
    kept = np.zeros(n + 1, bool)
    kept[labels[strong]] = True
    kept[0] = False
    edges = kept[labels] & cand
    return (edges * np.uint8(255)).astype(np.uint8), cand, strong


def canny(image: np.ndarray, thres1=50, thres2=150) -> np.ndarray:
    return canny_maps(image, thres1, thres2)[0]


def image2canny(image: np.ndarray, thres1, thres2, isEdge1=True) -> np.ndarray:
    e = (canny(image, thres1, thres2) / 255.0).astype(np.float32)
    return e if isEdge1 else (1.0 - e).astype(np.float32)


# ---- images the host and GPU tests share ----------------------------------------------------------------------------
def grey(levels: np.ndarray) -> np.ndarray:
    """[H,W] integer grey levels -> float32 [H,W,3] whose uint8 conversion gives exactly those levels ((k + 0.5) / 255
    sits in the middle of level k's interval, away from the truncation's borders)."""
    g = ((np.asarray(levels, np.float64) + 0.5) / 255.0).astype(np.float32)
    return np.repeat(g[..., None], 3, axis=-1)


def two_line_levels() -> np.ndarray:
    """70 x 300, filled with 100; rows >= 20 plus 20; rows >= 50 plus 20; rows < 20 of columns 0-2 minus 40: two
    weak horizontal lines (steps of 20 grey levels), the upper one with a strong head at its left end."""
    lv = np.full((70, 300), 100, np.int32)
    lv[20:] += 20
    lv[50:] += 20
    lv[:20, :3] -= 40
    return lv


def smooth_random(height=65, width=127, seed=0) -> np.ndarray:
    """Uniform noise, Gaussian-filtered with sigma (2, 2, 0), rescaled to [0, 1]: float32 [H,W,3]."""
    x = np.random.default_rng(seed).uniform(size=(height, width, 3))
    x = ndimage.gaussian_filter(x, sigma=(2, 2, 0))
    x = (x - x.min()) / (x.max() - x.min())
    return x.astype(np.float32)


def ring_levels(size=200) -> np.ndarray:
    """Concentric rings, 8 pixels wide, of contrast 20 (their borders are weak: mag 80 at the most) around the centre.
    On every second border a 3 x 4 pixel notch just inside it, above the centre, raises the step across the border to
    60 (strong): those borders are kept as wholes, the others dropped as wholes -- components that wind through many
    tiles."""
    yy, xx = np.mgrid[:size, :size]
    c = (size - 1) / 2.0
    r = np.sqrt((yy - c) ** 2 + (xx - c) ** 2)
    band = (r // 8).astype(np.int32)
    lv = 100 + 20 * (band % 2)
    cx = int(c)
    for b in range(2, int(band.max()) + 1, 2):  # the border between band b - 1 and band b
        notch = (np.abs(xx - cx) <= 1) & (yy < c) & (r >= 8 * b - 4) & (r < 8 * b)
        lv[notch] += 40  # (b is even: band b - 1 is the brighter of the two, 120 against 100)
    return lv
