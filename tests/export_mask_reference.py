"""NumPy restatement of the object mask of the toolkit's TSDF export (exporter/tsdf_fusion.py:105-130, 234-262), for
tests/test_export_mask_host.py and tests/test_gpu_export_masked.py: the gray value of an annotation image, the pixels
it keeps, and the bounding rectangle with a margin."""
import numpy as np


def gray_uint8(mask_rgb: np.ndarray) -> np.ndarray:
    """0.21 R + 0.72 G + 0.07 B in float64 (a uint8 channel times a Python float), left to right, cut to uint8."""
    gray = 0.21 * mask_rgb[:, :, 0] + 0.72 * mask_rgb[:, :, 1] + 0.07 * mask_rgb[:, :, 2]
    return gray.astype(np.uint8)


def bounding_box_mask(gray: np.ndarray, margin: int) -> np.ndarray:
    nonzero = np.argwhere(gray)
    if len(nonzero) == 0:
        raise ValueError("empty mask")
    y_min, x_min = nonzero.min(axis=0)
    y_max, x_max = nonzero.max(axis=0)
    y_min, y_max = max(y_min - margin, 0), min(y_max + margin, gray.shape[0] - 1)
    x_min, x_max = max(x_min - margin, 0), min(x_max + margin, gray.shape[1] - 1)
    out = np.zeros(gray.shape, bool)
    out[y_min:y_max + 1, x_min:x_max + 1] = True
    return out


def export_mask(mask: np.ndarray, bounding_box: bool = False, margin: int = 5) -> np.ndarray:
    gray = gray_uint8(mask) if mask.ndim == 3 else mask
    return bounding_box_mask(gray, margin) if bounding_box else gray != 0
