"""float64 NumPy restatement of the co-gs depth regularisation (include/gsraster.h; the
reference's depth_gs.py:521-528 with `nearMean_map` and `l2_loss`) -- forward and gradient, the yardstick of
tests/test_depth_reg_host.py and tests/test_gpu_depth_reg.py."""
import numpy as np


def plus_sum(a: np.ndarray) -> np.ndarray:
    """Plus-shaped five-tap sum (centre, up, down, left, right) with zero padding."""
    p = np.pad(a, 1)
    return p[1:-1, 1:-1] + p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:]


def depth_reg(pred: np.ndarray, mask: np.ndarray):
    """-> (loss, d loss / d pred) in float64; `mask` and `pred > 0` are constants of the differentiation."""
    pred, mask = np.asarray(pred, np.float64), np.asarray(mask, np.float64)
    live = (pred > 0).astype(np.float64)
    m = mask * live
    inv = 1.0 / (plus_sum(m) + 1e-8)
    res = plus_sum(pred * m) * inv - pred * live
    g = 2.0 * res / pred.size
    return float((res ** 2).mean()), m * plus_sum(g * inv) - g * live

