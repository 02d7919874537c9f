"""float64 NumPy restatement of the three monocular-depth terms of the co-gs loss (include/gsraster.h, DESIGN.md
section 4.11; the reference's utils/losses.py:26-45, 197-207 and depth_gs.py:492-519) -- values and gradients w.r.t. the
predicted depth, per-view masks included -- the yardstick of tests/test_mono_depth_host.py, tests/test_gpu_mono_depth.py
and tests/test_gpu_cogs_mono_depth.py.

A mask is multiplied in as the model does it, in float32 (`pred * mask`, `gt * mask`, depth_gs.py:424-437): `products`
forms them; every function below takes the PRODUCTS plus, for the gradient's chain rule, the mask itself."""
import numpy as np


def products(pred, gt, mask):
    """-> (pred * mask, gt * mask) as float32 products (what the heads form inside their kernels), in float64."""
    m = np.asarray(mask).reshape(np.asarray(pred).shape).astype(np.float32)
    p, g = np.asarray(pred, np.float32) * m, np.asarray(gt, np.float32) * m
    return p.astype(np.float64), g.astype(np.float64)


def _chain(grad, mask):
    return grad if mask is None else grad * np.asarray(mask, np.float64).reshape(grad.shape)


def _valid(r, c, H, W, box):
    return 0 <= r <= H - box and 0 <= c <= W - box


def local_pearson_loop(src, tgt, box, rows, cols):
    """The source's loop over patches, literally (utils/losses.py:26-45 with pearson_depth_loss, :12-23): the value
    only.  A corner outside the image is NaN (the source would slice a smaller patch or fail; the heads do not read)."""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    H, W = src.shape
    total = 0.0
    with np.errstate(all="ignore"):
        for r, c in zip(np.asarray(rows).tolist(), np.asarray(cols).tolist()):
            if not _valid(r, c, H, W, box):
                total += np.nan
                continue
            a = src[r:r + box, c:c + box].reshape(-1)
            b = tgt[r:r + box, c:c + box].reshape(-1)
            cov = ((a - a.mean()) * (b - b.mean())).mean()
            total += 1 - cov / (np.std(a, ddof=1) * np.std(b, ddof=1))
        return float(np.float64(total) / np.float64(len(np.asarray(rows))))


def local_pearson(src, tgt, box, rows, cols, mask=None):
    """-> (loss, d loss / d pred) by the closed form: per patch of n = box^2 pixels with centred sums S_ss, S_tt, S_st
        loss_p = 1 - (n - 1) / n * S_st / sqrt(S_ss S_tt)
        d loss / d s_i = -(A / n_corr) ((t_i - m_t) - B (s_i - m_s)),  A = (n - 1) / (n sqrt(S_ss S_tt)),  B = S_st / S_ss
    (the mean-centring terms cancel), summed over the patches in ascending index.  `src`, `tgt`: the (masked) images."""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    H, W = src.shape
    rows, cols = np.asarray(rows).tolist(), np.asarray(cols).tolist()
    n_corr, n = len(rows), box * box
    grad = np.zeros((H, W))
    total = 0.0
    with np.errstate(all="ignore"):
        for r, c in zip(rows, cols):
            if not _valid(r, c, H, W, box):
                total += np.nan
                continue
            a, b = src[r:r + box, c:c + box], tgt[r:r + box, c:c + box]
            da, db = a - a.mean(), b - b.mean()
            sss, stt, sst = (da * da).sum(), (db * db).sum(), (da * db).sum()
            root = np.sqrt(sss * stt)
            total += 1 - np.float64(n - 1) / n * sst / root
            A, B = np.float64(n - 1) / (n * root), sst / sss
            grad[r:r + box, c:c + box] += A * (B * da - db)
        grad = grad / np.float64(n_corr)
        if n_corr == 0:
            grad[:] = np.nan  # 0 / 0, as the loss
        return float(np.float64(total) / np.float64(n_corr)), _chain(grad, mask)


def _edge_weights(img):
    img = np.asarray(img, np.float64)
    lx = np.exp(-np.abs(img[:, :-1] - img[:, 1:]).mean(-1))
    ly = np.exp(-np.abs(img[:-1] - img[1:]).mean(-1))
    return lx, ly


def _mean(a):
    return float(a.sum() / np.float64(a.size)) if a.size else float("nan")  # (torch: the mean of an empty tensor)


def log_depth(pred, gt, img, scale=1.0, shift=0.0, mask=None):
    """-> (loss, d loss / d pred): depth_gs.py:492-519.  `pred`, `gt`: the (masked) depths."""
    pred, gt = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    H, W = pred.shape
    scale, shift = float(scale), float(shift)
    e = scale * pred + shift - gt
    l = np.log(1 + np.abs(e))
    lx, ly = _edge_weights(img)
    loss = _mean(lx * l[:, :-1]) + _mean(ly * l[:-1])
    w = np.zeros((H, W))
    if W > 1:
        w[:, :-1] += lx / (H * (W - 1))
    if H > 1:
        w[:-1] += ly / ((H - 1) * W)
    return loss, _chain(scale * np.sign(e) / (1 + np.abs(e)) * w, mask)


def tv(pred, mask=None):
    """-> (loss, d loss / d pred): utils/losses.py:197-207 on the [H,W] (masked) depth."""
    pred = np.asarray(pred, np.float64)
    H, W = pred.shape
    dx, dy = pred[:, :-1] - pred[:, 1:], pred[:-1] - pred[1:]
    loss = _mean(np.abs(dx)) + _mean(np.abs(dy))
    grad = np.zeros((H, W))
    if W > 1:
        s = np.sign(dx) / (H * (W - 1))
        grad[:, :-1] += s
        grad[:, 1:] -= s
    if H > 1:
        s = np.sign(dy) / ((H - 1) * W)
        grad[:-1] += s
        grad[1:] -= s
    return loss, _chain(grad, mask)


def smooth_noise(H, W, seed, noise=0.05):
    """-> (pred, gt, img) float32: smooth surfaces plus noise, so that no patch is constant and no difference is an
    exact tie unless a test makes one."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    base = 3.0 + 0.6 * np.sin(0.11 * x + rng.uniform(0, 6)) * np.cos(0.07 * y + rng.uniform(0, 6)) + 0.004 * (x - y)
    gt = (base + noise * rng.normal(size=(H, W))).astype(np.float32)
    pred = (0.8 * base + 0.4 + 0.2 * np.sin(0.05 * (x + 2 * y)) + noise * rng.normal(size=(H, W))).astype(np.float32)
    img = (0.5 + 0.3 * np.sin(0.09 * x[..., None] + np.arange(3)) * np.cos(0.13 * y[..., None])
           + 0.1 * rng.uniform(size=(H, W, 3))).astype(np.float32)
    return pred, gt, img
