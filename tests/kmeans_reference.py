"""Restatements of the k-means kernels (include/gsraster.h, gsr_kmeans_assign / _update / _inertia; DESIGN.md section
4.24) and of the codec of gs_io.compressed, and the case builders of tests/test_kmeans_host.py and
tests/test_gpu_kmeans.py.

`assign` is the assignment rule in float32 NumPy, every operation rounded on its own in the order the header writes
it: what the kernel must produce bit for bit (`assign_sequential` is the rule read literally, centroid by centroid;
`assign` the same arithmetic over all centroids at once).  `update` and `inertia` are float64 evaluations the kernels
are held to within the reordering bound of a float64 sum.  `quantize` / `dequantize` are the codec in float64 NumPy.
"""
import numpy as np

F32, F64 = np.float32, np.float64


# ---- the assignment ---------------------------------------------------------------------------------------------------
def distances(points, centroids) -> np.ndarray:
    """float32 [N,K]: d(i,k) = sum_j (x_ij - c_kj)^2, j = 0, 1, ... from 0.0f, each operation rounded on its own."""
    x, c = np.asarray(points, F32), np.asarray(centroids, F32)
    acc = np.zeros((x.shape[0], c.shape[0]), F32)
    with np.errstate(all="ignore"):
        for j in range(x.shape[1]):
            t = x[:, j:j + 1] - c[None, :, j]
            acc = acc + t * t
    assert acc.dtype == F32
    return acc


def assign(points, centroids):
    """-> (labels int32 [N], dist float32 [N]).  `d < best` from best = +inf in index order is the first index of the
    smallest distance with NaN counted as +inf; when that smallest is +inf nothing was ever below `best`: label 0."""
    d = distances(points, centroids)
    d = np.where(np.isnan(d), F32(np.inf), d)
    labels = np.argmin(d, axis=1).astype(np.int32)  # the first occurrence
    dist = d[np.arange(d.shape[0]), labels].astype(F32)
    labels[np.isinf(dist)] = 0
    return labels, dist


def assign_sequential(points, centroids):
    """The rule as written, one centroid after the other."""
    x, c = np.asarray(points, F32), np.asarray(centroids, F32)
    n = x.shape[0]
    best, label = np.full(n, np.inf, F32), np.zeros(n, np.int32)
    with np.errstate(all="ignore"):
        for k in range(c.shape[0]):
            acc = np.zeros(n, F32)
            for j in range(x.shape[1]):
                t = x[:, j] - c[k, j]
                acc = acc + t * t
            win = acc < best
            best, label = np.where(win, acc, best).astype(F32), np.where(win, k, label).astype(np.int32)
    return label, best


def tied_rows(points, centroids) -> np.ndarray:
    """bool [N]: rows whose smallest finite distance is attained by more than one centroid."""
    d = distances(points, centroids)
    d = np.where(np.isnan(d), F32(np.inf), d)
    m = d.min(axis=1, keepdims=True)
    return np.isfinite(m[:, 0]) & ((d == m).sum(axis=1) > 1)


def assign_case(n, k, d, seed, tile):
    """points [n,d], centroids [k,d].  Half the values sit on a coarse grid (quarters in [-1, 1]), so that equal
    distances occur among distinct centroids too.  Built in, where the sizes allow it:
      centroids: 1 == 0 (a duplicate); tile == tile - 1 (a duplicate across the tile boundary); 2 is all NaN
      points:    0 == centroid 0 (dist 0, a tie with centroid 1); 1 is all NaN; 2 is all +inf;
                 3 == centroid tile - 1 (dist 0, a tie across the boundary); 4 == the last centroid"""
    rng = np.random.default_rng(seed)
    grid = lambda shape: (rng.integers(-4, 5, shape) / 4.0).astype(F32)  # noqa: E731
    x = np.where(rng.random((n, 1)) < 0.5, grid((n, d)), rng.standard_normal((n, d))).astype(F32)
    c = np.where(rng.random((k, 1)) < 0.5, grid((k, d)), rng.standard_normal((k, d))).astype(F32)
    if k > 1:
        c[1] = c[0]
    if k > tile:
        c[tile] = c[tile - 1]
    if k > 3:
        c[2] = np.nan
    x[0] = c[0]
    if n > 4:
        x[1], x[2] = np.nan, np.inf
        x[3] = c[min(tile, k) - 1]
        x[4] = c[k - 1]
    return x, c


# ---- the update and the inertia -----------------------------------------------------------------------------------------
def update(points, labels, centroids, weights=None):
    """-> dict(mean float64 [K,D], new float32 [K,D], counts int32 [K], kept bool [K], scale float64 [K,D]): per
    cluster `np.add.reduce` of w x and of w in float64 over the members in index order, mean = S / W,
    new = float32(mean); a cluster without a member or with W == 0 keeps the old row (`kept`).
    scale = sum |w x| / W, the weighted mean magnitude the reordering bound is stated in."""
    x, old = np.asarray(points, F32).astype(F64), np.asarray(centroids, F32)
    k = old.shape[0]
    w_all = np.ones(x.shape[0], F64) if weights is None else np.asarray(weights, F32).astype(F64)
    mean, scale = np.zeros(old.shape, F64), np.zeros(old.shape, F64)
    new, counts, kept = old.copy(), np.zeros(k, np.int32), np.zeros(k, bool)
    for c in range(k):
        idx = np.flatnonzero(labels == c)
        counts[c] = idx.size
        w = w_all[idx]
        ws = np.add.reduce(w) if idx.size else 0.0
        if idx.size == 0 or ws == 0:
            kept[c] = True
            continue
        wx = w[:, None] * x[idx]
        mean[c] = np.add.reduce(wx, axis=0) / ws
        scale[c] = np.add.reduce(np.abs(wx), axis=0) / ws
        new[c] = mean[c].astype(F32)
    return {"mean": mean, "new": new, "counts": counts, "kept": kept, "scale": scale}


def inertia(points, centroids, labels, weights=None) -> float:
    x, c = np.asarray(points, F32).astype(F64), np.asarray(centroids, F32).astype(F64)
    d = ((x - c[labels]) ** 2).sum(axis=1)
    return float(d.sum() if weights is None else (np.asarray(weights, F32).astype(F64) * d).sum())


UPDATE_SIZES = (0, 1, 63, 64, 65, 1000, 0, 7, 300)  # members per cluster; 7 and 300 get zero weights in the weighted case


def update_case(d, seed, weighted):
    """points [N,d], labels int32 [N] (shuffled), old centroids [K,d], weights float32 [N] or None.  Clusters of
    UPDATE_SIZES members: two empty ones; with weights, the cluster of 7 has all weights zero and the cluster of 300
    some."""
    rng = np.random.default_rng(seed)
    labels = np.concatenate([np.full(s, c, np.int32) for c, s in enumerate(UPDATE_SIZES)])
    rng.shuffle(labels)
    n, k = labels.size, len(UPDATE_SIZES)
    x = (rng.standard_normal((n, d)) * rng.uniform(0.1, 3.0, (1, d)) + rng.uniform(-2, 2, (1, d))).astype(F32)
    old = rng.standard_normal((k, d)).astype(F32)
    w = None
    if weighted:
        w = rng.uniform(0.0, 2.0, n).astype(F32)
        w[labels == 7] = 0.0
        w[(labels == 8) & (rng.random(n) < 0.3)] = 0.0
    return x, labels, old, w


def loop_case(n=1000, d=45, centres=20, seed=3):
    """points [n,d] drawn around `centres` well-separated centres (spread 0.05 against a separation of order
    sqrt(2 d)), the last 50 rows duplicates of the first 50."""
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((centres, d)).astype(F32)
    x = (mu[rng.integers(0, centres, n)] + 0.05 * rng.standard_normal((n, d))).astype(F32)
    x[-50:] = x[:50]
    return x


# ---- the codec --------------------------------------------------------------------------------------------------------
def codec_scales(lo, hi, bits):
    """Python floats: inv = Q / (hi - lo) (0 when hi == lo), step = (hi - lo) / Q."""
    q = float(2 ** bits - 1)
    lo, hi = float(lo), float(hi)
    return (q / (hi - lo) if hi > lo else 0.0), (hi - lo) / q


def quantize(x, lo, hi, bits) -> np.ndarray:
    """x [N,C], per-column lo / hi -> integer codes as float64 [N,C]: floor((float64(x) - lo) * inv + 0.5)."""
    x = np.asarray(x).astype(F64)
    out = np.empty_like(x)
    for c in range(x.shape[1]):
        inv, _ = codec_scales(lo[c], hi[c], bits)
        out[:, c] = np.floor((x[:, c] - F64(lo[c])) * F64(inv) + F64(0.5))
    return out


def dequantize(codes, lo, hi, bits) -> np.ndarray:
    """-> float32 [N,C]: float32(lo + code * step)."""
    q = np.asarray(codes).astype(F64)
    out = np.empty(q.shape, F32)
    for c in range(q.shape[1]):
        _, step = codec_scales(lo[c], hi[c], bits)
        out[:, c] = (q[:, c] * F64(step) + F64(lo[c])).astype(F32)
    return out


def decode_bound(x, lo, hi, bits) -> np.ndarray:
    """(hi - lo) / (2 Q) (1 + 2^-20) + 2^-24 |x| per element of x [N,C]: half a step, the float64 arithmetic's slack,
    and the rounding of x' to float32."""
    x = np.asarray(x).astype(F64)
    q = float(2 ** bits - 1)
    half = (np.asarray(hi, F64) - np.asarray(lo, F64)) / (2.0 * q)
    return half[None, :] * (1.0 + 2.0 ** -20) + 2.0 ** -24 * np.abs(x)


def gaussian_params(n, degree, seed):
    """The six raw parameters of a model, float32 NumPy: a constant column (hi == lo) in features_dc included."""
    rng = np.random.default_rng(seed)
    bands = (degree + 1) ** 2 - 1
    p = {"means": rng.uniform(-3, 5, (n, 3)), "features_dc": rng.standard_normal((n, 3)),
         "features_rest": 0.2 * rng.standard_normal((n, bands, 3)), "opacities": rng.uniform(-6, 6, (n, 1)),
         "scales": rng.uniform(-7, -1, (n, 3)), "quats": rng.standard_normal((n, 4))}
    p["features_dc"][:, 1] = 0.25
    return {k: v.astype(F32) for k, v in p.items()}


def normalised_quats(quats) -> np.ndarray:
    q = np.asarray(quats).astype(F64)
    s = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]  # the order of the codec
    return q / np.sqrt(s)[:, None]
