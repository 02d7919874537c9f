"""NumPy restatements of the k-nearest-neighbour rule of include/gsraster.h and the inputs the
host and GPU tests share.

  brute64    float64 brute force: the truth the tolerances are held against
  brute32    float32, the kernel's operation order: dx = q - p, d2 = (dx*dx + dy*dy) + dz*dz, sqrt; the k smallest
             pairs (d2, row) in lexicographic order; what the exhaustive kernel must return bit for bit
  Tree/walk  the implicit tree of csrc/knn.hip and its stackless walk, every query a "lane" of one NumPy array: the
             same seed, the same box bound, the same strict comparison, the same escape arithmetic
"""
import functools

import numpy as np

f32 = np.float32
LEAF = 8
MAX_K = 16
INT_MAX = np.iinfo(np.int32).max
U = 2.0 ** -24
# max |d32 - d64| / (2^-24 d64) over every input below, measured and pinned by tests/test_knn_host.py
R_PINNED = 3.08


def round_up_k(k):
    return next(K for K in (1, 2, 3, 4, 8, 16) if K >= k)


def seed_wing(K):
    return K // LEAF + 1


# ---- inputs ------------------------------------------------------------------------------------------------------------
CLOUDS = ("uniform", "line", "plane", "identical", "lattice", "clusters", "outlier", "far", "duplicates")
KS = (1, 3, 8, 16)
SHAPE_N = (2, 63, 64, 65, 257, 4097)
QUERY_M = (1, 63, 65, 4097)
CLOUD_N = 257


@functools.lru_cache(maxsize=None)
def cloud(name, n):
    g = np.random.default_rng([CLOUDS.index(name), n])
    if name == "uniform":
        p = g.uniform(-1, 1, (n, 3))
    elif name == "line":
        p = g.uniform(-1, 1, (n, 1)) * np.array([[1.0, 2.0, 3.0]])
    elif name == "plane":
        p = np.concatenate([g.uniform(-1, 1, (n, 2)), np.full((n, 1), 0.25)], 1)
    elif name == "identical":
        p = np.tile([[0.3, -0.7, 1.1]], (n, 1))
    elif name == "lattice":  # massive exact ties: the index rule decides
        s = int(np.ceil(n ** (1 / 3)))
        p = np.stack(np.meshgrid(*[np.arange(s)] * 3, indexing="ij"), -1).reshape(-1, 3)[g.permutation(s ** 3)[:n]].astype(float)
    elif name == "clusters":  # 1e3 apart, 1e3 contrast in spacing
        a = g.uniform(0, 1, (n - n // 2, 3))
        b = g.uniform(0, 1e-3, (n // 2, 3)) + np.array([[1000.0, 0, 0]])
        p = np.concatenate([a, b])[g.permutation(n)]
    elif name == "outlier":
        p = g.uniform(-1, 1, (n, 3))
        p[n // 3] = (1e4, 1e4, 1e4)
    elif name == "far":
        p = g.uniform(-1, 1, (n, 3)) + np.array([[1000.0, -1000.0, 500.0]])
    elif name == "duplicates":
        base = g.uniform(-1, 1, ((n + 2) // 3, 3))
        p = base[g.integers(0, len(base), n)]
    else:
        raise KeyError(name)
    return np.ascontiguousarray(p, f32)


@functools.lru_cache(maxsize=None)
def queries(name, n, m):
    """m query points in (and a little around) the cloud's bounding box; the first is a reference point itself."""
    p = cloud(name, n)
    g = np.random.default_rng([77, CLOUDS.index(name), n, m])
    lo, hi = p.min(0).astype(float), p.max(0).astype(float)
    pad = 0.1 * np.maximum(hi - lo, 1e-3)
    q = g.uniform(lo - pad, hi + pad, (m, 3)).astype(f32)
    q[0] = p[len(p) // 2]
    return np.ascontiguousarray(q)


def shape_cases():
    return [(n, k) for k in KS for n in sorted({k + 1, *SHAPE_N}) if n > k]


def small_cases():
    """Every small input of the GPU tests: (cloud, n, m or None for self mode, k)."""
    out = [("uniform", n, None, k) for n, k in shape_cases()]
    out += [("uniform", CLOUD_N, m, k) for m in QUERY_M for k in KS]
    out += [(c, CLOUD_N, None, k) for c in CLOUDS if c != "uniform" for k in KS]
    out += [(c, CLOUD_N, 65, 3) for c in CLOUDS if c != "uniform"]
    return out


def case_inputs(case):
    name, n, m, k = case
    return cloud(name, n), (None if m is None else queries(name, n, m)), k


# ---- brute force -------------------------------------------------------------------------------------------------------
def _usable(P):
    return np.isfinite(P).all(1)


def _top(d, rows, k, self_rows):
    """The k smallest (d, row) pairs of every line of d [m, nu] (rows ascending along a line: a stable sort is the
    lexicographic order)."""
    if self_rows is not None:
        d = np.where(rows[None, :] == self_rows[:, None], np.inf, d)
    o = np.argsort(d, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(d, o, 1), rows[o].astype(np.int32)


def _pairs(P, Q, k, dtype):
    self_mode = Q is None
    Q = P if self_mode else Q
    keep = _usable(P)
    rows = np.nonzero(keep)[0]
    if len(rows) < k + self_mode:
        raise ValueError(f"{len(rows)} usable points, k = {k}")
    R, X = P[rows].astype(dtype), Q.astype(dtype)
    okq = _usable(Q)
    d2 = np.empty((len(Q), len(rows)), dtype)
    for s in range(0, len(Q), 1024):  # (in slabs: the 4097 x 4097 cases)
        x = np.where(okq[s:s + 1024, None], X[s:s + 1024], 0).astype(dtype)
        dx, dy, dz = (x[:, None, c] - R[None, :, c] for c in range(3))
        d2[s:s + 1024] = (dx * dx + dy * dy) + dz * dz
    d2, idx = _top(d2, rows, k, np.arange(len(Q)) if self_mode else None)
    d = np.sqrt(d2)
    d[~okq], idx[~okq] = np.nan, -1
    return d, idx


def brute64(P, Q=None, k=3):
    """-> (d float64 [m,k] ascending, idx int32 [m,k]); NaN / -1 for a non-finite query."""
    return _pairs(P, Q, k, np.float64)


def brute32(P, Q=None, k=3):
    """The rule in float32, operation for operation -> (d float32 [m,k], idx int32 [m,k])."""
    return _pairs(np.asarray(P, f32), None if Q is None else np.asarray(Q, f32), k, f32)


def own_distance64(P, Q, idx):
    """float64 distance from query i to P[idx[i, j]]."""
    Q = P if Q is None else Q
    return np.sqrt(((Q.astype(np.float64)[:, None, :] - P.astype(np.float64)[idx]) ** 2).sum(-1))


@functools.lru_cache(maxsize=None)
def _truth(name, n, m):
    P, Q, _ = case_inputs((name, n, m, 0))
    k = min(MAX_K, n - (m is None))
    return brute64(P, Q, k), brute32(P, Q, k)


def truth(case):
    """((d64, idx64), (d32, idx32)) of a small case, computed once per (cloud, n, m) at the largest k and cut."""
    name, n, m, k = case
    (a, b), (c, d) = _truth(name, n, m)
    return (a[:, :k], b[:, :k]), (c[:, :k], d[:, :k])


def tolerance(d64, r=R_PINNED):
    """|d - d64| <= 4 r 2^-24 d64, never below 4 2^-24 relative."""
    return 4.0 * max(r, 1.0) * U * np.abs(d64)


# ---- the tree and the walk ---------------------------------------------------------------------------------------------
def _spread10(v):
    v = v.astype(np.uint32)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000FF)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300F00F)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030C30C3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


class Tree:
    def __init__(self, P):
        P = np.asarray(P, f32)
        rows = np.nonzero(_usable(P))[0]
        self.skipped = len(P) - len(rows)
        R = P[rows]
        self.lo = R.min(0) if len(rows) else np.zeros(3, f32)
        ext = (R.max(0) - self.lo) if len(rows) else np.zeros(3, f32)
        with np.errstate(divide="ignore", over="ignore"):
            self.scale = np.where((ext > 0) & np.isfinite(ext), f32(1024) / ext, f32(0)).astype(f32)
        code = self.morton(R)
        order = np.argsort((code.astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64), kind="stable")
        self.pts, self.rows, self.code = R[order], rows[order].astype(np.int32), code[order]
        self.nu = nu = len(rows)
        self.L = -(-nu // LEAF)
        self.Lp = 1
        while self.Lp < self.L:
            self.Lp <<= 1
        Lp = self.Lp
        pad = np.full((Lp * LEAF - nu, 3), np.nan, f32)
        slots = np.concatenate([self.pts, pad]).reshape(Lp, LEAF, 3)
        self.box_lo = np.full((2 * Lp, 3), np.inf, f32)
        self.box_hi = np.full((2 * Lp, 3), -np.inf, f32)
        with np.errstate(all="ignore"):
            self.box_lo[Lp:] = np.where(np.isnan(slots), np.inf, slots).min(1)
            self.box_hi[Lp:] = np.where(np.isnan(slots), -np.inf, slots).max(1)
        c = Lp // 2
        while c >= 1:
            self.box_lo[c:2 * c] = np.minimum(self.box_lo[2 * c:4 * c:2], self.box_lo[2 * c + 1:4 * c:2])
            self.box_hi[c:2 * c] = np.maximum(self.box_hi[2 * c:4 * c:2], self.box_hi[2 * c + 1:4 * c:2])
            c >>= 1

    def morton(self, X):
        f = np.clip((X - self.lo) * self.scale, f32(0), f32(1023)).astype(f32)
        u = f.astype(np.uint32)
        return (_spread10(u[:, 0]) << np.uint32(2)) | (_spread10(u[:, 1]) << np.uint32(1)) | _spread10(u[:, 2])


def walk(tree, Q=None, k=3, self_mode=False, invert=False):
    """The query kernel, lane for lane -> (d float32 [m,k], idx int32 [m,k], leaf tests per query [m]).
    `invert`: enter a subtree iff its bound EXCEEDS the k-th d2 -- the comparison the wrong way round."""
    t = tree
    Q = np.asarray(Q, f32)
    m, K, nu, Lp = len(Q), round_up_k(k), t.nu, t.Lp
    assert nu >= k + self_mode
    bd = np.full((m, K), np.inf, f32)
    bi = np.full((m, K), INT_MAX, np.int32)
    tests = np.zeros(m, np.int64)
    live = _usable(Q)
    skip = np.arange(m) if self_mode else np.full(m, -1)

    def leaf_test(lanes, leaf):
        at = leaf[:, None] * LEAF + np.arange(LEAF)[None, :]
        ok = at < nu
        at = np.minimum(at, nu - 1)
        p, q = t.pts[at], Q[lanes]
        dx, dy, dz = (q[:, None, c] - p[:, :, c] for c in range(3))
        d2 = ((dx * dx + dy * dy) + dz * dz).astype(f32)
        row = t.rows[at]
        out = ~ok | (row == skip[lanes][:, None])
        d2, row = np.where(out, f32(np.inf), d2), np.where(out, INT_MAX, row)
        cd, cr = np.concatenate([bd[lanes], d2], 1), np.concatenate([bi[lanes], row], 1)
        o = np.argsort(cr, axis=1, kind="stable")
        cd, cr = np.take_along_axis(cd, o, 1), np.take_along_axis(cr, o, 1)
        o = np.argsort(cd, axis=1, kind="stable")[:, :K]
        bd[lanes], bi[lanes] = np.take_along_axis(cd, o, 1), np.take_along_axis(cr, o, 1)
        tests[lanes] += ok.any(1)

    c = t.morton(np.where(live[:, None], Q, 0).astype(f32)).astype(np.int64)
    code = t.code.astype(np.int64)
    lo = np.searchsorted(code, c, "left")
    at = np.minimum(lo, nu - 1)
    inner = (lo > 0) & (lo < nu)
    nearer = inner & (c - code[np.maximum(lo - 1, 0)] < code[np.minimum(lo, nu - 1)] - c)
    at = np.where(nearer, lo - 1, at)
    s0 = np.maximum(at // LEAF - seed_wing(K), 0)
    s1 = np.minimum(at // LEAF + seed_wing(K), t.L - 1)
    for off in range(2 * seed_wing(K) + 1):
        lanes = np.nonzero(live & (s0 + off <= s1))[0]
        if len(lanes):
            leaf_test(lanes, (s0 + off)[lanes])
    node = np.where(live, 1, 0).astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        while True:
            a = np.nonzero(node)[0]
            if not len(a):
                break
            nd, q = node[a], Q[a]
            g = np.maximum(np.maximum(t.box_lo[nd] - q, q - t.box_hi[nd]), f32(0)).astype(f32)
            b = ((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]).astype(f32)
            kth = bd[a, K - 1]
            enter = (b > kth) if invert else ~(b > kth)
            down = enter & (nd < Lp)
            leaf = enter & (nd >= Lp)
            l = nd - Lp
            hit = leaf & ((l < s0[a]) | (l > s1[a]))
            if hit.any():
                leaf_test(a[hit], l[hit])
            up = nd.copy()
            while True:  # escape: strip the trailing ones, then the right sibling (or 0: done)
                odd = ~down & ((up & 1) == 1)
                if not odd.any():
                    break
                up[odd] >>= 1
            node[a] = np.where(down, 2 * nd, np.where(up > 0, up + 1, 0))
    d = np.sqrt(bd[:, :k])
    idx = bi[:, :k].copy()
    d[~live], idx[~live] = np.nan, -1
    return d, idx, tests
