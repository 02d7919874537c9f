"""NumPy statement of the surface-distance rule of include/gsraster.h, and the inputs the tests
of tests/test_surface_distance_host.py and tests/test_gpu_surface_distance.py share.

`distance(points, vertices, triangles, dtype)` is a brute force over every (point, triangle) pair.  With
dtype = float64 it is the truth the GPU is held to; with dtype = float32 it performs the operations of
`tri_closest` / `leaf_test` (csrc/mesh_distance.hip) in the same order, every one rounded on its own.
`distance_by_projection` is an independent formulation (projection onto the plane if it falls inside, else the nearest
of the three edges) the first is checked against.  `Tree` restates the tree build and the stackless walk of the kernels
in plain Python, so that their logic can be rehearsed without a device.
"""
import functools

import numpy as np

FLAT = 2.0 ** -40   # |n|^2 <= FLAT |ab|^2 |ac|^2: the triangle counts as its three edges
SLACK = 2.0 ** -18  # the walk's prune slack, in units of the node's reach R
U = 2.0 ** -24

# The worst |d32 - d64| / (2^-24 S) of the float32 restatement over every input of `cases()`, S the largest
# |coordinate| of mesh and points: measured by tests/test_surface_distance_host.py (which prints it per case), pinned
# here.  The GPU tests allow tol = 4 R_PINNED 2^-24 S.
R_PINNED = 3.36


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _along(a, t, e):
    return a + t[..., None] * e


def _quot(num, den):
    """num / den where den > 0, else 0 (the guarded quotients of the rule)"""
    ok = den > 0
    return np.where(ok, num / np.where(ok, den, 1), 0).astype(num.dtype)


def _seg(a, e):
    t = _quot(-_dot(a, e), _dot(e, e))
    t = np.fmin(np.fmax(t, t.dtype.type(0)), t.dtype.type(1))
    return _along(a, t, e)


def closest_translated(a, b, c):
    """Closest point of the triangles (a, b, c) [..., 3] to the origin, in the arrays' dtype."""
    T = a.dtype.type
    ab, ac, bc = b - a, c - a, c - b
    n = np.stack([ab[..., 1] * ac[..., 2] - ab[..., 2] * ac[..., 1], ab[..., 2] * ac[..., 0] - ab[..., 0] * ac[..., 2],
                  ab[..., 0] * ac[..., 1] - ab[..., 1] * ac[..., 0]], -1)
    d1, d2 = -_dot(ab, a), -_dot(ac, a)
    d3, d4 = -_dot(ab, b), -_dot(ac, b)
    d5, d6 = -_dot(ab, c), -_dot(ac, c)
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
    flat = ~(_dot(n, n) > T(FLAT) * (_dot(ab, ab) * _dot(ac, ac)))
    # the three edges as segments: the fallback, overwritten below in reverse order of priority
    q0, q1, q2 = _seg(a, ab), _seg(b, bc), _seg(a, ac)
    s0, s1, s2 = _dot(q0, q0), _dot(q1, q1), _dot(q2, q2)
    q, s = q0, s0
    take = s1 < s
    q, s = np.where(take[..., None], q1, q), np.where(take, s1, s)
    q = np.where((s2 < s)[..., None], q2, q)
    fallback = q
    zero = T(0)
    inside = (va > zero) & (vb > zero) & (vc > zero)
    tot = (va + vb) + vc
    ok = np.where(inside, tot, T(1))
    q = np.where(inside[..., None], _along(_along(a, (vb / ok).astype(a.dtype), ab), (vc / ok).astype(a.dtype), ac), q)
    e0, e1 = d4 - d3, d5 - d6
    m = (va <= zero) & (e0 >= zero) & (e1 >= zero)
    q = np.where(m[..., None], _along(b, _quot(e0, e0 + e1), bc), q)
    m = (vb <= zero) & (d2 >= zero) & (d6 <= zero)
    q = np.where(m[..., None], _along(a, _quot(d2, d2 - d6), ac), q)
    m = (vc <= zero) & (d1 >= zero) & (d3 <= zero)
    q = np.where(m[..., None], _along(a, _quot(d1, d1 - d3), ab), q)
    q = np.where(((d6 >= zero) & (d5 <= d6))[..., None], c, q)
    q = np.where(((d3 >= zero) & (d4 <= d3))[..., None], b, q)
    q = np.where(((d1 <= zero) & (d2 <= zero))[..., None], a, q)
    return np.where(flat[..., None], fallback, q).astype(a.dtype)


def usable(vertices, triangles):
    """Mask [F] of the triangles that enter the tree: finite vertices and a finite float32 centroid."""
    t = np.asarray(vertices, np.float32)[np.asarray(triangles)]
    with np.errstate(all="ignore"):
        g = ((t[:, 0] + t[:, 1]) + t[:, 2]) * np.float32(1.0 / 3.0)
    return np.isfinite(t).all((1, 2)) & np.isfinite(g).all(1)


def pair_distances(points, tri, dtype):
    """-> [K] distances in `dtype` from float32 points [K,3] to float32 triangles [K,3,3], pair by pair."""
    p, tri = np.asarray(points, np.float32).astype(dtype), np.asarray(tri, np.float32).astype(dtype)
    out = np.empty(len(p), dtype)
    with np.errstate(all="ignore"):
        for i in range(0, len(p), 4096):  # (temporaries of a chunk stay in cache)
            o = p[i:i + 4096]
            q = closest_translated(tri[i:i + 4096, 0] - o, tri[i:i + 4096, 1] - o, tri[i:i + 4096, 2] - o)
            out[i:i + 4096] = np.sqrt(_dot(q, q))
    return out


def _candidates(points, tri):
    """Pairs (point, triangle) that can hold a point's minimum, as two index arrays ordered by point: a triangle
    whose bounding sphere lies farther from the point than the far side of the nearest sphere, by more than a margin
    a thousand times any float32 rounding, cannot -- in float64 or in float32.  Every other pair is evaluated."""
    p, t = np.asarray(points, np.float64), np.asarray(tri, np.float64)
    centre = t.mean(1)
    radius = np.sqrt(((t - centre[:, None]) ** 2).sum(-1)).max(1)
    margin = 1e-4 * max(np.abs(p).max(initial=0.0), np.abs(t).max(initial=0.0)) + 1e-30
    rows, cols = [], []
    for i in range(0, len(p), 512):
        D = np.sqrt(((p[i:i + 512, None, :] - centre[None]) ** 2).sum(-1))
        far = (D + radius).min(1)
        r, c = np.nonzero(D - radius <= far[:, None] + margin)
        rows.append(r + i)
        cols.append(c)
    return np.concatenate(rows), np.concatenate(cols)


def distance(points, vertices, triangles, dtype=np.float64):
    """-> (d [n] in `dtype`, face int32 [n], the lowest minimiser): NaN / -1 for a non-finite point; triangles that
    are not `usable` are left out."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    triangles = np.asarray(triangles)
    keep = np.nonzero(usable(vertices, triangles))[0]
    if not len(keep):
        raise ValueError("no usable triangle")
    tri = np.asarray(vertices, np.float32)[triangles[keep]]
    good = np.nonzero(np.isfinite(points).all(1))[0]
    d = np.full(len(points), np.nan, dtype)
    f = np.full(len(points), -1, np.int32)
    if len(good):
        rows, cols = _candidates(points[good], tri)
        x = pair_distances(points[good][rows], tri[cols], dtype)
        first = np.nonzero(np.r_[True, rows[1:] != rows[:-1]])[0]
        low = np.minimum.reduceat(x, first)
        hit = np.nonzero(x == low[rows])[0]
        _, at = np.unique(rows[hit], return_index=True)
        d[good] = low
        f[good] = keep[cols[hit[at]]]
    return d, f


def face_distance(points, vertices, triangles, faces, dtype=np.float64):
    """-> [n] distance of point i to triangle faces[i] alone."""
    tri = np.asarray(vertices, np.float32)[np.asarray(triangles)[np.asarray(faces)]]
    return pair_distances(points, tri, dtype)


def distance_by_projection(points, vertices, triangles):
    """float64, written apart from `closest_translated`: the projection onto the plane when it falls inside the
    triangle, else the nearest point of the three edges; flat triangles (the rule's threshold) are edges only."""
    p = np.asarray(points, np.float64)[:, None, :]
    t = np.asarray(vertices, np.float64)[np.asarray(triangles)][None]
    a, b, c = t[:, :, 0], t[:, :, 1], t[:, :, 2]
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    flat = ~(nn > FLAT * ((b - a) ** 2).sum(-1) * ((c - a) ** 2).sum(-1))
    with np.errstate(all="ignore"):
        h = ((p - a) * n).sum(-1) / nn
        foot = p - h[..., None] * n
        inside = np.ones(h.shape, bool)
        for u, v in ((a, b), (b, c), (c, a)):
            inside &= (np.cross(v - u, foot - u) * n).sum(-1) >= 0
        best = np.where(inside & ~flat, np.abs(h) * np.sqrt(nn), np.inf)
        for u, v in ((a, b), (b, c), (c, a)):
            e = v - u
            ee = (e * e).sum(-1)
            s = np.clip(np.where(ee > 0, ((p - u) * e).sum(-1) / np.where(ee > 0, ee, 1), 0), 0, 1)
            best = np.minimum(best, np.sqrt(((u + s[..., None] * e - p) ** 2).sum(-1)))
    return best.min(1)


def scale_of(points, vertices, triangles):
    """S: the largest finite |coordinate| of the usable mesh and the points."""
    v = np.asarray(vertices, np.float32)[np.asarray(triangles)[usable(vertices, triangles)]]
    p = np.asarray(points, np.float32)
    both = np.concatenate([v.reshape(-1), p[np.isfinite(p)].reshape(-1), [0.0]])
    return float(np.abs(both).max())


def tolerance(points, vertices, triangles):
    return 4.0 * R_PINNED * U * scale_of(points, vertices, triangles)


# ---- the tree, restated --------------------------------------------------------------------------------------------
NODE_END = -2 ** 31


def _spread10(v):
    v = (v | (v << 16)) & 0x030000FF
    v = (v | (v << 8)) & 0x0300F00F
    v = (v | (v << 4)) & 0x030C30C3
    v = (v | (v << 2)) & 0x09249249
    return v


class Tree:
    """The build and the walk of csrc/mesh_distance.hip on the host (plain Python: small meshes only)."""

    def __init__(self, vertices, triangles, tie_break=True):
        f32 = np.float32
        vertices, triangles = np.asarray(vertices, f32), np.asarray(triangles)
        keep = usable(vertices, triangles)
        t = vertices[triangles[keep]]
        self.lo = t.reshape(-1, 3).min(0)
        ext = t.reshape(-1, 3).max(0) - self.lo
        with np.errstate(all="ignore"):
            self.scale = np.where((ext > 0) & np.isfinite(ext), f32(1024) / ext, f32(0)).astype(f32)
        cent = ((t[:, 0] + t[:, 1]) + t[:, 2]) * f32(1.0 / 3.0)
        faces = np.nonzero(keep)[0]
        keys = [(int(self.code(g)) << 32) | (int(f) if tie_break else 0) for g, f in zip(cent, faces)]
        order = sorted(range(len(keys)), key=lambda k: (keys[k], faces[k]))
        self.key = [keys[k] for k in order]
        self.face = faces[order]
        self.tri = t[order]
        self.code_of_leaf = [k >> 32 for k in self.key]
        n = self.n = len(order)
        self.left, self.right, self.last = [0] * n, [0] * n, [0] * n
        self.after, self.parent_node, self.parent_leaf = [NODE_END] * n, [-1] * n, [-1] * n
        for i in range(n - 1):
            self._karras(i)
        self.escape_node = [NODE_END if self.last[i] == n - 1 else self.after[self.last[i]] for i in range(n - 1)]
        self.escape_leaf = [NODE_END if l == n - 1 else self.after[l] for l in range(n)]
        self.root = ~0 if n == 1 else 0
        self._refit()

    def code(self, p):
        f32 = np.float32
        with np.errstate(all="ignore"):
            g = np.fmin(np.fmax((np.asarray(p, f32) - self.lo) * self.scale, f32(0)), f32(1023)).astype(np.int64)
        return (_spread10(int(g[0])) << 2) | (_spread10(int(g[1])) << 1) | _spread10(int(g[2]))

    def _delta(self, i, j):
        if j < 0 or j >= self.n:
            return -1
        x = self.key[i] ^ self.key[j]
        return 64 - x.bit_length()  # (64 for equal keys: what the tie-break removes)

    def _karras(self, i):
        d = 1 if self._delta(i, i + 1) > self._delta(i, i - 1) else -1
        dmin = self._delta(i, i - d)
        lmax = 2
        while self._delta(i, i + lmax * d) > dmin:
            lmax <<= 1
        length, t = 0, lmax >> 1
        while t >= 1:
            if self._delta(i, i + (length + t) * d) > dmin:
                length += t
            t >>= 1
        j = i + length * d
        dnode = self._delta(i, j)
        s, t = 0, (length + 1) >> 1
        while True:
            if self._delta(i, i + (s + t) * d) > dnode:
                s += t
            if t <= 1:
                break
            t = (t + 1) >> 1
        split = i + s * d + min(d, 0)
        first, lst = min(i, j), max(i, j)
        L = ~split if first == split else split
        R = ~(split + 1) if lst == split + 1 else split + 1
        self.left[i], self.right[i], self.last[i] = L, R, lst
        if 0 <= split < self.n:
            self.after[split] = R
        for c in (L, R):
            if c < 0:
                if 0 <= ~c < self.n:
                    self.parent_leaf[~c] = i
            elif c < self.n:
                self.parent_node[c] = i

    def _refit(self):
        n = self.n
        self.box_lo, self.box_hi = np.zeros((max(n - 1, 1), 3), np.float32), np.zeros((max(n - 1, 1), 3), np.float32)
        count = [0] * n
        self.refit_complete = n < 2
        for l in range(n):
            lo, hi = self.tri[l].min(0), self.tri[l].max(0)
            child, p = ~l, self.parent_leaf[l]
            while p >= 0:
                count[p] += 1
                if count[p] == 1:
                    break
                sib = self.right[p] if child == self.left[p] else self.left[p]
                if sib < 0:
                    olo, ohi = self.tri[~sib].min(0), self.tri[~sib].max(0)
                else:
                    olo, ohi = self.box_lo[sib], self.box_hi[sib]
                lo, hi = np.minimum(lo, olo), np.maximum(hi, ohi)
                self.box_lo[p], self.box_hi[p] = lo, hi
                child, p = p, self.parent_node[p]
                if p < 0:
                    self.refit_complete = True

    def leaves_reached(self):
        """Leaves in the order an unpruned walk meets them (each exactly once, ascending, in a sound tree)."""
        out, node, steps = [], self.root, 0
        while node != NODE_END and steps < 4 * self.n + 4:
            steps += 1
            if node >= 0:
                node = self.left[node]
            else:
                out.append(~node)
                node = self.escape_leaf[~node]
        return out

    def query(self, points, slack=SLACK):
        """-> (d float32 [n], face [n], leaf tests per point): the walk of `md_query_kernel`."""
        f32 = np.float32
        points = np.asarray(points, f32)
        d, face, tests = np.full(len(points), np.nan, f32), np.full(len(points), -1, np.int32), []
        for r, p in enumerate(points):
            if not np.isfinite(p).all():
                tests.append(0)
                continue
            code = self.code(p)
            lo = int(np.searchsorted(np.asarray(self.code_of_leaf, np.int64), code, "left"))
            seed = min(lo, self.n - 1)
            if 0 < lo < self.n and code - self.code_of_leaf[lo - 1] < self.code_of_leaf[lo] - code:
                seed = lo - 1
            best, bf, count = f32(np.inf), -1, 0

            def leaf(l, best, bf):
                t = self.tri[l] - p
                with np.errstate(all="ignore"):
                    q = closest_translated(t[0][None], t[1][None], t[2][None])
                    x = np.sqrt(_dot(q, q))[0]
                return (x, int(self.face[l])) if x < best else (best, bf)

            best, bf = leaf(seed, best, bf)
            node = self.root
            while node != NODE_END:
                if node >= 0:
                    a, b = self.box_lo[node] - p, p - self.box_hi[node]
                    dd = np.fmax(np.fmax(a, b), f32(0))
                    db2 = (dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]
                    reach = best + f32(slack) * max(np.abs(a).max(), np.abs(b).max())
                    node = self.escape_node[node] if db2 > reach * reach else self.left[node]
                else:
                    best, bf = leaf(~node, best, bf)
                    count += 1
                    node = self.escape_leaf[~node]
            d[r], face[r] = best, bf
            tests.append(count)
        return d, face, tests


# ---- inputs ------------------------------------------------------------------------------------------------------------
SHAPE_F = (1, 2, 63, 64, 65, 257, 4096)
SHAPE_N = (1, 63, 64, 65, 4097)


def soup(F, seed, lo=1e-3, hi=1.0, box=1.0):
    """F triangles with edge lengths log-uniform in [lo, hi], first vertices uniform in [-box, box]^3 -> (v, t)."""
    g = np.random.default_rng(seed)
    a = g.uniform(-box, box, (F, 3))
    e = []
    for _ in range(2):
        u = g.normal(size=(F, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        e.append(u * np.exp(g.uniform(np.log(lo), np.log(hi), (F, 1))))
    v = np.stack([a, a + e[0], a + e[1]], 1).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def cloud(n, seed, box=1.2, centre=(0.0, 0.0, 0.0)):
    g = np.random.default_rng(seed)
    return (np.asarray(centre) + g.uniform(-box, box, (n, 3))).astype(np.float32)


def near_surface(n, v, t, seed, sigma=0.02):
    """Points scattered about random triangles of the mesh (what a generated mesh's vertices look like)."""
    g = np.random.default_rng(seed)
    tri = np.asarray(v, np.float64)[np.asarray(t)][g.integers(0, len(t), n)]
    w = g.dirichlet((1, 1, 1), n)
    return ((tri * w[:, :, None]).sum(1) + g.normal(scale=sigma, size=(n, 3))).astype(np.float32)


def sphere(subdivisions=2, radius=1.0, bump=0.0, seed=0):
    """Closed subdivided-tetrahedron approximation of a sphere, welded -> (v float32, t int32)."""
    v = [np.array(x, np.float64) / np.sqrt(3) for x in ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1))]
    t = [(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)]
    for _ in range(subdivisions):
        mid, nt = {}, []

        def m(i, j):
            k = (min(i, j), max(i, j))
            if k not in mid:
                x = v[i] + v[j]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in t:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = nt
    v = np.array(v)
    if bump:
        v = v * (1 + bump * np.random.default_rng(seed).uniform(-1, 1, (len(v), 1)))
    return (radius * v).astype(np.float32), np.array(t, np.int32)


SEVEN_TRI = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32))
# point -> exact distance: the face, the three vertex regions, the three edge regions; on a vertex, an edge, the face
SEVEN_POINTS = (((0.25, 0.25, 0.5), 0.5), ((-3, -4, 0), 5.0), ((2, 0, 0), 1.0), ((0.5, -2, 0), 2.0),
                ((0, 4, 3), np.sqrt(18.0)), ((4, 4, 0), np.sqrt(24.5)), ((-2, 0.5, 0), 2.0), ((4, -3, 0), np.sqrt(18.0)),
                ((0, 0, 0), 0.0), ((1, 0, 0), 0.0), ((0.5, 0, 0), 0.0), ((0.5, 0.5, 0), 0.0), ((0.25, 0.5, 0), 0.0),
                ((0.25, 0.25, -2), 2.0))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (vertices float32 [V,3], triangles int32 [F,3], points float32 [n,3]) of a named test input."""
    if name.startswith("shape"):  # "shape F": the mesh of that F with the 4097 shared points (tests take prefixes)
        F = int(name.split()[1])
        v, t = soup(F, 100 + F)
        half = SHAPE_N[-1] // 2
        return v, t, np.concatenate([cloud(half, 7), near_surface(SHAPE_N[-1] - half, v, t, 8)])
    if name == "seven regions":
        return SEVEN_TRI + (np.array([p for p, _ in SEVEN_POINTS], np.float32),)
    if name == "two triangles":  # a roof: points in the symmetry plane are equidistant from both
        v = np.array([[0, 0, 1], [0, 1, 1], [1, 0.5, 0], [-1, 0.5, 0]], np.float32)
        t = np.array([[0, 1, 2], [1, 0, 3]], np.int32)
        p = np.array([[0, y, z] for y in (0.25, 0.5, 2.0) for z in (-1.0, 0.5, 3.0)], np.float32)
        return v, t, p
    if name == "identical":
        v, t = soup(1, 5)
        return v, np.tile(t, (300, 1)), cloud(200, 6)
    if name == "line":  # centroids on one line
        v, t = soup(300, 9, 1e-2, 1e-1, 0.0)
        v = v + np.repeat(np.linspace(-1, 1, 300), 3)[:, None].astype(np.float32) * np.float32([1, 0, 0])
        g0 = v.reshape(-1, 3, 3).mean(1, keepdims=True)
        v = (v.reshape(-1, 3, 3) - g0 * np.float32([0, 1, 1])).reshape(-1, 3).astype(np.float32)
        return v, t, cloud(300, 10)
    if name == "plane":  # centroids in one plane
        v, t = soup(500, 11, 1e-2, 1e-1)
        g0 = v.reshape(-1, 3, 3).mean(1, keepdims=True)
        v = (v.reshape(-1, 3, 3) - g0 * np.float32([0, 0, 1])).reshape(-1, 3).astype(np.float32)
        return v, t, cloud(300, 12)
    if name == "one large":  # one triangle across the scene among 4 095 tiny ones
        v, t = soup(4096, 13, 1e-3, 1e-2)
        v[3 * 2000:3 * 2000 + 3] = np.float32([[-1.2, -1.1, -0.9], [1.3, -0.8, 0.2], [0.1, 1.2, 1.1]])
        return v, t, np.concatenate([cloud(300, 14), near_surface(300, v, t, 15)])
    if name == "degenerate":  # collinear and single-point triangles (dyadic) among normal ones
        v, t = soup(60, 16)
        extra = np.float32([[0, 0, 2], [1, 0, 2], [3, 0, 2],          # collinear, c beyond b
                            [0, 2, 2], [4, 2, 2], [1, 2, 2],          # collinear, c between
                            [2, 2, 2], [2, 2, 2], [2, 2, 2],          # a point
                            [-2, 0, 2], [-2, 0, 2], [-2, 1, 2]])      # a == b
        v = np.concatenate([v, extra])
        t = np.concatenate([t, np.arange(180, 192, dtype=np.int32).reshape(4, 3)])
        p = np.concatenate([cloud(100, 17, 3.0), np.float32([[2, 0, 2.5], [5, 0, 2], [2, 2, 3], [2, 2.5, 2],
                                                              [-2, 0.5, 2.25], [-2, 3, 2], [0.5, 1, 2]])])
        return v, t, p
    if name == "poisoned":  # NaN / Inf vertices in some triangles, NaN / Inf rows among the points
        v, t = soup(200, 18)
        v = v.copy()
        v[3 * 5, 1], v[3 * 77 + 2, 0], v[3 * 199 + 1, 2] = np.nan, np.inf, -np.inf
        p = cloud(300, 19)
        p[0, 0], p[64, 2], p[150, 1], p[299] = np.nan, np.inf, -np.inf, np.nan
        return v, t, p
    if name == "far":  # the precision case: triangles of size 0.01, everything moved by (1000, -1000, 500)
        v, t = soup(257, 20, 0.01, 0.01)
        off = np.float32([1000, -1000, 500])
        return (v + off).astype(np.float32), t, (np.concatenate([cloud(300, 21), near_surface(300, v, t, 22)]) + off).astype(np.float32)
    raise KeyError(name)


CASES = tuple(f"shape {F}" for F in SHAPE_F) + ("seven regions", "two triangles", "identical", "line", "plane",
                                                  "one large", "degenerate", "poisoned", "far")
POISONED_TRIANGLES, POISONED_POINTS = (5, 77, 199), (0, 64, 150, 299)


@functools.lru_cache(maxsize=None)
def truth(name):
    """-> (d64 [n], face [n]) of a named case: computed once per process, read-only."""
    v, t, p = case(name)
    out = distance(p, v, t, np.float64)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restated(name):
    """-> (d32 [n], face [n]) of a named case by the float32 restatement."""
    v, t, p = case(name)
    out = distance(p, v, t, np.float32)
    for a in out:
        a.setflags(write=False)
    return out


def medium(seed=30):
    """50 000-odd triangles: a bumpy sphere and 100 large floor triangles; 100 000 points -> (v, t, p)."""
    v, t = sphere(7, 1.0, 0.01, seed)  # 4 * 4^7 = 65 536 triangles
    t = t[:49900]
    g = np.random.default_rng(seed)
    fa = np.concatenate([g.uniform(-3, 3, (100, 2)), np.full((100, 1), -1.2)], 1)
    fl = np.stack([fa, fa + [2.0, 0.1, 0], fa + [0.2, 2.0, 0]], 1).reshape(-1, 3).astype(np.float32)
    t = np.concatenate([t, (np.arange(300, dtype=np.int32) + len(v)).reshape(100, 3)])
    v = np.concatenate([v, fl]).astype(np.float32)
    p = np.concatenate([cloud(50000, seed + 1, 1.5), near_surface(50000, v, t, seed + 2, 0.01)])
    return v, t.astype(np.int32), p


# ---- files -------------------------------------------------------------------------------------------------------------
def write_binary_stl(path, tri):
    tri = np.asarray(tri, np.float32)
    rec = np.zeros(len(tri), np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]))
    rec["v"] = tri
    with open(path, "wb") as f:
        f.write(b"solid binary, despite this word".ljust(80, b" "))
        f.write(np.uint32(len(tri)).tobytes())
        f.write(rec.tobytes())


def write_ascii_stl(path, tri):
    with open(path, "w") as f:
        f.write("solid fixture\n")
        for t in np.asarray(tri, np.float32):
            f.write(" facet normal 0 0 0\n  outer loop\n")
            for x in t:
                f.write("   vertex %s %s %s\n" % tuple(repr(float(c)) for c in x))
            f.write("  endloop\n endfacet\n")
        f.write("endsolid fixture\n")
