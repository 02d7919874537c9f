"""NumPy oracle of the mesh-cleaning rules of include/gsraster.h, written apart from
csrc/mesh_clean.hip: `np.unique` on sorted triples and sorted pairs, then min-label propagation with pointer jumping to
a fixed point -- no sort-and-scan, no union-find.  Also the seeded meshes the host and GPU tests share.
"""
import functools

import numpy as np

DEFAULT_MIN = 20000


def null_faces(tri, vertices=None):
    """Rule 2: a repeated index, or a cross product whose three float32 components are all exactly 0."""
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    null = (a == b) | (b == c) | (a == c)
    if vertices is not None and len(tri):
        v = np.asarray(vertices, np.float32)
        with np.errstate(all="ignore"):
            u, w = v[b] - v[a], v[c] - v[a]  # float32 arrays: every operation is rounded on its own
            nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
            ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
            nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
            null |= (nx == 0) & (ny == 0) & (nz == 0)
    return null


def duplicate_faces(tri, alive):
    """Rule 3 over the faces `alive`: True for every face whose index set occurred at a lower (alive) face index."""
    idx = np.nonzero(alive)[0]
    s = np.sort(tri[idx].astype(np.int64), axis=1)
    _, first = np.unique(s, axis=0, return_index=True)  # indices of the FIRST occurrences
    dup = np.zeros(len(tri), bool)
    dup[idx] = True
    dup[idx[first]] = False
    return dup


def component_labels(tri, alive):
    """Rule 4: label = the lowest face index of the edge-connected component, -1 where not `alive`."""
    F = len(tri)
    labels = np.full(F, -1, np.int64)
    idx = np.nonzero(alive)[0]
    n = len(idx)
    if n == 0:
        return labels
    t = tri[idx].astype(np.int64)
    pairs = np.stack([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], 1).reshape(-1, 2)  # half-edge 3 i + k of face i
    pairs.sort(axis=1)
    _, edge = np.unique(pairs, axis=0, return_inverse=True)
    edge = edge.reshape(-1)
    order = np.argsort(edge, kind="stable")
    starts = np.nonzero(np.diff(edge[order], prepend=-1))[0]
    face_sorted = order // 3
    lab = np.arange(n)
    while True:
        edge_min = np.minimum.reduceat(lab[face_sorted], starts)   # lowest label on every edge
        m = np.minimum(edge_min[edge].reshape(n, 3).min(1), lab)  # lowest label among a face and its neighbours
        new = lab.copy()
        np.minimum.at(new, lab, m)  # hang the face's representative under it
        new = np.minimum(new, m)
        while True:  # pointer jumping
            j = new[new]
            if np.array_equal(j, new):
                break
            new = j
        if np.array_equal(new, lab):
            break
        lab = new
    labels[idx] = idx[lab]  # (idx ascends: the lowest compact index is the lowest face index)
    return labels


def clean_reference(vertices, triangles, colors=None, min_faces=DEFAULT_MIN, num_vertices=None):
    """-> dict(labels, sizes, vertices, colors, triangles, info); `vertices` None: labels and sizes only (only the
    repeated-index part of the null rule), with `num_vertices` given."""
    tri = np.asarray(triangles, np.int32).reshape(-1, 3)
    V = len(vertices) if vertices is not None else int(num_vertices)
    F = len(tri)
    if F and (tri.min() < 0 or tri.max() >= V):
        raise ValueError("triangle index outside [0, V)")
    null = null_faces(tri, vertices)
    dup = duplicate_faces(tri, ~null)
    alive = ~null & ~dup
    labels = component_labels(tri, alive)
    sizes = np.zeros(F, np.int64)
    if alive.any():
        sizes[alive] = np.bincount(labels[alive], minlength=F)[labels[alive]]
    keep = alive & (sizes >= min_faces)
    roots = alive & (labels == np.arange(F))
    out = {"labels": labels.astype(np.int32), "sizes": sizes.astype(np.int32)}
    used = np.zeros(V, bool)
    used[tri[keep].reshape(-1)] = True
    remap = np.cumsum(used) - 1
    out["triangles"] = remap[tri[keep]].astype(np.int32).reshape(-1, 3)
    out["vertices"] = None if vertices is None else np.asarray(vertices, np.float32)[used]
    out["colors"] = None if colors is None else np.asarray(colors, np.float32)[used]
    out["info"] = {"null_faces": int(null.sum()), "duplicate_faces": int(dup.sum()), "components": int(roots.sum()),
                   "components_kept": int((roots & keep).sum()),
                   "faces_removed_small": int(alive.sum() - keep.sum()), "vertices_removed": int(V - used.sum())}
    return out


def union_find_labels(tri, alive):
    """The same labels by a plain Python union-find over a dict of edges (small meshes only)."""
    parent = list(range(len(tri)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    seen = {}
    for f in np.nonzero(alive)[0].tolist():
        a, b, c = (int(x) for x in tri[f])
        for e in ((min(a, b), max(a, b)), (min(b, c), max(b, c)), (min(c, a), max(c, a))):
            g = seen.setdefault(e, f)
            ra, rb = find(f), find(g)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(f) if alive[f] else -1 for f in range(len(tri))], np.int32)


# ---- meshes ----------------------------------------------------------------------------------------------------------
def permuted(vertices, tri, seed, colors=None):
    """Random vertex numbering, face order and starting corner (the winding is kept)."""
    rng = np.random.default_rng(seed)
    V, F = len(vertices), len(tri)
    new_id = rng.permutation(V)  # old -> new
    v = np.empty_like(vertices)
    v[new_id] = vertices
    t = new_id[tri][rng.permutation(F)]
    shift = rng.integers(0, 3, F)
    t = np.stack([t[np.arange(F), (shift + k) % 3] for k in range(3)], 1).astype(np.int32)
    if colors is None:
        return v, t
    c = np.empty_like(colors)
    c[new_id] = colors
    return v, t, c


def strip(n=4099):
    """n triangles in one strip: vertex i at (i // 2, i % 2, 0), triangle i = (i, i + 1, i + 2) (alternating winding)."""
    i = np.arange(n + 2)
    v = np.stack([i // 2, i % 2, np.zeros_like(i)], 1).astype(np.float32)
    k = np.arange(n)
    return v, np.stack([k, k + 1, k + 2], 1).astype(np.int32)


def fan(centre, k, first_vertex, radius=1.0, phase=0.0):
    """k triangles round a centre vertex: -> vertices [k + 2, 3], triangles [k, 3] numbered from `first_vertex`."""
    ang = phase + 0.45 * np.arange(k + 1)
    rim = np.asarray(centre, np.float64) + radius * np.stack([np.cos(ang), np.sin(ang), np.zeros(k + 1)], 1)
    v = np.concatenate([np.asarray(centre, np.float64)[None], rim]).astype(np.float32)
    j = np.arange(k)
    return v, (first_vertex + np.stack([np.zeros(k, int), 1 + j, 2 + j], 1)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def beads(count=3000, seed=5):
    """`count` separate fans of 1..12 triangles (every size occurs), ids and order permuted."""
    rng = np.random.default_rng(seed)
    sizes = np.concatenate([np.arange(1, 13), rng.integers(1, 13, count - 12)])
    vs, ts, n = [], [], 0
    for b, k in enumerate(sizes.tolist()):
        v, t = fan((4.0 * (b % 64), 4.0 * (b // 64), 0.25 * (b % 7)), k, n, phase=0.1 * (b % 11))
        vs.append(v)
        ts.append(t)
        n += len(v)
    v, t = permuted(np.concatenate(vs), np.concatenate(ts), seed + 1)
    v.setflags(write=False)
    t.setflags(write=False)
    return v, t


def two_fans_at_a_vertex():
    """Two fans of three triangles that share their centre vertex only -> 2 components."""
    t = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 5, 6], [0, 6, 7], [0, 7, 8]], np.int32)
    ang = np.array([0.0, 0.5, 1.0, 1.5, 3.0, 3.5, 4.0, 4.5])
    v = np.concatenate([[[0, 0, 0]], np.stack([np.cos(ang), np.sin(ang), 0 * ang], 1)]).astype(np.float32)
    return v, t, np.array([0, 0, 0, 3, 3, 3], np.int32)


def two_fans_at_an_edge(same_direction=False):
    """Two fans whose border triangles share the edge (0, 1) -> 1 component.  The shared edge is listed as (0, 1) in
    one face and (1, 0) in the other, or as (0, 1) in both."""
    second = [0, 1, 4] if same_direction else [1, 0, 4]
    t = np.array([[0, 1, 2], [0, 2, 3], second, [0, 4, 5]], np.int32)
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [1, -1, 0], [0, -1, 0.5]], np.float32)
    return v, t, np.zeros(4, np.int32)


def three_faces_on_an_edge():
    """Three triangles on the edge (0, 1) -> 1 component."""
    t = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32)
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], np.float32)
    return v, t, np.zeros(3, np.int32)


def null_bridge(kind):
    """Fan A = faces 0-2, face 3 = a NULL face, fan B = faces 4-6; A and B meet in vertex 2 only.  -> vertices,
    triangles, expected labels.  Vertices 5-8 are unreferenced rows of NaN.
      collinear:  face 3 = (1, 2, 9), three points of the x axis; it shares the edge (1, 2) with face 0 and the edge
                  (2, 9) with face 4 -- the only bridge between the fans.
      coincident: vertex 13 lies exactly on vertex 9; face 3 = (2, 9, 13) shares (2, 9) with face 4 and (2, 13) with
                  face 0 -- again the only bridge.
      repeated:   face 3 = (2, 9, 2).  A face that repeats an index has ONE proper edge, so it cannot bridge two
                  faces that do not share that edge themselves; it hangs on fan B's edge (2, 9), and what can be
                  checked is that it is not counted: fan B has three faces, not four."""
    v = np.zeros((14, 3), np.float32)
    v[[0, 1, 2, 3, 4]] = [[0, 0, 0], [1, 0, 0], [2, 0, 0], [1, 1, 0], [0, 1, 0]]
    v[[9, 10, 11, 12]] = [[3, 0, 0], [3, 1, 0], [2, 1, 0.5], [4, 1, 0]]
    v[13] = [5, 5, 5]
    v[5:9] = np.nan
    fan_a = [[1, 2, 3], [1, 3, 4], [1, 4, 0]]
    fan_b = [[2, 9, 10], [2, 10, 11], [9, 12, 10]]
    if kind == "collinear":
        bridge = [1, 2, 9]
    elif kind == "coincident":
        v[13] = v[9]
        bridge = [2, 9, 13]
        fan_a = [[13, 2, 3], [13, 3, 4], [13, 4, 0]]
    elif kind == "repeated":
        bridge = [2, 9, 2]
    else:
        raise ValueError(kind)
    t = np.array(fan_a + [bridge] + fan_b, np.int32)
    return v, t, np.array([0, 0, 0, -1, 4, 4, 4], np.int32)


SIX_AT = (7, 3001, 6007, 9001, 12007, 15013)  # face indices of the six orderings of one triple
SIX_ORDER = ((2, 1, 0), (0, 1, 2), (1, 2, 0), (0, 2, 1), (2, 0, 1), (1, 0, 2))  # the lowest index holds a REVERSED one
FAN_REST_AT = (20, 4000, 8000, 16000)  # the other four faces of the fan


@functools.lru_cache(maxsize=None)
def six_orderings():
    """The beads, and between their faces a fan of five triangles one of which occurs in all six orderings, at
    `SIX_AT`.  Alive, the fan has 5 faces (label SIX_AT[0]); counting duplicates it would have 10.
    -> vertices, triangles, the fan's first triangle as its lowest occurrence spells it."""
    vb, tb = beads()
    vf, tf = fan((-10.0, -10.0, 1.0), 5, len(vb))
    first = tf[0]
    rows = {at: first[list(o)] for at, o in zip(SIX_AT, SIX_ORDER)}
    rows.update({at: tf[1 + k] for k, at in enumerate(FAN_REST_AT)})
    at = sorted(rows)
    t = np.insert(np.asarray(tb), [a - k for k, a in enumerate(at)], np.array([rows[a] for a in at], np.int32), axis=0)
    assert all(np.array_equal(t[a], rows[a]) for a in at)
    v = np.concatenate([vb, vf])
    v.setflags(write=False)
    t.setflags(write=False)
    return v, t, first[list(SIX_ORDER[0])].copy()


GRID_N, GRID_DROP = 600, 0.22


@functools.lru_cache(maxsize=None)
def grid(permute, n=GRID_N, drop=GRID_DROP, seed=9):
    """An n x n grid of quads (2 n^2 triangles) of which a random share `drop` is removed: one giant component and
    many of every small size (neighbours over edges: each triangle has three, the giant one survives up to a share
    of about 0.3).  Colours are a function of the vertex.  -> vertices, colours, triangles."""
    rng = np.random.default_rng(seed)
    y, x = np.divmod(np.arange((n + 1) ** 2), n + 1)
    v = np.stack([x, y, 0.001 * (x * y % 17)], 1).astype(np.float32)
    c = np.stack([x / n, y / n, (x ^ y) % 5 / 4.0], 1).astype(np.float32)
    q = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).reshape(-1)
    t = np.stack([np.stack([q, q + 1, q + n + 2], 1), np.stack([q, q + n + 2, q + n + 1], 1)], 1).reshape(-1, 3)
    t = t[rng.random(len(t)) >= drop].astype(np.int32)
    if permute:
        v, t, c = permuted(v, t, seed + 1, c)
    for a in (v, c, t):
        a.setflags(write=False)
    return v, c, t


@functools.lru_cache(maxsize=None)
def grid_reference(permute, min_faces=DEFAULT_MIN):
    v, c, t = grid(permute)
    return clean_reference(v, t, c, min_faces)


def closed_surface_report(tri):
    """-> (every edge on exactly two faces, V - E + F over the referenced vertices)"""
    t = np.asarray(tri, np.int64)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    return bool((counts == 2).all()), int(len(np.unique(t)) - len(counts) + len(t))
