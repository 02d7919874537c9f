"""float64 torch restatement of the contribution walk (include/gsraster.h, gsr_contribution_accumulate; DESIGN.md section
4.21), and the screen-space scenes the contribution tests share.

Per tile, vectorised over the tile's pixels, on the lists as given (``ids``, ``bins``).  The rule is the forward
compositing's: pixel centre = the integer pixel coordinate, sigma = (a dx^2 + c dy^2) / 2 + b dx dy,
alpha = min(0.999, opac exp(-sigma)); an entry with sigma < 0 or alpha < 1/255 is skipped; the walk stops before the
entry that would make T (1 - alpha) <= 1e-4.  With T the transmittance in front of a contributing entry, w = alpha T:

    max_w[g]    = the largest w of g's pairs            sum_w[g] = the sum of w (``dtype``)
    sum_q[g]    = the sum of floor(w 2^24) (int64)      hits[g]  = the number of pairs
    dominant[g] = the number of pixels whose largest w is g's entry (of equal weights the front-most entry)

Decision stability, with the margins of tests/distortion_reference.py: a (pixel, entry) pair is
*near* when its alpha is within 1e-5 relative of 1/255 or of the clamp, its sigma within 1e-6 of 0, or its next_T within
1e-5 relative of 1e-4.  ``near[g]``: any pair of g is near.  ``tie_pixels`` [H,W]: the pixel's two largest w lie within
1e-5 relative of each other; ``near_tie[g]``: g holds one of the two at such a pixel.

``dtype=torch.float32`` with the float64 run's ``decisions`` gives the same weights in float32; `e32_of` is the largest
|w32 - w64| over the contributing pairs: the float32 error of w itself."""
import numpy as np
import torch

import absgrad_reference as A
import distortion_reference as D

ALPHA_MIN, ALPHA_MAX, T_EPS = D.ALPHA_MIN, D.ALPHA_MAX, D.T_EPS
Q_ONE = float(1 << 24)
STATS = ("max_w", "sum_q", "hits", "dominant")


def _walk(px, py, g, xy, co, op, dtype, decisions=None):
    """One tile: pixels (px, py) [P], list entries g [L] (front to back) -> the weights [P,L] (0 where the pair does not
    contribute), the contributing mask, the near mask, and the final T [P]."""
    P, L = px.numel(), g.numel()
    a, b, c = co[g, 0][None, :], co[g, 1][None, :], co[g, 2][None, :]
    dx, dy = xy[g, 0][None, :] - px[:, None], xy[g, 1][None, :] - py[:, None]
    sigma = 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy
    raw = op[g][None, :] * torch.exp(-sigma)
    alpha = torch.clamp(raw, max=ALPHA_MAX)
    T = torch.ones(P, dtype=dtype)
    alive = torch.ones(P, dtype=torch.bool)
    w = torch.zeros((P, L), dtype=dtype)
    contrib = torch.zeros((P, L), dtype=torch.bool)
    near = torch.zeros((P, L), dtype=torch.bool)
    for e in range(L):
        al = alpha[:, e]
        next_T = T * (1.0 - al)
        if decisions is not None:
            cnt = decisions[:, e]
        else:
            skip = (sigma[:, e] < 0.0) | (al < ALPHA_MIN)
            stop = alive & ~skip & (next_T <= T_EPS)
            cnt = alive & ~skip & ~stop
            r, s = raw[:, e], sigma[:, e]
            nr = (torch.abs(r - ALPHA_MIN) <= 1e-5 * ALPHA_MIN) | (torch.abs(r - ALPHA_MAX) <= 1e-5 * ALPHA_MAX) | \
                (torch.abs(s) <= 1e-6) | (~skip & (torch.abs(next_T - T_EPS) <= 1e-5 * T_EPS))
            near[:, e] = alive & nr
            alive = alive & ~stop
        contrib[:, e] = cnt
        w[:, e] = torch.where(cnt, al * T, torch.zeros_like(T))
        T = torch.where(cnt, next_T, T)
    return w, contrib, near, T


def contribution_reference(H, W, ids, bins, xys, conics, opacities, dtype=torch.float64, decisions=None):
    """-> dict: ``max_w``, ``sum_w`` [N] (``dtype``), ``sum_q``, ``hits``, ``dominant`` [N] int64, ``near``,
    ``near_tie`` [N] bool, ``tie_pixels`` [H,W] bool, ``alpha_img`` [H,W] (1 - final T), ``best`` [H,W] (the dominant
    Gaussian, -1 where nothing contributes), ``decisions`` and ``weights`` (per tile: [P,L])."""
    t = lambda arr: torch.from_numpy(np.ascontiguousarray(np.asarray(arr, np.float32))).to(dtype)  # noqa: E731
    n = np.asarray(xys).shape[0]
    xy, co, op = t(xys).reshape(n, 2), t(conics).reshape(n, 3), t(opacities).reshape(n)
    ids = torch.from_numpy(np.asarray(ids).reshape(-1).astype(np.int64))
    bins = np.asarray(bins).reshape(-1, 2)
    tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
    out = dict(max_w=torch.zeros(n, dtype=dtype), sum_w=torch.zeros(n, dtype=dtype),
               sum_q=torch.zeros(n, dtype=torch.int64), hits=torch.zeros(n, dtype=torch.int64),
               dominant=torch.zeros(n, dtype=torch.int64), near=torch.zeros(n, dtype=torch.bool),
               near_tie=torch.zeros(n, dtype=torch.bool), tie_pixels=torch.zeros((H, W), dtype=torch.bool),
               alpha_img=torch.zeros((H, W), dtype=dtype), best=torch.full((H, W), -1, dtype=torch.long),
               decisions={}, weights={})
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            tile = ty * tiles_x + tx
            lo, hi = int(bins[tile, 0]), int(bins[tile, 1])
            if hi <= lo:
                continue
            rows = torch.arange(ty * 16, min(ty * 16 + 16, H))
            cols = torch.arange(tx * 16, min(tx * 16 + 16, W))
            py, px = (m.reshape(-1) for m in torch.meshgrid(rows, cols, indexing="ij"))
            g = ids[lo:hi]
            w, contrib, near, T = _walk(px.to(dtype), py.to(dtype), g, xy, co, op, dtype,
                                        None if decisions is None else decisions[tile])
            out["decisions"][tile], out["weights"][tile] = contrib, w
            out["alpha_img"][py, px] = 1.0 - T
            out["max_w"][g] = torch.maximum(out["max_w"][g], w.max(dim=0).values)  # (a tile's ids are distinct)
            out["sum_w"].index_add_(0, g, w.sum(dim=0))
            out["sum_q"].index_add_(0, g, torch.floor(w.double() * Q_ONE).to(torch.int64).sum(dim=0))
            out["hits"].index_add_(0, g, contrib.sum(dim=0))
            out["near"][g[near.any(dim=0)]] = True
            # the dominant entry per pixel: the first of the largest (argmax of a strict `>` walk, front to back)
            top = w.max(dim=1).values
            has = top > 0
            first = (w == top[:, None]).to(torch.int8).argmax(dim=1)
            out["dominant"].index_add_(0, g[first[has]], torch.ones(int(has.sum()), dtype=torch.int64))
            out["best"][py[has], px[has]] = g[first[has]]
            if g.numel() >= 2:
                two = torch.topk(w, 2, dim=1)
                tie = has & (two.values[:, 1] > 0) & ((two.values[:, 0] - two.values[:, 1]) <= 1e-5 * two.values[:, 0])
                out["tie_pixels"][py[tie], px[tie]] = True
                out["near_tie"][g[two.indices[tie].reshape(-1)]] = True
    return out


def e32_of(ref64, ref32):
    """max |w32 - w64| over the contributing pairs (0.0 where nothing contributes)."""
    worst = 0.0
    for tile, w in ref64["weights"].items():
        if w.numel():
            worst = max(worst, float((ref32["weights"][tile].double() - w).abs().max()))
    return worst


def near_share(ref):
    """The share of the Gaussians with ``hits > 0`` that a comparison leaves out as near a decision or a tie."""
    seen = ref["hits"] > 0
    return float(((ref["near"] | ref["near_tie"]) & seen).sum()) / max(1, int(seen.sum()))


# ---- the scenes (screen space: what the projection hands to the op) ----------------------------------------------------

def _scene(H, W, xy, sx, sy, rho, opac, depths, rng):
    sc = D._scene(H, W, xy, sx, sy, rho, opac, depths, rng)
    for k in ("values", "v_distortion"):
        sc.pop(k)
    return sc


def scene_edges(seed=0, n=150, shift=(0.0, 0.0)):
    """40 x 24 (W x H): 3 x 2 tiles, partial on the right (8 px) and at the bottom (8 px).  ``shift`` moves every centre:
    a second view of the same Gaussians."""
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.uniform(3, 37, n), rng.uniform(3, 21, n)], 1) + np.asarray(shift, np.float64)
    return _scene(24, 40, xy, rng.uniform(1.5, 6, n), rng.uniform(1.5, 6, n), rng.uniform(-0.4, 0.4, n),
                  rng.uniform(0.05, 0.8, n), 1.0 + 0.02 * rng.permutation(n), rng)


def scene_deep(seed=0, n=600):
    """16 x 16, one tile, 600 Gaussians around the centre: three staging batches of 256.  At the centre the weights add
    up until the stop rule fires inside the second batch; at the corners hardly anything reaches 1/255 and the walk goes
    through all three."""
    rng = np.random.default_rng(seed)
    return _scene(16, 16, rng.uniform(5, 11, (n, 2)), rng.uniform(3, 5, n), rng.uniform(3, 5, n),
                  rng.uniform(-0.3, 0.3, n), rng.uniform(0.02, 0.05, n), 1.0 + 0.01 * rng.permutation(n), rng)


HIDDEN_GROUPS = {"front": 9, "wall": 2, "stopper": 1, "hidden": 50, "faint": 12}


def scene_hidden(seed=0):
    """32 x 32: nine small Gaussians in front (a 3 x 3 grid 10 px apart: no overlap to speak of), a wall of two Gaussians
    200 px wide over the whole image (opacity 0.8, then 1.0: T falls to 2e-4 ... 1.4e-3), a third such Gaussian -- the
    entry at which every pixel's walk stops, which therefore never counts itself -- and behind it 50 small Gaussians
    wholly inside the image; plus twelve of opacity 0.003 < 1/255 in front of everything.  In this order in the arrays
    (`HIDDEN_GROUPS`); the depth order is the same."""
    rng = np.random.default_rng(seed)
    f, h, q = HIDDEN_GROUPS["front"], HIDDEN_GROUPS["hidden"], HIDDEN_GROUPS["faint"]
    gx, gy = np.meshgrid([6.0, 16.0, 26.0], [6.0, 16.0, 26.0])
    front = np.stack([gx.reshape(-1), gy.reshape(-1)], 1) + rng.uniform(-0.4, 0.4, (f, 2))
    centre = np.full((3, 2), 15.5)
    hidden = rng.uniform(8, 24, (h, 2))
    faint = rng.uniform(4, 28, (q, 2))
    xy = np.concatenate([front, centre, hidden, faint])
    sx = np.concatenate([np.full(f, 1.5), np.full(3, 200.0), rng.uniform(0.8, 2.0, h), rng.uniform(2, 4, q)])
    opac = np.concatenate([rng.uniform(0.3, 0.8, f), [0.8, 1.0, 1.0], rng.uniform(0.2, 0.9, h), np.full(q, 0.003)])
    n = xy.shape[0]
    depths = np.concatenate([1.0 + 0.01 * np.arange(f), 2.0 + 0.01 * np.arange(3), 3.0 + 0.01 * np.arange(h),
                             0.5 + 0.01 * np.arange(q)])
    return _scene(32, 32, xy, sx, sx.copy(), np.zeros(n), opac, depths, rng)


def hidden_rows():
    """name -> slice of `scene_hidden`'s arrays."""
    out, at = {}, 0
    for k, m in HIDDEN_GROUPS.items():
        out[k] = slice(at, at + m)
        at += m
    return out


# name -> (builder, seed): the cases tests/test_gpu_contribution.py runs and tests/test_contribution_host.py holds to the
# cap on the near share
CASES = {"edges": (scene_edges, 0), "deep": (scene_deep, 0), "hidden": (scene_hidden, 0)}


def build_case(name):
    fn, seed = CASES[name]
    return fn(seed)


oracle_lists = D.oracle_lists
