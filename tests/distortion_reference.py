"""float64 torch restatement of the depth-distortion walk (include/gsraster.h, gsr_distortion_*)
with AUTOGRAD gradients, and the screen-space scenes the distortion tests share.

Per tile, vectorised over the tile's pixels, on the lists as given (``ids``, ``bins``).  The rule is the forward
compositing's: pixel centre = the integer pixel coordinate, sigma = (a dx^2 + c dy^2) / 2 + b dx dy,
alpha = min(0.999, opac exp(-sigma)); an entry with sigma < 0 or alpha < 1/255 is skipped; the walk stops before the
entry that would make T (1 - alpha) <= 1e-4.  With T_i the transmittance before contributing entry i, w_i = alpha_i T_i:

    distortion = 2 sum_i w_i (z_i A_{i-1} - B_{i-1}),   A_i = 1 - T_{i+1},   B_i = sum_{j<=i} w_j z_j
    median     = z_i of the last contributing entry with T_i > 0.5 (the float32 value, 0 where none contributes)

The decisions (skip, stop, the 0.5 crossing) are taken under ``no_grad`` from the float32 inputs' values; the clamp is
``torch.clamp``, whose autograd passes nothing where it is active.  The value is built from differentiable ops, so
v_xy, v_conic, v_opacity and v_values come from autograd -- independent of the closed form the kernel implements.

Decision stability.  A float32 kernel may take a decision the other way when it is within
rounding of flipping.  A (pixel, splat) pair is *near* when its alpha is within 1e-5 relative of 1/255 or of the clamp,
its sigma within 1e-6 of 0, or its next_T within 1e-5 relative of 1e-4.  ``unstable`` marks the pixels with a near
pair, and those where an incoming T is within 1e-6 relative of 0.5 (the median's decision).  ``U[g]`` is the sum of
|term| over the near pairs of Gaussian g, per gradient component -- the term as it is if the pair counts: taken from
the walk where it counted, and from a second walk of that one pixel with the pair forced to count where it did not.
A per-pair term is autograd's gradient w.r.t. the pair's own sigma, opac exp(-sigma) and z, times the chain factor.

``dtype=torch.float32`` with the float64 run's ``decisions`` gives the same values in float32: ``e32``."""
import numpy as np
import torch

import absgrad_reference as A

ALPHA_MIN = 1.0 / 255.0
ALPHA_MAX = 0.999
T_EPS = 1e-4
NAMES = ("v_xy", "v_conic", "v_opacity", "v_values")


def _walk(px, py, g, leaves, dtype, decisions=None, force=None):
    """One tile: pixels (px, py) [P], list entries g [L] (Gaussian ids, front to back) -> dict of per-pixel results and
    the per-pair tensors.  ``decisions``: a contributing mask [P,L] to use instead of deciding; ``force``: pairs
    [P,L] that count whatever the rule says."""
    xy, co, op, z = leaves
    P, L = px.numel(), g.numel()
    a, b, c = co[g, 0][None, :], co[g, 1][None, :], co[g, 2][None, :]
    dx, dy = xy[g, 0][None, :] - px[:, None], xy[g, 1][None, :] - py[:, None]
    sigma = 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy      # [P,L]
    vis = torch.exp(-sigma)
    raw = op[g][None, :] * vis
    zb = z[g][None, :] + torch.zeros((P, 1), dtype=dtype)          # the pair's own z
    alpha = torch.clamp(raw, max=ALPHA_MAX)
    T, B, D = (torch.ones(P, dtype=dtype), torch.zeros(P, dtype=dtype), torch.zeros(P, dtype=dtype))
    alive = torch.ones(P, dtype=torch.bool)
    contrib = torch.zeros((P, L), dtype=torch.bool)
    near = torch.zeros((P, L), dtype=torch.bool)
    near_half = torch.zeros(P, dtype=torch.bool)
    med_e = torch.full((P,), -1, dtype=torch.long)
    last = torch.full((P,), -1, dtype=torch.long)
    for e in range(L):
        al = alpha[:, e]
        next_T = T * (1.0 - al)
        with torch.no_grad():
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
                near_half |= alive & ~skip & (torch.abs(T - 0.5) <= 1e-6 * 0.5)
                if force is not None:
                    f = force[:, e]
                    cnt, stop = cnt | f, stop & ~f
                alive = alive & ~stop
            contrib[:, e] = cnt
            med_e = torch.where(cnt & (T > 0.5), torch.full_like(med_e, e), med_e)
            last = torch.where(cnt, torch.full_like(last, e), last)
        zero = torch.zeros_like(T)
        w = al * T
        D = D + torch.where(cnt, w * (zb[:, e] * (1.0 - T) - B), zero)
        B = B + torch.where(cnt, w * zb[:, e], zero)
        T = torch.where(cnt, next_T, T)
    return dict(D=2.0 * D, B=B, T=T, med_e=med_e, last=last, contrib=contrib, near=near, near_half=near_half,
                pair=(sigma, raw, zb), chain=(a * dx + b * dy, b * dx + c * dy, 0.5 * dx * dx, dx * dy, 0.5 * dy * dy, vis))


def _pair_terms(loss, walk):
    """autograd's per-pair gradients -> the four per-pair terms [P,L,k] of v_xy, v_conic, v_opacity, v_values."""
    v_sigma, v_raw, v_z = torch.autograd.grad(loss, walk["pair"], retain_graph=True, allow_unused=True)
    tx, ty, caa, cab, cac, vis = (t.detach() for t in walk["chain"])
    zero = torch.zeros_like(tx)
    v_sigma = zero if v_sigma is None else v_sigma
    v_raw = zero if v_raw is None else v_raw
    v_z = zero if v_z is None else v_z
    return (torch.stack([v_sigma * tx, v_sigma * ty], -1), torch.stack([v_sigma * caa, v_sigma * cab, v_sigma * cac], -1),
            (v_raw * vis)[..., None], v_z[..., None])


def distortion_reference(H, W, ids, bins, xys, conics, opacities, values, v_distortion=None, dtype=torch.float64,
                         decisions=None):
    """-> dict: ``distortion``, ``vsum``, ``final_T`` [H,W] (``dtype``), ``median`` [H,W] float32, ``final_idx`` [H,W]
    (list index, -1 where nothing contributes), ``unstable`` [H,W] bool, ``decisions`` (per tile; pass them to a
    float32 run), and with ``v_distortion`` [H,W]: ``v_xy`` [N,2], ``v_conic`` [N,3], ``v_opacity`` [N], ``v_values``
    [N] by autograd and the slack ``U`` (a dict by the same names)."""
    t = lambda arr: torch.from_numpy(np.ascontiguousarray(np.asarray(arr, np.float32))).to(dtype)  # noqa: E731
    n = np.asarray(xys).shape[0]
    leaves = [t(xys).reshape(n, 2), t(conics).reshape(n, 3), t(opacities).reshape(n), t(values).reshape(n)]
    want_grad = v_distortion is not None
    for leaf in leaves:
        leaf.requires_grad_(want_grad)
    z32 = torch.from_numpy(np.asarray(values, np.float32).reshape(n))
    ids = torch.from_numpy(np.asarray(ids).reshape(-1).astype(np.int64))
    bins = np.asarray(bins).reshape(-1, 2)
    vD = None if not want_grad else t(v_distortion).reshape(H, W)
    tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
    out = dict(distortion=torch.zeros((H, W), dtype=dtype), vsum=torch.zeros((H, W), dtype=dtype),
               final_T=torch.ones((H, W), dtype=dtype), median=torch.zeros((H, W), dtype=torch.float32),
               final_idx=torch.full((H, W), -1, dtype=torch.long), unstable=torch.zeros((H, W), dtype=torch.bool),
               decisions={})
    shapes = ((n, 2), (n, 3), (n, 1), (n, 1))
    grads = [torch.zeros(s, dtype=dtype) for s in shapes]
    U = [torch.zeros(s, dtype=dtype) for s in shapes]
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            tile = ty * tiles_x + tx
            lo, hi = int(bins[tile, 0]), int(bins[tile, 1])
            if hi <= lo:
                continue
            rows = torch.arange(ty * 16, min(ty * 16 + 16, H))
            cols = torch.arange(tx * 16, min(tx * 16 + 16, W))
            py, px = (m.reshape(-1) for m in torch.meshgrid(rows, cols, indexing="ij"))
            fpx, fpy = px.to(dtype), py.to(dtype)
            g = ids[lo:hi]
            wk = _walk(fpx, fpy, g, leaves, dtype, None if decisions is None else decisions[tile])
            out["decisions"][tile] = wk["contrib"]
            out["distortion"][py, px] = wk["D"].detach()
            out["vsum"][py, px] = wk["B"].detach()
            out["final_T"][py, px] = wk["T"].detach()
            has = wk["med_e"] >= 0
            out["median"][py, px] = torch.where(has, z32[g[wk["med_e"].clamp(min=0)]], torch.zeros(()))
            out["final_idx"][py, px] = torch.where(wk["last"] >= 0, wk["last"] + lo, wk["last"])
            out["unstable"][py, px] = wk["near"].any(dim=1) | wk["near_half"]
            if not want_grad:
                continue
            vp = vD[py, px]
            loss = (wk["D"] * vp).sum()
            near = wk["near"]
            if near.any():
                counted = near & wk["contrib"]
                terms = _pair_terms(loss, wk)
                for k in range(4):
                    U[k].index_add_(0, g, (terms[k].abs() * counted[..., None]).sum(dim=0))
                # near pairs the rule decided against: the term they have if they count, from a walk of that one pixel
                for p, e in torch.nonzero(near & ~wk["contrib"]).tolist():
                    force = torch.zeros((1, g.numel()), dtype=torch.bool)
                    force[0, e] = True
                    w1 = _walk(fpx[p:p + 1], fpy[p:p + 1], g, leaves, dtype, force=force)
                    t1 = _pair_terms((w1["D"] * vp[p:p + 1]).sum(), w1)
                    for k in range(4):
                        U[k][g[e]] += t1[k][0, e].abs()
            got = torch.autograd.grad(loss, leaves, allow_unused=True)
            for k in range(4):
                if got[k] is not None:
                    grads[k] += got[k].reshape(shapes[k])
    if want_grad:
        for k, name in enumerate(NAMES):
            out[name] = grads[k].reshape(shapes[k] if k < 2 else (n,))
        out["U"] = {name: U[k].reshape(shapes[k] if k < 2 else (n,)) for k, name in enumerate(NAMES)}
    return out


def double_sum(w, z):
    """sum_i sum_j w_i w_j |z_i - z_j| (float64 NumPy), what the O(n) form equals for z sorted along the list."""
    w, z = np.asarray(w, np.float64), np.asarray(z, np.float64)
    return float((w[:, None] * w[None, :] * np.abs(z[:, None] - z[None, :])).sum())


def e32_of(ref64, ref32, names=("distortion", "vsum", "final_T"), keep=None):
    """max|X32 - X64| / max|X64| per forward map (over ``keep`` pixels): the restatement's own float32 error."""
    res = {}
    for k in names:
        a, b = ref64[k].double(), ref32[k].double()
        if keep is not None:
            a, b = a[keep], b[keep]
        res[k] = float((a - b).abs().max() / a.abs().max().clamp(min=1e-300)) if a.numel() else 0.0
    return res


# ---- the scenes (screen space: what the projection hands to the op) ----------------------------------------------------

def _scene(H, W, xy, sx, sy, rho, opac, depths, rng, values=None):
    sc = A._finish(H, W, np.asarray(xy, np.float64), np.asarray(sx, np.float64), np.asarray(sy, np.float64),
                   np.asarray(rho, np.float64), np.asarray(opac, np.float64), rng)
    sc["depths"] = np.asarray(depths, np.float32)
    sc["values"] = sc["depths"].copy() if values is None else np.asarray(values, np.float32)
    sc["v_distortion"] = rng.uniform(-1.0, 1.0, (H, W)).astype(np.float32)
    for k in ("colors", "background"):
        sc.pop(k)
    return sc


def scene_single(seed=0):
    """1 x 1 image, one Gaussian."""
    rng = np.random.default_rng(seed)
    return _scene(1, 1, [[0.2, -0.1]], [2.0], [2.5], [0.1], [0.7], [2.0], rng)


def scene_equal_depth(seed=0):
    """16 x 16, two Gaussians at the same depth (the order is the sort's; the term between them is zero)."""
    rng = np.random.default_rng(seed)
    return _scene(16, 16, [[5.3, 6.1], [9.2, 8.4]], [4.0, 5.0], [5.0, 3.5], [0.2, -0.3], [0.6, 0.5], [1.5, 1.5], rng)


def scene_deep(seed=0, n=600):
    """16 x 16, 600 wide translucent Gaussians that all cover the tile: a list of 600 entries (more than two LDS batches
    of 256) that no pixel saturates.  The values are a non-monotone function of the depths: the kernel does not care."""
    rng = np.random.default_rng(seed)
    depths = 1.0 + 0.01 * rng.permutation(n)
    return _scene(16, 16, rng.uniform(2, 14, (n, 2)), rng.uniform(8, 14, n), rng.uniform(8, 14, n),
                  rng.uniform(-0.5, 0.5, n), rng.uniform(0.006, 0.02, n), depths, rng,
                  values=depths + 0.5 * np.sin(3.0 * depths))


def scene_opaque(seed=0, n=40):
    """16 x 16, a stack of 40 Gaussians of opacity 0.85 to 0.95 over the whole tile: T falls below 1e-4 after about
    five entries, so every pixel meets the stop rule inside the first batch."""
    rng = np.random.default_rng(seed)
    return _scene(16, 16, rng.uniform(6, 10, (n, 2)), rng.uniform(20, 30, n), rng.uniform(20, 30, n), np.zeros(n),
                  rng.uniform(0.85, 0.95, n), 1.0 + 0.05 * rng.permutation(n), rng)


def scene_clamp(seed=0):
    """16 x 16: a Gaussian of opacity 0.9995 on the centre of pixel (8, 8) -- 0.05 px beside it, so that
    sigma = 1.25e-5: exactly on the centre sigma is 0, which the stability rule itself counts as within 1e-6 of the
    ``sigma < 0`` decision, and the pixel would leave the checks.  opac exp(-sigma) = 0.99949 > 0.999: clamped at that
    pixel alone.  A faint Gaussian in front of it and five behind."""
    rng = np.random.default_rng(seed)
    xy = np.concatenate([[[8.05, 8.0], [7.3, 9.4]], rng.uniform(3, 13, (5, 2))])
    sx = np.concatenate([[10.0, 6.0], rng.uniform(3, 6, 5)])
    opac = np.concatenate([[0.9995, 0.1], rng.uniform(0.3, 0.6, 5)])
    depths = np.concatenate([[1.5, 1.0], 2.0 + 0.1 * np.arange(5)])
    return _scene(16, 16, xy, sx, sx.copy(), np.zeros(7), opac, depths, rng)


def scene_partial(seed=0, n=60):
    """17 x 33 (H x W): partial tiles in both axes, 2 x 3 tiles.  Values: 2DGS's map of the depths (near 0.2, far 100)."""
    rng = np.random.default_rng(seed)
    depths = 1.0 + 0.05 * rng.permutation(n)
    return _scene(17, 33, np.stack([rng.uniform(0, 33, n), rng.uniform(0, 17, n)], 1), rng.uniform(1.5, 6, n),
                  rng.uniform(1.5, 6, n), rng.uniform(-0.4, 0.4, n), rng.uniform(0.05, 0.8, n), depths, rng,
                  values=100.0 / 99.8 * (1.0 - 0.2 / depths))


def scene_empty_tile(seed=0, n=150):
    """48 x 64 (H x W): 3 x 4 tiles; small Gaussians everywhere but the bottom-right tile, whose list stays empty."""
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.uniform(0, 64, 4 * n), rng.uniform(0, 48, 4 * n)], 1)
    xy = xy[~((xy[:, 0] > 40) & (xy[:, 1] > 24))][:n]  # (3-sigma radius <= 7.5 px: 8 px off the tile's edges)
    n = xy.shape[0]
    return _scene(48, 64, xy, rng.uniform(1.0, 2.5, n), rng.uniform(1.0, 2.5, n), rng.uniform(-0.3, 0.3, n),
                  rng.uniform(0.05, 0.9, n), 1.0 + 0.02 * rng.permutation(n), rng)


# name -> (builder, seed): the cases tests/test_gpu_distortion.py runs and tests/test_distortion_host.py holds to the
# stability cap
CASES = {"single": (scene_single, 0), "equal_depth": (scene_equal_depth, 0), "deep": (scene_deep, 0),
         "opaque": (scene_opaque, 0), "clamp": (scene_clamp, 0), "partial": (scene_partial, 0),
         "empty_tile": (scene_empty_tile, 0)}


def build_case(name):
    fn, seed = CASES[name]
    return fn(seed)


def oracle_lists(sc):
    """The bounding-box lists of a scene from the CPU oracle -> (ids, bins); what ``rasterizer.utils``' binning entries
    build on the GPU."""
    from oracle import oracle as O

    H, W = sc["H"], sc["W"]
    tb = ((W + 15) // 16, (H + 15) // 16, 1)
    n = sc["xys"].shape[0]
    I, cum = O.compute_cumulative_intersects(sc["num_tiles_hit"])
    _, _, _, ids, bins = O.bin_and_sort_gaussians(n, I, sc["xys"], sc["depths"], sc["radii"], cum, tb, 16)
    return ids, bins


def stability(ref):
    """-> (share of unstable pixels, share of Gaussians with any slack)."""
    any_u = torch.zeros(ref["U"]["v_opacity"].shape[0], dtype=torch.bool)
    for u in ref["U"].values():
        any_u |= (u.reshape(any_u.shape[0], -1) > 0).any(dim=1)
    return float(ref["unstable"].float().mean()), float(any_u.float().mean())
