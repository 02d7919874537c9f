"""float64 NumPy restatement of the compositing backward's rule for the screen-space gradient ``v_xy`` and for the
absgrad (include/gsraster.h, gsr_rasterize_backward_abs), and the synthetic screen-space scenes the absgrad tests share.

The rule (csrc/raster_bwd.hip header; 16 x 16 tiles, pixel centre = the integer pixel coordinate): every pixel with
final_T < 1 re-walks its tile's list back to front from its own ``final_idx``, and for every entry with
``sigma >= 0`` and ``alpha = min(0.99, opac exp(-sigma)) >= 1/255``

    ra = 1 / (1 - alpha);  T *= ra;  fac = alpha T
    v_alpha = sum_c (rgb_c T - buffer_c ra) v_out_c + T_final ra v_out_alpha - T_final ra sum_c bg_c v_out_c
    buffer += rgb fac
    v_sigma = -opac vis v_alpha
    v_xy(p, g) = v_sigma (a dx + b dy, b dx + c dy),   (dx, dy) = xy_g - pixel

``v_xy[g]`` is the sum of v_xy(p, g) over the pixels, ``v_xy_abs[g]`` the sum of |v_xy(p, g)| per component.

Decisions are taken in float64 on the float32 inputs; a float32 kernel may decide a pair the other way when the
decision is within rounding of flipping.  ``U[g]`` (the decision-stability rule) is the sum of
|term| per component over the (pixel, splat) pairs whose alpha is within 1e-5 relative of 1/255 or whose sigma is
within 1e-6 of 0: the slack a comparison grants Gaussian g.
"""
import numpy as np

ALPHA_MIN = 1.0 / 255.0
ALPHA_MAX_BWD = 0.99


def tile_entries(tile, bins, bins2=None, idx_base2=0):
    """Indices into the sorted id array of one tile's list, front to back: its range in ``bins`` followed by its
    range in ``bins2`` (two-round lists, relative to ``idx_base2``)."""
    e = np.arange(int(bins[tile, 0]), int(bins[tile, 1]), dtype=np.int64)
    if bins2 is not None:
        e = np.concatenate([e, np.arange(int(bins2[tile, 0]), int(bins2[tile, 1]), dtype=np.int64) + int(idx_base2)])
    return e


def absgrad_reference(H, W, ids, bins, xys, conics, colors, opacities, background, final_Ts, final_idx, v_out,
                      v_out_alpha=None, bins2=None, idx_base2=0, block=16):
    """-> (v_xy [N,2], v_xy_abs [N,2], U [N,2]) in float64.

    ``colors`` [N,C], ``v_out`` [H,W,C], ``background`` [C] with any C (RGB + one extra channel: C = 4)."""
    f8 = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    xys, conics, colors, bg = f8(xys), f8(conics), f8(colors), f8(background).reshape(-1)
    opac = f8(opacities).reshape(-1)
    n = xys.shape[0]
    final_Ts, v_out = f8(final_Ts), f8(v_out).reshape(H, W, -1)
    final_idx = np.asarray(final_idx).astype(np.int64)
    v_oa = np.zeros((H, W)) if v_out_alpha is None else f8(v_out_alpha).reshape(H, W)
    ids = np.asarray(ids).reshape(-1).astype(np.int64)
    bins = np.asarray(bins).reshape(-1, 2)
    if bins2 is not None:
        bins2 = np.asarray(bins2).reshape(-1, 2)
    tiles_x, tiles_y = (W + block - 1) // block, (H + block - 1) // block
    v_xy, v_abs, U = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros((n, 2))
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            entries = tile_entries(ty * tiles_x + tx, bins, bins2, idx_base2)
            if entries.size == 0:
                continue
            rows = np.arange(ty * block, min((ty + 1) * block, H))
            cols = np.arange(tx * block, min((tx + 1) * block, W))
            py, px = (a.reshape(-1) for a in np.meshgrid(rows, cols, indexing="ij"))
            Tf = final_Ts[py, px]
            drawn = Tf < 1.0
            fidx = np.where(drawn, final_idx[py, px], -1)
            vo = v_out[py, px]                                  # [P,C]
            tail = Tf * (v_oa[py, px] - vo @ bg)                # T_final (v_out_alpha - bg . v_out)
            T = Tf.copy()
            buf = np.zeros_like(vo)
            fpx, fpy = px.astype(np.float64), py.astype(np.float64)
            for e in entries[::-1]:
                live = e <= fidx
                if not live.any():
                    continue
                g = ids[e]
                a, b, c = conics[g]
                dx, dy = xys[g, 0] - fpx, xys[g, 1] - fpy
                sigma = 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy
                vis = np.exp(-sigma)
                alpha_raw = opac[g] * vis
                alpha = np.minimum(ALPHA_MAX_BWD, alpha_raw)
                valid = live & (sigma >= 0.0) & (alpha >= ALPHA_MIN)
                near = live & ((np.abs(alpha_raw - ALPHA_MIN) <= 1e-5 * ALPHA_MIN) | (np.abs(sigma) <= 1e-6))
                if not (valid.any() or near.any()):
                    continue
                al = np.where(valid, alpha, 0.0)
                ra = 1.0 / (1.0 - al)
                Tn = T * ra
                # what the pair contributes if it counts (also for a near pair that this side decided against)
                ra_c = 1.0 / (1.0 - alpha)
                Tc = T * ra_c
                v_alpha = ((colors[g] * Tc[:, None] - buf * ra_c[:, None]) * vo).sum(axis=1) + ra_c * tail
                v_sigma = -opac[g] * vis * v_alpha
                tx_, ty_ = v_sigma * (a * dx + b * dy), v_sigma * (b * dx + c * dy)
                v_xy[g, 0] += tx_[valid].sum()
                v_xy[g, 1] += ty_[valid].sum()
                v_abs[g, 0] += np.abs(tx_[valid]).sum()
                v_abs[g, 1] += np.abs(ty_[valid]).sum()
                if near.any():
                    U[g, 0] += np.abs(tx_[near]).sum()
                    U[g, 1] += np.abs(ty_[near]).sum()
                fac = al * Tn
                buf += colors[g][None, :] * fac[:, None]
                T = Tn
    return v_xy, v_abs, U


def within_bound(got, ref, U):
    """The bound the GPU tests hold the kernel to: |got - ref| <= 1e-3 max(ref_g, 1e-3 max ref) + U_g, elementwise.
    -> (ok: bool, worst ratio of the error to its bound)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bound = 1e-3 * np.maximum(np.abs(ref), 1e-3 * np.abs(ref).max()) + U
    err = np.abs(got - ref)
    tiny = np.finfo(np.float64).tiny
    return bool((err <= bound).all()), float((err / np.maximum(bound, tiny)).max())


def slack_fraction(U):
    """The share of the Gaussians with any slack (the tests cap it at 5 %)."""
    return float((np.asarray(U) > 0).any(axis=1).mean())


# ---- synthetic scenes in screen space (what the projection would hand to rasterize_gaussians) -------------------------

def _finish(H, W, xy, sx, sy, rho, opac, rng):
    """conics / radii / num_tiles_hit of Gaussians with standard deviations (sx, sy) and correlation rho, the way the
    projection derives them (radius = ceil(3 sqrt(largest eigenvalue)), the tile box of oracle/gsr_oracle.c)."""
    n = xy.shape[0]
    cxx, cyy, cxy = sx * sx, sy * sy, rho * sx * sy
    det = cxx * cyy - cxy * cxy
    conics = np.stack([cyy / det, -cxy / det, cxx / det], axis=1).astype(np.float32)
    mid = 0.5 * (cxx + cyy)
    lam = mid + np.sqrt(np.maximum(0.1, mid * mid - det))
    radii = np.ceil(3.0 * np.sqrt(lam)).astype(np.int32)
    xy = xy.astype(np.float32)
    tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
    tc, tr = xy / np.float32(16), (radii.astype(np.float32) / np.float32(16))[:, None]
    lo = np.clip((tc - tr).astype(np.int32), 0, [tiles_x, tiles_y])
    hi = np.clip((tc + tr + np.float32(1)).astype(np.int32), 0, [tiles_x, tiles_y])
    tiles = ((hi[:, 0] - lo[:, 0]) * (hi[:, 1] - lo[:, 1])).astype(np.int32)
    assert (tiles > 0).all()
    depths = rng.permutation(n).astype(np.float32) * np.float32(0.01) + np.float32(1.0)  # distinct: one depth order
    return dict(xys=xy, depths=depths, radii=radii, conics=conics, num_tiles_hit=tiles,
                opacities=opac.astype(np.float32).reshape(n, 1),
                colors=rng.uniform(0.05, 1.0, (n, 3)).astype(np.float32),
                background=np.array([0.2, 0.5, 0.3], np.float32), H=H, W=W)


def _cotangents(sc, rng):
    H, W = sc["H"], sc["W"]
    sc["v_img"] = rng.uniform(-1, 1, (H, W, 3)).astype(np.float32)
    sc["v_alpha"] = rng.uniform(-1, 1, (H, W)).astype(np.float32)
    sc["v_extra"] = rng.uniform(-1, 1, (H, W)).astype(np.float32)
    return sc


# the 40 x 24 scene's Gaussians by the tiles they reach (3 x 2 tiles: columns 16 + 16 + 8 px, rows 16 + 8 px)
SMALL_COUNTS = {"all": 1, "row3": 69, "row2": 31, "col": 22, "own": 7}
SMALL_LIST_LENGTHS = [130, 101, 70, 23, 1, 1]  # tiles (0,0) (1,0) (2,0) (0,1) (1,1) (2,1)


def small_scene(seed=0):
    """40 x 24 (3 x 2 tiles, partial edge tiles), 130 Gaussians placed so that the tiles' lists hold 130, 101, 70, 23,
    1 and 1 entries: across the 64-entry chunk, lengths that are no multiple of 4, on both sides of the small-grid split
    threshold (96).  Every Gaussian reaches tile (0,0); who else it reaches is decided with a wide margin (several
    sigma), so the list lengths do not hang on a rounding."""
    rng = np.random.default_rng(seed)
    kinds = sum(([k] * c for k, c in SMALL_COUNTS.items()), [])
    n = len(kinds)
    xy, sx, sy = np.zeros((n, 2)), np.zeros(n), np.zeros(n)
    for i, k in enumerate(kinds):
        j = rng.uniform(-1.5, 1.5, 2)
        s = rng.uniform(0.85, 1.15, 2)
        if k == "all":    # every tile
            xy[i], sx[i], sy[i] = (20, 12) + j, 12 * s[0], 12 * s[1]
        elif k == "row3":  # the top row's three tiles
            xy[i], sx[i], sy[i] = (24, 8) + j, 8 * s[0], 1.5 * s[1]
        elif k == "row2":  # tiles (0,0) and (1,0)
            xy[i], sx[i], sy[i] = (16, 8) + j, 3 * s[0], 1.5 * s[1]
        elif k == "col":   # tiles (0,0) and (0,1)
            xy[i], sx[i], sy[i] = (8, 16) + j, 1.5 * s[0], 3 * s[1]
        else:              # tile (0,0) alone
            xy[i], sx[i], sy[i] = (8, 8) + j, 1.5 * s[0], 1.5 * s[1]
    perm = rng.permutation(n)
    sc = _finish(24, 40, xy[perm], sx[perm], sy[perm], np.zeros(n), rng.uniform(0.05, 0.4, n), rng)
    return _cotangents(sc, rng)


def deep_scene(seed=0, n=1500):
    """32 x 32 (four tiles), 1 500 wide translucent Gaussians that all reach all four tiles: lists of 1 500 entries
    (> 1 024) that no pixel saturates early, so every depth-segment run carries live pixels."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(8, 24, (n, 2))
    sx, sy = rng.uniform(8, 14, n), rng.uniform(8, 14, n)
    rho = rng.uniform(-0.5, 0.5, n)
    sc = _finish(32, 32, xy, sx, sy, rho, rng.uniform(0.006, 0.02, n), rng)
    return _cotangents(sc, rng)


def single_splat_scene():
    """One Gaussian wholly to one side of a 16 x 16 image (x_g < 0: dx < 0 at every pixel), b = 0, and cotangents of
    one sign (v_img > 0, no alpha cotangent, black background): every per-pixel v_xy_x has the same sign, so the
    absgrad's x component equals |v_xy_x| up to the rounding of 256 same-sign additions."""
    rng = np.random.default_rng(5)
    sc = _finish(16, 16, np.array([[-3.0, 7.5]]), np.array([9.0]), np.array([9.0]), np.zeros(1), np.array([0.6]), rng)
    sc["background"] = np.zeros(3, np.float32)
    sc["v_img"] = rng.uniform(0.2, 1.0, (16, 16, 3)).astype(np.float32)
    sc["v_alpha"] = np.zeros((16, 16), np.float32)
    sc["v_extra"] = np.zeros((16, 16), np.float32)
    return sc


def oracle_lists(sc):
    """The reference's bounding-box lists and its float32 forward for a scene -> (ids, bins, final_Ts, final_idx).
    (The package's 16-px lists leave out entries that reach no pixel: other indices, the same contributions.)"""
    from oracle import oracle as O

    H, W = sc["H"], sc["W"]
    tb = ((W + 15) // 16, (H + 15) // 16, 1)
    n = sc["xys"].shape[0]
    I, cum = O.compute_cumulative_intersects(sc["num_tiles_hit"])
    _, _, _, ids, bins = O.bin_and_sort_gaussians(n, I, sc["xys"], sc["depths"], sc["radii"], cum, tb, 16)
    _, Ts, idx = O.rasterize_forward(tb, (16, 16, 1), (W, H, 1), ids, bins, sc["xys"], sc["conics"], sc["colors"],
                                     sc["opacities"], sc["background"])
    return ids, bins, Ts, idx
