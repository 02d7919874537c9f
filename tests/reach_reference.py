"""float64 truth for the two reach culls, a float32 NumPy emulation of the 16-px row rule, and seeded screen-space
families built to graze them.

The culls (csrc/tile_rows.h ``make_row_params`` / ``row_range``: which 16-px tiles of its box a splat is listed in;
csrc/raster_common.h ``make_reach`` / ``reaches_rect`` / ``splat_reach_mask``: which 8 x 8 sub-tiles of a tile a staged
splat is composited in) may only leave out a (splat, rectangle) pair in which no pixel passes the compositing rule's
``alpha = opac exp(-sigma) >= 1/255``.  Inputs are screen-space arrays as ``tests/absgrad_reference.py::_finish`` makes
them (float32 / int32); every decision here is taken in float64 on those float32 values.

* ``live_pairs``     per (splat, rectangle) of the splat's tile box: the largest alpha over the rectangle's pixels
* ``composite64``    the forward rule of csrc/raster_fwd.hip in float64, with the oracle's ``ambig_eps = 1e-5`` flag
* ``row_rule32``     the list rule in float32, one rounding per operation, its three margins as parameters
* ``family(name)``   graze16 / graze8 (ellipses that reach ONE pixel of a rectangle by a relative margin delta in
                     alpha, and their mirrors that miss it by delta), needles, tiny, norule
"""
import functools

import numpy as np

ALPHA_MIN = 1.0 / 255.0
SLACK = 1e-5           # decision slack (the oracle's ambig_eps)
DELTAS = (1e-3, 3e-3, -1e-3, -3e-3)
MUST_KEEP, UNDECIDED, DEAD = 2, 1, 0
F = np.float32


def _f8(a):
    return np.asarray(a, dtype=np.float64)


# ---- the tile box (csrc/gsr_common.h gsr_tile_bbox, in float32 as _finish restates it) ---------------------------------

def tile_box(xys, radii, tiles_x, tiles_y):
    """-> int32 [N,4] (minx, miny, maxx, maxy) in 16-px tiles, max exclusive; radius <= 0: an empty box."""
    xy = np.asarray(xys, F)
    tc, tr = xy / F(16), (np.asarray(radii).astype(F) / F(16))[:, None]
    with np.errstate(invalid="ignore"):
        lo = np.clip((tc - tr).astype(np.int64), 0, [tiles_x, tiles_y])
        hi = np.clip((tc + tr + F(1)).astype(np.int64), 0, [tiles_x, tiles_y])
    box = np.concatenate([lo, hi], axis=1).astype(np.int32)
    box[np.asarray(radii) <= 0] = 0
    return box


def grid(sc):
    return (sc["W"] + 15) // 16, (sc["H"] + 15) // 16


def box_pairs(sc):
    """Every (splat, 16-px tile) of the splats' boxes, splat-major then row-major -> int64 arrays (g, tx, ty)."""
    tiles_x, tiles_y = grid(sc)
    box = tile_box(sc["xys"], sc["radii"], tiles_x, tiles_y)
    gs, txs, tys = [], [], []
    for g, (x0, y0, x1, y1) in enumerate(box):
        if x1 > x0 and y1 > y0:
            ty, tx = np.meshgrid(np.arange(y0, y1), np.arange(x0, x1), indexing="ij")
            gs.append(np.full(tx.size, g)), txs.append(tx.reshape(-1)), tys.append(ty.reshape(-1))
    cat = lambda l: np.concatenate(l).astype(np.int64) if l else np.zeros(0, np.int64)  # noqa: E731
    return cat(gs), cat(txs), cat(tys)


# ---- float64 truth -------------------------------------------------------------------------------------------------------

def _alpha_at(sc, g, px, py):
    """(sigma, alpha) of splat g at float64 pixel coordinates; alpha is 0 where sigma < 0 (the rule skips those)."""
    a, b, c = _f8(sc["conics"][g])
    dx, dy = float(sc["xys"][g, 0]) - px, float(sc["xys"][g, 1]) - py
    sigma = 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy
    with np.errstate(over="ignore", invalid="ignore"):
        alpha = float(sc["opacities"].reshape(-1)[g]) * np.exp(-sigma)
    return sigma, np.where(sigma >= 0.0, alpha, 0.0)


def _band_pixels(sc, g, x0, x1, y0, y1):
    """The pixels of the window [x0, x1) x [y0, y1) that can be live for a positive-definite splat: per row the
    x-interval of the ellipse {sigma <= log(255 opac) + 0.1}, widened by 2 px -- float64, margins far above any
    rounding; every pixel left out has alpha < exp(-0.1) / 255.  None: not applicable (evaluate the whole window)."""
    a, b, c = _f8(sc["conics"][g])
    opac = float(sc["opacities"].reshape(-1)[g])
    D = a * c - b * b
    if not (a > 0 and c > 0 and D > 1e-9 * a * c and opac == opac):
        return None
    if not 255.0 * opac > 0:
        return np.zeros(0), np.zeros(0)
    s = np.log(255.0 * opac) + 0.1
    if s < 0:
        return np.zeros(0), np.zeros(0)
    rows = np.arange(y0, y1, dtype=np.float64)
    v = rows - float(sc["xys"][g, 1])
    disc = 2.0 * a * s - D * v * v
    ok = disc >= 0
    rows, v, disc = rows[ok], v[ok], disc[ok]
    root = np.sqrt(disc)
    cx = float(sc["xys"][g, 0])
    xl = np.maximum(np.floor(cx + (-b * v - root) / a - 2.0), x0).astype(np.int64)
    xr = np.minimum(np.ceil(cx + (-b * v + root) / a + 2.0), x1 - 1).astype(np.int64)
    cnt = np.maximum(xr - xl + 1, 0)
    if cnt.sum() == 0:
        return np.zeros(0), np.zeros(0)
    py = np.repeat(rows, cnt)
    first = np.repeat(np.cumsum(cnt) - cnt, cnt)
    px = np.repeat(xl, cnt) + (np.arange(cnt.sum()) - first)
    return px.astype(np.float64), py


def live_pairs(sc, unit, banded=None):
    """For every (splat, unit x unit rectangle) inside the splat's tile box: ``amax``, the largest
    ``opac exp(-sigma)`` over the rectangle's pixels that lie inside the image and have ``sigma >= 0`` (0 if none), and
    its class -- MUST_KEEP: amax >= (1 + 1e-5) / 255, UNDECIDED: within 1e-5 relative of 1/255, DEAD: the rest.
    -> dict of arrays g, rx, ry (rectangle coordinates in units), amax, cls; unit 16 in the order of `box_pairs`.
    ``banded``: evaluate only the pixels of `_band_pixels` (default: for windows above 2^18 pixels)."""
    assert unit in (16, 8)
    W, H = sc["W"], sc["H"]
    tiles_x, tiles_y = grid(sc)
    box = tile_box(sc["xys"], sc["radii"], tiles_x, tiles_y)
    k = 16 // unit
    out = {n: [] for n in ("g", "rx", "ry", "amax")}
    for g, (bx0, by0, bx1, by1) in enumerate(box):
        if bx1 <= bx0 or by1 <= by0:
            continue
        x0, y0, x1, y1 = bx0 * 16, by0 * 16, min(bx1 * 16, W), min(by1 * 16, H)
        nrx, nry = (bx1 - bx0) * k, (by1 - by0) * k
        amax = np.zeros((nry, nrx))
        band = None
        if banded or (banded is None and (x1 - x0) * (y1 - y0) > (1 << 18)):
            band = _band_pixels(sc, g, x0, x1, y0, y1)
        if band is None:
            py, px = np.meshgrid(np.arange(y0, y1, dtype=np.float64), np.arange(x0, x1, dtype=np.float64), indexing="ij")
            px, py = px.reshape(-1), py.reshape(-1)
        else:
            px, py = band
        if px.size:
            _, alpha = _alpha_at(sc, g, px, py)
            alpha = np.where(alpha == alpha, alpha, np.inf)  # NaN (a NaN opacity) is never < 1/255: it is drawn
            ix, iy = ((px - x0) // unit).astype(np.int64), ((py - y0) // unit).astype(np.int64)
            np.maximum.at(amax, (iy, ix), alpha)
        ry, rx = np.meshgrid(np.arange(nry) + by0 * k, np.arange(nrx) + bx0 * k, indexing="ij")
        inside = (rx * unit < W) & (ry * unit < H)
        out["g"].append(np.full(int(inside.sum()), g)), out["rx"].append(rx[inside]), out["ry"].append(ry[inside])
        out["amax"].append(amax[inside])
    res = {n: (np.concatenate(v) if v else np.zeros(0)) for n, v in out.items()}
    for n in ("g", "rx", "ry"):
        res[n] = res[n].astype(np.int64)
    rel = res["amax"] * 255.0
    res["cls"] = np.where(rel >= 1.0 + SLACK, MUST_KEEP, np.where(rel > 1.0 - SLACK, UNDECIDED, DEAD)).astype(np.int8)
    return res


def composite64(sc, ids, bins):
    """The forward rule of csrc/raster_fwd.hip in float64 over the lists (ids, bins):
    alpha = min(0.999, opac exp(-sigma)); skip on sigma < 0 or alpha < 1/255; a pixel is finished (that splat NOT drawn)
    at T (1 - alpha) <= 1e-4; out = C + T background.
    -> (img [H,W,3], final_T, final_idx (index into ``ids`` of the last drawn entry, 0 if none), unstable [H,W]).
    ``unstable``: a decision of that pixel's walk is within the oracle's ``ambig_eps = 1e-5`` of flipping (the rule of
    oracle/gsr_oracle.c: sigma may move by stol = 1e-5 + 1e-6 x the sum of its terms' magnitudes; |sigma| <= stol,
    |T (1 - alpha) - 1e-4| <= (20 x 1e-5 + stol) 1e-4, and the alpha test where sigma is within stol of
    log(255 opac) -- the oracle's |alpha - 1/255| <= stol / 255 to first order, without its false alarms where
    stol >= 1 and alpha is nowhere near), or an alpha is NaN."""
    H, W = sc["H"], sc["W"]
    tiles_x, tiles_y = grid(sc)
    ids, bins = np.asarray(ids).reshape(-1).astype(np.int64), np.asarray(bins).reshape(-1, 2)
    xys, conics, colors = _f8(sc["xys"]), _f8(sc["conics"]), _f8(sc["colors"])
    opac, bg = _f8(sc["opacities"]).reshape(-1), _f8(sc["background"])
    img, Tf = np.zeros((H, W, 3)), np.ones((H, W))
    fidx, unstable = np.zeros((H, W), np.int64), np.zeros((H, W), bool)
    for t in range(tiles_x * tiles_y):
        lo, hi = int(bins[t, 0]), int(bins[t, 1])
        rows = np.arange((t // tiles_x) * 16, min((t // tiles_x + 1) * 16, H))
        cols = np.arange((t % tiles_x) * 16, min((t % tiles_x + 1) * 16, W))
        py, px = (a.reshape(-1) for a in np.meshgrid(rows, cols, indexing="ij"))
        P = px.size
        T, C = np.ones(P), np.zeros((P, 3))
        last, amb, done = np.zeros(P, np.int64), np.zeros(P, bool), np.zeros(P, bool)
        if hi > lo:
            g = ids[lo:hi]
            a, b, c = conics[g, 0][:, None], conics[g, 1][:, None], conics[g, 2][:, None]
            dx, dy = xys[g, 0][:, None] - px[None, :], xys[g, 1][:, None] - py[None, :]
            sigma = 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy
            stol = SLACK + 1e-6 * (0.5 * (np.abs(a) * dx * dx + np.abs(c) * dy * dy) + np.abs(b * dx * dy))
            with np.errstate(over="ignore", invalid="ignore"):
                raw = opac[g][:, None] * np.exp(-sigma)
            nan = raw != raw
            alpha = np.minimum(0.999, np.where(nan, 0.0, raw))
            valid = (sigma >= 0.0) & (alpha >= ALPHA_MIN) & ~nan
            with np.errstate(divide="ignore", invalid="ignore"):
                bound = np.log(255.0 * opac[g])[:, None]  # alpha >= 1/255  <=>  sigma <= bound
                near = (np.abs(sigma) <= stol) | (np.abs(sigma - bound) <= stol) | nan
            for e in np.nonzero((valid | near).any(axis=1))[0]:
                amb |= near[e] & ~done
                v = valid[e] & ~done
                nT = T * (1.0 - alpha[e])
                amb |= v & (np.abs(nT - 1e-4) <= (20.0 * SLACK + stol[e]) * 1e-4)
                stop = v & (nT <= 1e-4)
                done |= stop
                v &= ~stop
                C[v] += colors[g[e]][None, :] * (alpha[e] * T)[v, None]
                T = np.where(v, nT, T)
                last[v] = lo + e
                if done.all():
                    break
        img[py, px] = C + T[:, None] * bg[None, :]
        Tf[py, px], fidx[py, px], unstable[py, px] = T, last, amb
    return img, Tf, fidx, unstable


# ---- the 16-px list rule in float32, one rounding per operation ----------------------------------------------------------

def conic_det32(a, b, c, plain=False):
    """``conic_det`` of csrc/raster_common.h: a c - b^2 with the rounding error of b b taken back out (each fma is one
    rounding of an exact float64 value: products of two float32 are exact in float64).  ``plain``: the float32
    expression a * c - b * b, three roundings."""
    if plain:
        return (a * c - b * b).astype(F)
    w = (b * b).astype(F)
    e = (_f8(b) * _f8(b) - _f8(w)).astype(F)
    return ((_f8(a) * _f8(c) - _f8(w)).astype(F) - e).astype(F)


def row_rule32(sc, log_margin=0.01, rel_margin=1e-3, px_margin=0.05, plain_det=False):
    """``make_reach`` + ``make_row_params`` + ``row_range`` (csrc/raster_common.h, csrc/tile_rows.h) in NumPy float32:
    every operation rounded on its own, no FMA but the two of `conic_det32`, ``log`` correctly rounded.  The margins are
    the kernel's by default: ``log_margin`` added to log(255 opac), the row interval widened by ``rel_margin`` x extent
    + ``px_margin``.  ``plain_det``: the determinant as the plain float32 expression (the rule before `conic_det`).
    -> bool [pairs]: is the pair of `box_pairs` kept."""
    tiles_x, tiles_y = grid(sc)
    g, tx, ty = box_pairs(sc)
    box = tile_box(sc["xys"], sc["radii"], tiles_x, tiles_y)
    x, y = np.asarray(sc["xys"], F)[:, 0], np.asarray(sc["xys"], F)[:, 1]
    a, b, c = (np.asarray(sc["conics"], F)[:, i] for i in range(3))
    opac = np.asarray(sc["opacities"], F).reshape(-1)
    with np.errstate(all="ignore"):
        smax = np.log(F(255) * opac).astype(F) + F(log_margin)
        smax = np.where(smax >= 0, smax, np.where(opac == opac, F(-1), F(np.inf))).astype(F)
        det = conic_det32(a, b, c, plain_det)
        pd = (a > 0) & (c > 0) & (det > 0)
        smax = np.where(pd, smax, F(np.inf)).astype(F)
        fin = (smax >= 0) & np.isfinite(smax)
        D = np.where(fin, det, F(1)).astype(F)
        t = F(2) * smax / D
        umax = np.where(fin, np.sqrt(t * c), F(0)).astype(F)
        vmax = np.where(fin, np.sqrt(t * a), F(0)).astype(F)
        vstar = np.where(fin, b * umax / c, F(0)).astype(F)
        # per pair
        t0, t1 = box[g, 0].astype(F), box[g, 2].astype(F)
        v0 = F(16) * ty.astype(F) - y[g]
        v1 = v0 + F(15)
        mv, mu = F(rel_margin) * vmax[g] + F(px_margin), F(rel_margin) * umax[g] + F(px_margin)
        out_of_band = (v0 > vmax[g] + mv) | (v1 < -vmax[g] - mv)
        two_as = F(2) * a[g] * smax[g]
        vr = np.minimum(np.maximum(-vstar[g], v0), v1)
        vl = np.minimum(np.maximum(vstar[g], v0), v1)
        inv_a = F(1) / a[g]
        xr = (-b[g] * vr + np.sqrt(np.maximum(two_as - D[g] * vr * vr, F(0)))) * inv_a + mu
        xl = (-b[g] * vl - np.sqrt(np.maximum(two_as - D[g] * vl * vl, F(0)))) * inv_a - mu
        f0 = np.minimum(np.maximum(np.ceil((x[g] + xl - F(15)) * F(0.0625)), t0), t1)
        f1 = np.minimum(np.maximum(np.floor((x[g] + xr) * F(0.0625)) + F(1), t0), t1)
        assert all(v.dtype == F for v in (smax, D, umax, vmax, vstar, v1, mv, two_as, xr, xl, f0, f1))
        i0 = f0.astype(np.int64)
        i1 = np.maximum(f1.astype(np.int64), i0)
        keep = (tx >= i0) & (tx < i1) & ~out_of_band
    keep = np.where(smax[g] == np.inf, True, np.where(smax[g] < 0, False, keep))
    return keep


# ---- scenes ----------------------------------------------------------------------------------------------------------------

def conics_from_cov(l1, l2, theta):
    """float32 conics and radii of ellipses with eigenvalues (l1, l2) px^2 and major-axis angle theta, the way the
    projection derives them from a float32 cov2d (csrc/gsr_common.h gsr_cov2d_bounds: every operation in float32)."""
    l1, l2, theta = _f8(l1), _f8(l2), _f8(theta)
    cs, sn = np.cos(theta), np.sin(theta)
    c0 = (l1 * cs * cs + l2 * sn * sn).astype(F)
    c1 = ((l1 - l2) * sn * cs).astype(F)
    c2 = (l1 * sn * sn + l2 * cs * cs).astype(F)
    with np.errstate(all="ignore"):
        det = c0 * c2 - c1 * c1
        inv = F(1) / det
        conics = np.stack([c2 * inv, -c1 * inv, c0 * inv], axis=-1).astype(F)
        mid = F(0.5) * (c0 + c2)
        lam = mid + np.sqrt(np.maximum(F(0.1), mid * mid - det))
        radii = np.ceil(F(3) * np.sqrt(lam))
    return conics, radii, det


def _scene(H, W, xy, conics, radii, opac, rng, depths=None, color_lo=0.05, background=(0.2, 0.5, 0.3)):
    n = xy.shape[0]
    xy = np.asarray(xy, F)
    radii = np.asarray(radii).astype(np.int32)
    tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
    box = tile_box(xy, radii, tiles_x, tiles_y)
    tiles = ((box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])).astype(np.int32)
    assert (tiles > 0).all()
    if depths is None:
        depths = rng.permutation(n)
    depths = np.asarray(depths).astype(F) * F(0.01) + F(1.0)  # distinct: one depth order
    assert np.unique(depths).size == n
    return dict(xys=xy, depths=depths, radii=radii, conics=np.asarray(conics, F), num_tiles_hit=tiles,
                opacities=np.asarray(opac, F).reshape(n, 1), colors=rng.uniform(color_lo, 1.0, (n, 3)).astype(F),
                background=np.array(background, F), H=H, W=W)


GRAZE_SIZE = 128          # graze images: 8 x 8 whole tiles (the families shift into a larger grid unchanged)
GRAZE_PER_DELTA = 150     # x 4 deltas = 600 splats; the 8 sub-cases below in turn
GRAZE_CASES = ("corner", "edge", "above", "below", "left", "right", "diagonal", "solo")
MAX_TERMS = 200.0         # sum of |terms| of sigma at a target: float32 sigma is then good to ~1e-5 << |delta|


def _graze(unit, seed):
    """Splats that reach exactly ONE pixel (the target) of one unit x unit rectangle (the target rectangle) with
    alpha = (1 + delta) / 255, delta in DELTAS: opac = exp(smin) / 255 (1 + delta), smin the float64 minimum of sigma
    over the rectangle's pixels.  Sub-cases in equal shares (GRAZE_CASES): target at a rectangle corner / on an edge's
    interior; centre straight above / below / left of / right of the rectangle (``vstar`` clamps); centre diagonal to
    it; ``solo``: centre outside the image, the target the splat's only live pixel and the splat that pixel's only
    live one (every other sub-case has more live pixels).  unit 8: the other three sub-tiles of the target's tile are
    farther away (their minimum sigma > smin + 0.05).  At a target pixel at most one other splat is live, T in front
    of the target's own splat stays >= 0.5, and no other splat is within 1e-3 relative of 1/255; no other rectangle of
    a splat is within 1e-4 relative of it.  Centres are multiples of 1/64 px: exact in float32 wherever they move."""
    rng = np.random.default_rng(seed)
    S = GRAZE_SIZE
    w = unit - 1
    nrect = S // unit
    tiles = S // 16
    acc = dict(xy=[], conic=[], radius=[], opac=[], depth=[], target=[], smin=[], delta=[], case=[], rect=[])
    depth_pool = list(rng.permutation(len(DELTAS) * GRAZE_PER_DELTA))
    off = np.arange(unit, dtype=np.float64)
    oy, ox = (v.reshape(-1) for v in np.meshgrid(off, off, indexing="ij"))
    on_edge = (ox == 0) | (ox == w) | (oy == 0) | (oy == w)
    is_corner = ((ox == 0) | (ox == w)) & ((oy == 0) | (oy == w))
    t_px = np.zeros((0, 2))      # accepted targets
    t_depth, t_T, t_count = np.zeros(0), np.zeros(0), np.zeros(0, np.int64)
    t_allow = np.zeros(0, np.int64)  # other live splats a target tolerates: 1, a solo splat's target none

    def alpha_of(xy, conic, opac, px, py):  # one splat at many pixels
        dx, dy = xy[0] - px, xy[1] - py
        return opac * np.exp(-(0.5 * (conic[0] * dx * dx + conic[2] * dy * dy) + conic[1] * dx * dy))

    B = 512
    img_py, img_px = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    for delta in DELTAS:
        for i in range(GRAZE_PER_DELTA):
            case = GRAZE_CASES[i % len(GRAZE_CASES)]
            for _ in range(400):
                l1 = np.exp(rng.uniform(np.log(3.0), np.log(3e4), B))
                l2 = 0.3 + np.exp(rng.uniform(np.log(1e-3), np.log(30.0), B))
                l1, l2 = np.maximum(l1, l2), np.minimum(l1, l2)
                th = rng.uniform(0, np.pi, B)
                if case == "solo":  # a border rectangle
                    side = rng.integers(0, 4, B)
                    along = rng.integers(0, nrect, B)
                    rx = np.where(side == 0, 0, np.where(side == 1, nrect - 1, along))
                    ry = np.where(side == 2, 0, np.where(side == 3, nrect - 1, along))
                else:
                    rx, ry = rng.integers(0, nrect, B), rng.integers(0, nrect, B)
                x0, y0 = rx * unit, ry * unit
                q = rng.integers(0, unit * unit, B)
                tt = rng.uniform(0.05, 1.5 if case == "solo" else 5.4, B)
                ph = rng.uniform(0, 2 * np.pi, B)
                # half of the candidates approach the target with a TIP of a long ellipse at a small sigma: where sigma
                # is flattest, a bound on sigma that is short by 1e-3 falls short by the most pixels
                lane = np.arange(B)
                tip = lane % 2 == 0
                flat = tip & (case != "solo")
                l1 = np.where(flat, np.exp(rng.uniform(np.log(1e3), np.log(3e4), B)), l1)
                tt = np.where(flat, np.exp(rng.uniform(np.log(0.05), np.log(0.3), B)), tt)
                ph = np.where(tip, np.pi * rng.integers(0, 2, B) + 0.3 * np.sqrt(l2 / l1) * rng.standard_normal(B), ph)
                conic, radius, det = conics_from_cov(l1, l2, th)
                cn = _f8(conic)
                e1, e2 = np.sqrt(2 * tt * l1) * np.cos(ph), np.sqrt(2 * tt * l2) * np.sin(ph)
                mx = x0 + ox[q] + np.cos(th) * e1 - np.sin(th) * e2
                my = y0 + oy[q] + np.sin(th) * e1 + np.cos(th) * e2
                mx, my = np.round(mx * 64) / 64, np.round(my * 64) / 64  # exact in float32, also when shifted by 4096
                dx = mx[:, None] - (x0[:, None] + ox[None, :])
                dy = my[:, None] - (y0[:, None] + oy[None, :])
                sig = 0.5 * (cn[:, 0, None] * dx * dx + cn[:, 2, None] * dy * dy) + cn[:, 1, None] * dx * dy
                k = sig.argmin(axis=1)
                rows = np.arange(B)
                smin = sig[rows, k]
                second = np.partition(sig, 1, axis=1)[:, 1]
                terms = (0.5 * (np.abs(cn[:, 0]) * dx[rows, k] ** 2 + np.abs(cn[:, 2]) * dy[rows, k] ** 2)
                         + np.abs(cn[:, 1] * dx[rows, k] * dy[rows, k]))
                in_x, in_y = (mx >= x0) & (mx <= x0 + w), (my >= y0) & (my <= y0 + w)
                ok = ((det > 0) & (cn[:, 0] > 0) & (cn[:, 2] > 0) & (cn[:, 0] * cn[:, 2] - cn[:, 1] ** 2 > 0)
                      & (smin > 0.05) & (smin < 5.4) & (second >= smin + 0.02) & (terms <= MAX_TERMS) & on_edge[k]
                      & ~(in_x & in_y))
                if case == "corner":
                    ok &= is_corner[k]
                elif case == "edge":
                    ok &= ~is_corner[k]
                elif case == "above":
                    ok &= in_x & (my < y0)
                elif case == "below":
                    ok &= in_x & (my > y0 + w)
                elif case == "left":
                    ok &= in_y & (mx < x0)
                elif case == "right":
                    ok &= in_y & (mx > x0 + w)
                elif case == "diagonal":
                    ok &= ~in_x & ~in_y
                else:
                    ok &= (mx < -1) | (mx > S) | (my < -1) | (my > S)
                chosen = None
                for j in np.nonzero(ok)[0]:
                    xy = np.array([mx[j], my[j]])
                    tpx = np.array([x0[j] + ox[k[j]], y0[j] + oy[k[j]]], dtype=np.float64)
                    opac = float(F(np.exp(smin[j]) / 255.0 * (1.0 + delta)))
                    box = tile_box(xy[None].astype(F), radius[j:j + 1], tiles, tiles)[0]
                    ttx, tty = int(tpx[0]) // 16, int(tpx[1]) // 16
                    if not (box[0] <= ttx < box[2] and box[1] <= tty < box[3]):
                        continue  # the 3-sigma box is the law: a target outside it is in no list at all
                    al = alpha_of(xy, cn[j], opac, img_px, img_py)
                    # no other rectangle is left undecided: no sub-tile's largest alpha within 1e-4 relative of 1/255
                    blockmax = al.reshape(S // 8, 8, S // 8, 8).max(axis=(1, 3)) * 255.0
                    blockmax[int(tpx[1]) // 8, int(tpx[0]) // 8] = 0.0
                    if (np.abs(blockmax - 1.0) < 1e-4).any():
                        continue
                    if unit == 8:  # the tile's other three sub-tiles: farther away
                        with np.errstate(divide="ignore"):
                            tile = -np.log(al[tty * 16:tty * 16 + 16, ttx * 16:ttx * 16 + 16] / opac)
                        tile[int(tpx[1]) % 16 // 8 * 8:int(tpx[1]) % 16 // 8 * 8 + 8,
                             int(tpx[0]) % 16 // 8 * 8:int(tpx[0]) % 16 // 8 * 8 + 8] = np.inf
                        if tile.min() <= smin[j] + 0.05:
                            continue
                    al_rest = al.copy()
                    al_rest[int(tpx[1]), int(tpx[0])] = 0.0
                    if (al_rest.max() * 255.0 > 0.9) if case == "solo" else (al_rest.max() * 255.0 < 1.01):
                        continue  # (only the solo sub-case has no live pixel in the image besides its target)
                    d = depth_pool[-1]
                    # at the targets accepted so far: clearly dead, or the only other live splat with T staying >= 0.5
                    if t_px.shape[0]:
                        at = alpha_of(xy, cn[j], opac, t_px[:, 0], t_px[:, 1]) * 255.0
                        if (np.abs(at - 1.0) < 1e-3).any():
                            continue
                        live = at >= 1.0
                        front = live & (d < t_depth)
                        newT = np.where(front, t_T * (1.0 - np.minimum(0.999, at / 255.0)), t_T)
                        if ((t_count + live > t_allow) & live).any() or (newT < 0.5).any():
                            continue
                    # the accepted splats at this target
                    cnt, T = 0, 1.0
                    if t_px.shape[0]:
                        A_xy, A_cn = np.array(acc["xy"]), _f8(np.array(acc["conic"]))
                        ddx, ddy = A_xy[:, 0] - tpx[0], A_xy[:, 1] - tpx[1]
                        am = 255.0 * np.array(acc["opac"]) * np.exp(
                            -(0.5 * (A_cn[:, 0] * ddx * ddx + A_cn[:, 2] * ddy * ddy) + A_cn[:, 1] * ddx * ddy))
                        if (np.abs(am - 1.0) < 1e-3).any() or (np.abs(t_px - tpx[None]).max(axis=1) == 0).any():
                            continue
                        cnt = int((am >= 1.0).sum())
                        infront = (am >= 1.0) & (t_depth < d)
                        T = float(np.prod(1.0 - np.minimum(0.999, am[infront] / 255.0)))
                        if cnt > (0 if case == "solo" else 1) or T < 0.5:
                            continue
                    chosen = j
                    if t_px.shape[0]:
                        t_T, t_count = newT, t_count + live
                    t_px = np.concatenate([t_px, tpx[None]])
                    t_allow = np.append(t_allow, 0 if case == "solo" else 1)
                    t_depth, t_T, t_count = np.append(t_depth, d), np.append(t_T, T), np.append(t_count, cnt)
                    depth_pool.pop()
                    for name, val in (("xy", xy), ("conic", conic[j]), ("radius", radius[j]), ("opac", opac),
                                      ("depth", d), ("target", tpx), ("smin", smin[j]), ("delta", delta),
                                      ("case", i % len(GRAZE_CASES)), ("rect", (rx[j], ry[j]))):
                        acc[name].append(val)
                    break
                if chosen is not None:
                    break
            else:
                raise AssertionError(f"graze{unit}: no placement for case {case}")
    n = len(acc["xy"])
    sc = _scene(S, S, np.array(acc["xy"]), np.array(acc["conic"]), np.array(acc["radius"]), np.array(acc["opac"]), rng,
                depths=np.array(acc["depth"]), color_lo=0.5, background=(0.1, 0.1, 0.1))
    sc.update(target=np.array(acc["target"]).astype(np.int64), smin=np.array(acc["smin"]), delta=np.array(acc["delta"]),
              case=np.array(acc["case"]), rect=np.array(acc["rect"]).astype(np.int64), unit=unit)
    assert n == len(DELTAS) * GRAZE_PER_DELTA
    # T in front of every splat at its own target: the product over the live splats in front of it
    tx, ty = sc["target"][:, 0].astype(np.float64), sc["target"][:, 1].astype(np.float64)
    c8, xy8 = _f8(sc["conics"]), _f8(sc["xys"])
    dx, dy = xy8[:, 0][:, None] - tx[None, :], xy8[:, 1][:, None] - ty[None, :]          # [splat, target]
    sig = 0.5 * (c8[:, 0, None] * dx * dx + c8[:, 2, None] * dy * dy) + c8[:, 1, None] * dx * dy
    al = _f8(sc["opacities"]) * np.exp(-sig)
    front = (al >= ALPHA_MIN) & (sc["depths"][:, None] < sc["depths"][None, :])
    sc["T_front"] = np.prod(np.where(front, 1.0 - np.minimum(0.999, al), 1.0), axis=0)
    sc["others_live"] = ((al >= ALPHA_MIN) & ~np.eye(n, dtype=bool)).sum(axis=0)
    return sc


def _needles(seed, n=72, composited=True):
    """Needles: l1 up to 3e7 px^2 over the 0.3 blur floor (also floor 0), angles at 0, pi/4, pi/2 +- 1e-4 (b -> 0 and
    |b| -> sqrt(ac)) and random, centres inside the 128 x 128 image and up to 1e4 px outside it with the box still
    reaching in, opacities 0.006 .. 1.  (72 of them in the family whose image is composited: float32 cannot decide
    the pixels along the axis of a long tilted needle, and each costs the image a few dozen unstable pixels.)"""
    rng = np.random.default_rng(seed)
    S = 128
    grid_y, grid_x = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    xy, cn, rd, op = [], [], [], []
    special = [s + d for s in (0.0, np.pi / 4, np.pi / 2, 3 * np.pi / 4) for d in (-1e-4, 0.0, 1e-4)]
    while len(xy) < n:
        i = len(xy)
        l1 = np.exp(rng.uniform(np.log(1e2), np.log(3e7)))
        l2 = (0.3 if i % 5 else 0.0) + np.exp(rng.uniform(np.log(1e-3), np.log(10.0)))
        th = special[i % len(special)] if i % 2 else rng.uniform(0, np.pi)
        conic, radius, det = conics_from_cov(l1, l2, th)
        if not (np.isfinite(conic).all() and det != 0):
            continue
        if i % 3 == 0:
            # outside, along the needle's own axis so that it still points into the image.  float32 cannot evaluate sigma
            # r px down a tilted needle (its terms grow as r^2 sin^2(2 theta) / l2 and cancel): up to 1e4 px for the
            # axis-parallel ones, as far as the terms stay near 1e3 for the others
            r = np.exp(rng.uniform(np.log(50.0), np.log(1e4)))
            r = min(r, 50.0 + 30.0 * np.sqrt(max(l2, 0.3)) / max(abs(np.sin(2 * th)), 1e-9))
            c = np.array([64.0, 64.0]) + rng.uniform(-40, 40, 2) + r * np.array([np.cos(th), np.sin(th)]) * rng.choice([-1, 1])
        else:
            c = rng.uniform(0, S, 2)
        c = np.round(c * 64) / 64
        box = tile_box(c[None].astype(F), np.array([radius]), S // 16, S // 16)[0]
        if box[2] <= box[0] or box[3] <= box[1]:
            continue
        # float32 evaluates sigma to a few 1e-7 of the sum of its terms' magnitudes, and the image to alpha x that: the
        # opacity is capped so that no pixel of the 128 x 128 image moves by more than ~3e-5 for it (composited = False:
        # the list-only scenes keep the opacity as drawn)
        o = np.exp(rng.uniform(np.log(0.006), 0.0))
        if composited:
            c8 = _f8(conic)
            dx, dy = c[0] - grid_x, c[1] - grid_y
            p0, p1, p2 = 0.5 * c8[0] * dx * dx, 0.5 * c8[2] * dy * dy, c8[1] * dx * dy
            with np.errstate(over="ignore", invalid="ignore"):
                worst = np.nanmax(np.where(p0 + p1 + p2 >= 0, np.exp(-(p0 + p1 + p2)), 0.0) * (abs(p0) + abs(p1) + abs(p2)))
            o = max(0.006, min(o, 100.0 / max(worst, 1e-9)))
        xy.append(c), cn.append(conic), rd.append(radius)
        op.append(o)
    return _scene(S, S, np.array(xy), np.array(cn), np.array(rd), np.array(op), rng)


def _tiny(seed):
    """cov = 0.3 I .. 0.5 I on and next to tile and sub-tile borders of a 40 x 24 image (partial edge tiles):
    coordinates 16k - 0.5, 16k, 16k + 7.5, 16k + 8, 16k + 15.5; opacities 1/255 exactly, its float32 neighbours,
    0.0041 and 1 (and again 0.0041, 1 and 0.3, which keeps the undecided share of the pairs below 2 %)."""
    rng = np.random.default_rng(seed)
    H, W = 24, 40
    offs = (-0.5, 0.0, 7.5, 8.0, 15.5)
    xs = [16 * k + o for k in range(3) for o in offs if -0.5 <= 16 * k + o <= W]
    ys = [16 * k + o for k in range(2) for o in offs if -0.5 <= 16 * k + o <= H]
    third = F(1.0) / F(255.0)
    opacs = [third, np.nextafter(third, F(1)), np.nextafter(third, F(0)), F(0.0041), F(1.0), F(0.0041), F(1.0), F(0.3),
             F(0.0041), F(1.0)]
    xy, var, op = [], [], []
    i = 0
    for x in xs:
        for y in ys:
            xy.append((x, y)), var.append((0.3, 0.4, 0.5)[i % 3]), op.append(opacs[(i // 3) % len(opacs)])
            i += 1
    var = np.array(var)
    conic, radius, _ = conics_from_cov(var, var, np.zeros(len(var)))
    return _scene(H, W, np.array(xy), conic, radius, np.array(op), rng)


def _norule(seed):
    """Conics that are not positive definite (a <= 0; ac - b^2 <= 0), positive definite by one float32 ulp, and a NaN
    opacity: ``make_reach`` applies no culling to the first two kinds and the last, so their lists are the box's.
    128 x 72 (the bottom tile row is partial).  ``sc['whole_box']`` marks the splats that must keep their whole box:
    every one whose a c - b^2 is not positive in exact arithmetic (whatever rounding or contraction the device uses, the
    float32 test then cannot come out positive), a <= 0 or c <= 0, or a NaN opacity."""
    rng = np.random.default_rng(seed)
    H, W = 72, 128
    xy, cn, op = [], [], []
    for i in range(36):
        kind = i % 4
        a, c = F(rng.uniform(0.01, 0.2)), F(rng.uniform(0.01, 0.2))
        root = np.sqrt(float(a) * float(c))
        if kind == 0:    # a <= 0
            a, b = F(-a if i % 8 else 0.0), F(rng.uniform(-0.05, 0.05))
        elif kind == 1:  # a c - b^2 < 0
            b = F(root * rng.uniform(1.05, 2.0) * rng.choice([-1, 1]))
        elif kind == 2:  # a c - b^2 = 0 exactly: a = c = |b|
            c = a
            b = F(a if i % 8 == 2 else -a)
        else:            # positive definite by one ulp of b: the largest float32 |b| with b^2 < a c in float64
            b = F(root)
            while float(b) * float(b) >= float(a) * float(c):
                b = np.nextafter(b, F(0))
            b = F(b if i % 8 == 3 else -b)
        xy.append(rng.uniform(4, [W - 4, H - 4])), cn.append((a, b, c)), op.append(rng.uniform(0.05, 0.6))
    # a NaN opacity on an ordinary conic, in the partial bottom-right tile
    xy.append((W - 6.0, H - 3.0)), cn.append((2.0, 0.0, 2.0)), op.append(np.nan)
    xy, cn = np.array(xy), np.array(cn, F)
    sc = _scene(H, W, xy, cn, np.array([20] * 36 + [2]), np.array(op), rng)
    a, b, c = (_f8(cn[:, i]) for i in range(3))
    sc["whole_box"] = ~((a > 0) & (c > 0) & (a * c - b * b > 0)) | np.isnan(sc["opacities"].reshape(-1))
    return sc


FAMILIES = ("graze16", "graze8", "needles", "tiny", "norule")


@functools.lru_cache(maxsize=None)
def family(name):
    """The seeded scene of one family (cached: built once per process; callers must not write into it)."""
    sc = {"graze16": lambda: _graze(16, 16), "graze8": lambda: _graze(8, 8), "needles": lambda: _needles(3),
          "tiny": lambda: _tiny(4), "norule": lambda: _norule(5)}[name]()
    for v in sc.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return sc


def needles(seed, n):
    return _needles(seed, n, composited=False)


def shifted(parts, W, H, shift):
    """The splats of several scenes moved by ``shift`` (multiples of 16 px: tile borders stay where they are) into one
    W x H image -> a scene (tile boxes recomputed for the new grid; depths distinct again)."""
    rng = np.random.default_rng(1)
    xy = np.concatenate([_f8(p["xys"]) for p in parts]) + np.asarray(shift, np.float64)
    assert np.array_equal(xy.astype(F).astype(np.float64), xy)  # centres are multiples of 1/64: the move is exact
    return _scene(H, W, xy, np.concatenate([p["conics"] for p in parts]), np.concatenate([p["radii"] for p in parts]),
                  np.concatenate([p["opacities"].reshape(-1) for p in parts]), rng)


def subset(sc, idx):
    """The splats ``idx`` of a scene as a scene of their own."""
    n = sc["xys"].shape[0]
    return {k: (v[idx] if isinstance(v, np.ndarray) and v.shape[:1] == (n,) and k != "background" else v)
            for k, v in sc.items()}


@functools.lru_cache(maxsize=None)
def truth(name):
    """What the tests of one family share: the bounding-box lists of the CPU oracle, `composite64` over them and both
    `live_pairs` -> dict(ids, bins, img, T, idx, unstable, live16, live8)."""
    from oracle import oracle as O

    sc = family(name)
    tb = grid(sc) + (1,)
    n = sc["xys"].shape[0]
    I, cum = O.compute_cumulative_intersects(sc["num_tiles_hit"])
    _, _, _, ids, bins = O.bin_and_sort_gaussians(n, I, sc["xys"], sc["depths"], sc["radii"], cum, tb, 16)
    img, T, idx, unstable = composite64(sc, ids, bins)
    return dict(ids=ids, bins=bins, img=img, T=T, idx=idx, unstable=unstable, live16=live_pairs(sc, 16),
                live8=live_pairs(sc, 8))


def target_pairs(sc, live, unit):
    """Index into ``live`` (of `live_pairs(sc, unit)`) of every graze splat's (splat, target rectangle) pair."""
    key = (live["g"] * 4096 + live["ry"]) * 4096 + live["rx"]
    want = (np.arange(sc["target"].shape[0]) * 4096 + sc["target"][:, 1] // unit) * 4096 + sc["target"][:, 0] // unit
    order = np.argsort(key)
    pos = np.searchsorted(key[order], want)
    assert (key[order][pos] == want).all()
    return order[pos]


def solo_splats(sc, tr):
    """The grazing splats (delta > 0) with exactly one live pixel in the image: their target."""
    l8 = tr["live8"]
    live_rects = np.bincount(l8["g"][l8["cls"] != DEAD], minlength=sc["xys"].shape[0])
    py, px = np.meshgrid(np.arange(sc["H"], dtype=np.float64), np.arange(sc["W"], dtype=np.float64), indexing="ij")
    out = []
    for g in np.nonzero((sc["delta"] > 0) & (live_rects == 1))[0]:
        _, alpha = _alpha_at(sc, g, px, py)
        if (alpha * 255.0 > 1.0 - 1e-3).sum() == 1:
            out.append(g)
    return np.array(out, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def large_grid_scene():
    """About 600 splats on a 3840 x 2160 grid (tile-row bands, the two-level partition): 300 needles and every other
    graze16 splat, moved by (1920, 1024) so that tile and sub-tile borders stay where they were."""
    return shifted([needles(7, 300), subset(family("graze16"), np.arange(0, 600, 2))], 3840, 2160, (1920, 1024))


@functools.lru_cache(maxsize=None)
def cotangents(name):
    """(v_img [H,W,3], v_alpha [H,W]) float32, uniform in +-[0.5, 1] with one random sign per pixel: no pixel's
    cotangent is small, the terms of one pixel's v_alpha do not cancel one another, and the sums of a splat that covers
    thousands of pixels grow as a random walk, so the floor of the gradient rule (1e-3 x the largest) stays below a
    one-pixel splat's gradient."""
    sc = family(name)
    rng = np.random.default_rng(len(name))
    sign = rng.choice([-1.0, 1.0], (sc["H"], sc["W"]))
    v_img = (sign[..., None] * rng.uniform(0.5, 1.0, (sc["H"], sc["W"], 3))).astype(F)
    v_alpha = (sign * rng.uniform(0.5, 1.0, (sc["H"], sc["W"]))).astype(F)
    return v_img, v_alpha


@functools.lru_cache(maxsize=None)
def backward64(name):
    """`oracle.rasterize_backward_fp64` over the bounding-box lists with `cotangents` -> float64 (v_xy, v_conic,
    v_colors, v_opacity)."""
    from oracle import oracle as O

    sc, tr = family(name), truth(name)
    tb = grid(sc) + (1,)
    args = (tr["ids"], tr["bins"], sc["xys"], sc["conics"], sc["colors"], sc["opacities"], sc["background"])
    _, Ts, idx = O.rasterize_forward(tb, (16, 16, 1), (sc["W"], sc["H"], 1), *args)
    v_img, v_alpha = cotangents(name)
    return O.rasterize_backward_fp64(sc["H"], sc["W"], 16, *args, Ts, idx, v_img, v_alpha)
