"""The projection of 3-D Gaussians in float64: forward (numpy), the rows a 1-ulp difference may legitimately flip, and
the VJP (torch autograd).  Plain restatements of the rules of the reference's CUDA source (forward.cu:13-90,398-464,
backward.cu:305-453, helpers.cuh:7-219 -- the lines csrc/project.hip's header cites), not of project.hip or of
oracle/gsr_oracle.c: the tests hold both of those to this file.

The rules, as the CUDA source states them:
  * near plane: a Gaussian is culled when z_view <= clip_thresh (helpers.cuh:212-219; `<=`, not `<`);
  * cov3d = M M^T, M = R(q / |q|) diag(glob_scale * s) -- any quaternion norm;
  * EWA: the centre is clamped to 1.3x the frustum IN THE FORWARD ONLY (tx/tz to +-1.3 * 0.5 W / fx, ty/tz likewise
    with H and fy) before the Jacobian is formed; 0.3 is added to the diagonal of cov2d;
    compensation = sqrt(max(0, det(cov2d) / det(cov2d + 0.3 I)));
  * conic = inverse(cov2d + 0.3 I), culled when that determinant is 0;
    radius = ceil(3 sqrt(max eigenvalue)), the discriminant floored at 0.1;
  * xy = 0.5 * size * (P p)_{x,y} / ((P p)_w + 1e-6) + c - 0.5;
  * tile box: min = clamp(trunc((u - r) / bw), 0, tiles), max = clamp(trunc((u + r) / bw + 1), 0, tiles), culled when
    its area is 0;
  * every output of a culled Gaussian is zero;
  * backward: NO fov clamp (so only Gaussians inside the guard band are comparable with the forward's derivative); the
    quaternion is differentiated as the unit quaternion q / |q| (no projection onto the tangent space); the
    compensation's cotangent is scaled by 0.5 / (compensation + 1e-6) with the compensation that was handed in.

Scalars (focal lengths, principal point, glob_scale, clip_thresh) are rounded to float32 first: that is what the
C ABI hands the kernel, and `tz == clip` has to mean the same number on both sides."""
import numpy as np
import torch

AMBIG_EPS = 1e-5  # relative distance from a discrete boundary inside which fp32 may decide either way
OUTPUTS = ("cov3d", "xys", "depths", "conics", "compensation")  # the float outputs (radii, num_tiles_hit: integers)


def _f32(v):
    return float(np.float32(v))


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _near_integer(v, eps, lo, hi):
    """|v - k| <= eps * max(1, |v|) for an integer k in [lo, hi] (a boundary that can change a clamped truncation)."""
    k = np.rint(v)
    return (np.abs(v - k) <= eps * np.maximum(1.0, np.abs(v))) & (k >= lo) & (k <= hi)


def project_forward_fp64(means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy, img_height, img_width,
                         block_width, clip_thresh, cov3d=None, eps=AMBIG_EPS):
    """-> dict of float64 / integer numpy arrays: cov3d [n,6], xys [n,2], depths, radius (before ceil), radii,
    conics [n,3], compensation, tile_min / tile_max [n,2], num_tiles_hit, visible (radii > 0), clamped (the 1.3x clamp
    active), ambiguous (within `eps` relative of a discrete boundary, decided in float64 alone), `why`, the
    boundaries apart, and box_lo / box_hi [n,2], the tile box before truncation.  `cov3d` [n,6] (upper triangle) in place of `scales` / `quats` (both None): handed in."""
    fx, fy, cx, cy, g, clip = (_f32(v) for v in (fx, fy, cx, cy, glob_scale, clip_thresh))
    H, W, bw = int(img_height), int(img_width), int(block_width)
    p = _d(means3d)
    n = len(p)
    vm = _d(viewmat).reshape(-1, 4)[:3]
    pm = _d(projmat).reshape(4, 4)
    t = p @ vm[:, :3].T + vm[:, 3]
    tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
    front = tz > clip
    tzs = np.where(front, tz, 1.0)  # (culled rows: any finite stand-in, their outputs are zeroed below)

    if cov3d is None:
        q = _d(quats)
        q = q / np.linalg.norm(q, axis=1, keepdims=True)
        w, x, y, z = q.T
        R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                      np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                      np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)
        M = R * (g * _d(scales))[:, None, :]
        S = M @ M.transpose(0, 2, 1)
    else:
        assert scales is None and quats is None
        c = _d(cov3d)
        S = np.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], -2)

    limx, limy = 1.3 * (0.5 * W / fx), 1.3 * (0.5 * H / fy)
    rx, ry = tx / tzs, ty / tzs
    ex, ey = tzs * np.clip(rx, -limx, limx), tzs * np.clip(ry, -limy, limy)
    zero = np.zeros(n)
    J = np.stack([np.stack([fx / tzs, zero, -fx * ex / tzs ** 2], -1),
                  np.stack([zero, fy / tzs, -fy * ey / tzs ** 2], -1)], -2)
    T = J @ vm[:, :3]
    C2 = T @ S @ T.transpose(0, 2, 1)
    det_orig = C2[:, 0, 0] * C2[:, 1, 1] - C2[:, 0, 1] ** 2
    a, b, c_ = C2[:, 0, 0] + 0.3, C2[:, 0, 1], C2[:, 1, 1] + 0.3
    det = a * c_ - b * b
    valid = det != 0
    dets = np.where(valid, det, 1.0)
    comp = np.sqrt(np.maximum(0.0, det_orig / dets))
    conics = np.stack([c_ / dets, -b / dets, a / dets], -1)
    mid = 0.5 * (a + c_)
    disc = np.sqrt(np.maximum(0.1, mid * mid - det))
    radius = 3.0 * np.sqrt(np.maximum(mid + disc, mid - disc))
    rad = np.ceil(radius)

    h = p @ pm[:, :3].T + pm[:, 3]
    rw = 1.0 / (h[:, 3] + 1e-6)
    xy = np.stack([0.5 * W * (h[:, 0] * rw) + cx - 0.5, 0.5 * H * (h[:, 1] * rw) + cy - 0.5], -1)
    tiles = np.array([(W + bw - 1) // bw, (H + bw - 1) // bw])
    lo_f, hi_f = (xy - rad[:, None]) / bw, (xy + rad[:, None]) / bw
    tmin = np.clip(np.trunc(np.clip(lo_f, -2.0, 1e9)), 0, tiles).astype(np.int64)
    tmax = np.clip(np.trunc(np.clip(hi_f + 1.0, -2.0, 1e9)), 0, tiles).astype(np.int64)
    area = (tmax - tmin).prod(axis=1)
    visible = front & valid & (area > 0)

    # ---- rows a 1-ulp difference may flip: float64 alone decides
    rel = lambda v, ref: np.abs(v - ref) <= eps * np.maximum(np.abs(v), abs(ref))  # noqa: E731
    alive = front & valid
    why = {
        "near_plane": rel(tz, clip),
        "guard_band": alive & (rel(np.abs(rx), limx) | rel(np.abs(ry), limy)),
        "radius": alive & (np.abs(radius - np.rint(radius)) <= eps * radius),
        "tile_edge": alive & (_near_integer(lo_f, eps, 0, tiles).any(axis=1)
                              | _near_integer(hi_f, eps, 0, tiles).any(axis=1)),
        # the edges on which the box's area passes through zero: (u + r) / bw at 0, (u - r) / bw at the last tile
        "zero_area": alive & (_near_integer(hi_f, eps, 0, 0).any(axis=1)
                              | _near_integer(lo_f, eps, tiles, tiles).any(axis=1)),
    }
    ambiguous = np.zeros(n, bool)
    for m in why.values():
        ambiguous |= m

    def z(a_):
        keep = visible.reshape((n,) + (1,) * (a_.ndim - 1))
        return np.where(keep, a_, 0)

    cov6 = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], -1)
    return dict(cov3d=z(cov6), xys=z(xy), depths=z(tz), radius=z(radius), radii=z(rad).astype(np.int64),
                conics=z(conics), compensation=z(comp), tile_min=z(tmin), tile_max=z(tmax),
                num_tiles_hit=z(area), visible=visible,
                clamped=alive & ((np.abs(rx) > limx) | (np.abs(ry) > limy)), ambiguous=ambiguous, why=why,
                box_lo=lo_f, box_hi=hi_f)  # ((u, v) -+ r) / bw of EVERY row, culled ones too


def forward_condition_fp64(means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy, img_height, img_width):
    """-> {output: [n]}: by how much an fp32 evaluation's rounding (one part in 2^24 per operation) is amplified in a
    row of that output, relative to the row's largest magnitude -- the sum of the magnitudes of the terms of each
    sum over the magnitude of its result (depths, xys), and the same for the two determinants whose cancellation
    decides conics and compensation.  Float64 alone; it tells where an fp32 implementation is furthest from float64
    (the golden generator stores the reference's answer on the worst rows of every case, besides an even sample)."""
    fx, fy, cx, cy, g = (_f32(v) for v in (fx, fy, cx, cy, glob_scale))
    p = _d(means3d)
    vm, pm = _d(viewmat).reshape(-1, 4)[:3], _d(projmat).reshape(4, 4)
    hom = np.concatenate([p, np.ones((len(p), 1))], 1)
    tz = hom @ vm[2]
    depth = (np.abs(hom) @ np.abs(vm[2])) / np.abs(tz)
    h, habs = hom @ pm.T, np.abs(hom) @ np.abs(pm).T
    rw = 1.0 / np.abs(h[:, 3] + 1e-6)
    size, c = np.array([img_width, img_height], float), np.array([cx, cy])
    xy = 0.5 * size * h[:, :2] / (h[:, 3:] + 1e-6) + c - 0.5
    xys = ((0.5 * size * habs[:, :2] * rw[:, None] * (1.0 + habs[:, 3:] * rw[:, None]) + c + 0.5)
           / np.abs(xy).max(axis=1, keepdims=True)).max(axis=1)
    f = project_forward_fp64(means3d, scales, g, quats, viewmat, projmat, fx, fy, cx, cy, img_height, img_width, 16,
                             -np.inf)
    k0, k1, k2 = f["conics"].T  # cov2d + 0.3 I = inverse(conic)
    det_k = k0 * k2 - k1 * k1
    with np.errstate(all="ignore"):
        a, b, c_ = k2 / det_k, -k1 / det_k, k0 / det_k
        conics = (a * c_ + b * b) / (a * c_ - b * b)
        a0, c0 = a - 0.3, c_ - 0.3
        compensation = (a0 * c0 + b * b) / np.abs(a0 * c0 - b * b)
    return dict(depths=depth, xys=xys, conics=conics, compensation=compensation)


def cov2d_bounds_fp64(cov2d, eps=AMBIG_EPS):
    """-> (conics [n,3], radius before ceil, radii, valid, ambiguous) for cov2d rows (a, b, c) (helpers.cuh:36-59)."""
    a, b, c = _d(cov2d).T
    det = a * c - b * b
    valid = det != 0
    dets = np.where(valid, det, 1.0)
    conics = np.where(valid[:, None], np.stack([c / dets, -b / dets, a / dets], -1), 0.0)
    mid = 0.5 * (a + c)
    disc = np.sqrt(np.maximum(0.1, mid * mid - det))
    radius = np.where(valid, 3.0 * np.sqrt(np.maximum(mid + disc, mid - disc)), 0.0)
    ambiguous = valid & (np.abs(radius - np.rint(radius)) <= eps * radius)
    return conics, radius, np.ceil(radius), valid, ambiguous


def _unit_rotation(q):
    w, x, y, z = q.unbind(-1)
    return torch.stack([
        torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
        torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
        torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def project_vjp_fp64(means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy, img_height, img_width,
                     compensation, v_xy, v_depth, v_conic, v_compensation, cov3d=None):
    """-> (v_mean3d, v_scale, v_quat, guard) float64 numpy; `guard`: the Gaussians inside the 1.3x guard band (the
    forward's fov clamp inactive, so the unclamped backward is the forward's derivative there).  A cotangent that is
    None is a zero cotangent.  With `cov3d` [n,6] (and `scales` = `quats` = None) the covariances were handed in and the
    chain ends there: -> (v_mean3d, v_cov3d, guard), v_cov3d per upper-triangle entry (an off-diagonal entry stands
    for both of its places in the matrix)."""
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    fx, fy, cx, cy, glob_scale = (_f32(v) for v in (fx, fy, cx, cy, glob_scale))
    m = d(means3d).requires_grad_(True)
    n = m.shape[0]
    vm, pm = d(viewmat).reshape(-1, 4)[:3], d(projmat).reshape(4, 4)
    if cov3d is None:
        s = d(scales).requires_grad_(True)
        q = d(quats)
        qn = (q / q.norm(dim=-1, keepdim=True)).detach().requires_grad_(True)
        M = _unit_rotation(qn) * (glob_scale * s)[:, None, :]
        V = M @ M.transpose(1, 2)
        leaves = (m, s, qn)
    else:
        assert scales is None and quats is None
        c6 = d(cov3d).requires_grad_(True)
        V = torch.stack([c6[:, [0, 1, 2]], c6[:, [1, 3, 4]], c6[:, [2, 4, 5]]], -2)
        leaves = (m, c6)
    Wr = vm[:, :3]
    t = m @ Wr.T + vm[:, 3]
    tx, ty, tz = t.unbind(-1)
    zero = torch.zeros_like(tz)
    J = torch.stack([torch.stack([fx / tz, zero, -fx * tx / tz ** 2], -1),
                     torch.stack([zero, fy / tz, -fy * ty / tz ** 2], -1)], -2)
    T = J @ Wr
    Cv = T @ V @ T.transpose(1, 2)
    a, b, c = Cv[:, 0, 0] + 0.3, Cv[:, 0, 1], Cv[:, 1, 1] + 0.3
    det = a * c - b * b
    conic = torch.stack([c / det, -b / det, a / det], -1)
    comp_sq = (Cv[:, 0, 0] * Cv[:, 1, 1] - Cv[:, 0, 1] ** 2) / det  # compensation^2
    h = m @ pm[:, :3].T + pm[:, 3]
    rw = 1.0 / (h[:, 3] + 1e-6)
    xy = torch.stack([0.5 * img_width * h[:, 0] * rw + cx - 0.5, 0.5 * img_height * h[:, 1] * rw + cy - 0.5], -1)
    loss = (m * 0.0).sum()  # (all cotangents None: zero gradients)
    if v_xy is not None:
        loss = loss + (xy * d(v_xy)).sum()
    if v_depth is not None:
        loss = loss + (tz * d(v_depth)).sum()
    if v_conic is not None:
        loss = loss + (conic * d(v_conic)).sum()
    if v_compensation is not None:
        vcomp = d(v_compensation) * 0.5 / (d(compensation) + 1e-6)  # d comp = d(comp^2) / (2 (comp + 1e-6))
        loss = loss + (comp_sq * vcomp).sum()
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grads = [torch.zeros_like(x) if g is None else g for g, x in zip(grads, leaves)]
    with torch.no_grad():
        limx, limy = 1.3 * 0.5 * img_width / fx, 1.3 * 0.5 * img_height / fy
        guard = ((tx / tz).abs() < limx) & ((ty / tz).abs() < limy)
    assert len(guard) == n
    return tuple(g.numpy() for g in grads) + (guard.numpy(),)


def row_err(mine, ref):
    """Per row: max |mine - ref| over the row's components."""
    return np.abs(np.asarray(mine, np.float64) - ref).reshape(len(ref), -1).max(axis=1)


def row_max(ref):
    return np.abs(ref).reshape(len(ref), -1).max(axis=1)
