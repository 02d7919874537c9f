"""The projection of 3-D Gaussians through an equidistant fisheye camera in float64: forward (numpy), the rows a 1-ulp
difference may legitimately flip, and the VJP (torch autograd).  It follows tests/projection_reference.py and reuses
its pieces; the rule is the one csrc/project.hip's header and DESIGN.md section 4.23 state, written down here on its
own (gsplat's camera_model="fisheye" with an ideal lens):

  * near plane: culled when tz <= clip (`<=`), which keeps the polar angle below 90 degrees;
  * centre: r = sqrt(tx^2 + ty^2), theta = atan2(r, tz), s = theta / r (1 / tz at r = 0),
    xy = (fx s tx + cx - 0.5, fy s ty + cy - 0.5); the projection matrix is not read;
  * J = d(xy)/dt = [fx (s + tx^2 c), fx tx ty c, -fx tx / d^2; fy tx ty c, fy (s + ty^2 c), -fy ty / d^2] with
    d^2 = r^2 + tz^2 and c = (tz / d^2 - s) / r^2 -- the textbook closed form with a = tz / (d^2 r^2), b = theta / r^3
    regrouped (tx^2 a + ty^2 b = s + tx^2 c, a - b = c); no clamp of the centre, forward or backward;
  * cov2d = J W S W^T J^T, + 0.3 on the diagonal, compensation, conic, radius and tile box as the pinhole reference;
  * depths = tz; every output of a culled Gaussian is zero.

At and next to the axis the closed forms are 0/0 and cancel: below q = r^2 / tz^2 < REF_SERIES_Q this file takes the
power series of s and c in q (REF_SERIES_TERMS terms: the first dropped term is q^8 / 17 < 1e-33 there), above it
`atan2` directly.  The switch point is not the kernel's (1/32, six terms): the two agree only where both are right.
The same code runs in numpy.float32 (`dtype=`): the reference's own rounding error, the yardstick of the GPU tests.

Scalars (focal lengths, principal point, glob_scale, clip_thresh) are rounded to float32 first, as the C ABI does."""
import numpy as np
import torch

from projection_reference import AMBIG_EPS, OUTPUTS, _f32, _near_integer, _unit_rotation, row_err, row_max  # noqa: F401

REF_SERIES_Q = 1e-4
REF_SERIES_TERMS = 8


def _series(q, first, coef):
    """sum_{k >= first} coef(k) (-q)^(k - first) sign-adjusted: Horner over REF_SERIES_TERMS terms, in q's dtype."""
    ks = range(first + REF_SERIES_TERMS - 1, first - 1, -1)
    acc = None
    for k in ks:
        ck = ((-1.0) ** k) * coef(k)
        acc = ck if acc is None else ck + q * acc
    return acc


def _s_c_numpy(tx, ty, tz):
    """-> (s, c, w = 1 / d^2) in the dtype of the inputs; finite for every tz > 0, r = 0 and underflowing r^2 included."""
    r2 = tx * tx + ty * ty
    z2 = tz * tz
    q = r2 / z2
    small = q < REF_SERIES_Q
    qs = np.where(small, q, 0)  # (the series only where it is taken: q^7 of a row at the edge may overflow float32)
    s_ser = _series(qs, 0, lambda k: 1.0 / (2 * k + 1)) / tz
    c_ser = _series(qs, 1, lambda k: 2.0 * k / (2 * k + 1)) / (tz * z2)
    r2s = np.where(small, 1, r2).astype(r2.dtype)
    r = np.sqrt(r2s)
    w = 1 / (r2 + z2)
    s_cl = np.arctan2(r, tz) / r
    c_cl = (tz * w - s_cl) / r2s
    return (np.where(small, s_ser, s_cl).astype(r2.dtype), np.where(small, c_ser, c_cl).astype(r2.dtype), w)


def project_forward_fisheye_fp64(means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy, img_height,
                                 img_width, block_width, clip_thresh, cov3d=None, eps=AMBIG_EPS, dtype=np.float64):
    """-> the dictionary of projection_reference.project_forward_fp64 (cov3d, xys, depths, radius, radii, conics,
    compensation, tile_min, tile_max, num_tiles_hit, visible, clamped -- never --, ambiguous, why, box_lo, box_hi).
    `projmat` is accepted and not read.  `dtype=numpy.float32`: every operation in float32 (the flags are then that
    evaluation's own and of no use: take them from the float64 call)."""
    dt = np.dtype(dtype).type
    a_ = lambda v: np.ascontiguousarray(v, dtype=dtype)  # noqa: E731
    fx, fy, cx, cy, g, clip = (dt(_f32(v)) for v in (fx, fy, cx, cy, glob_scale, clip_thresh))
    H, W, bw = int(img_height), int(img_width), int(block_width)
    p = a_(means3d)
    n = len(p)
    vm = a_(viewmat).reshape(-1, 4)[:3]
    t = p @ vm[:, :3].T + vm[:, 3]
    tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
    front = tz > clip
    tzs = np.where(front, tz, dt(1.0))  # (culled rows: any finite stand-in, their outputs are zeroed below)

    if cov3d is None:
        q = a_(quats)
        q = q / np.linalg.norm(q, axis=1, keepdims=True)
        w, x, y, z = q.T
        R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                      np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                      np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)
        M = R * (g * a_(scales))[:, None, :]
        S = M @ M.transpose(0, 2, 1)
    else:
        assert scales is None and quats is None
        c = a_(cov3d)
        S = np.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], -2)

    with np.errstate(all="ignore"):
        s, cc, wd = _s_c_numpy(tx, ty, tzs)
    xyc = tx * ty * cc
    J = np.stack([np.stack([fx * (s + tx * tx * cc), fx * xyc, -fx * tx * wd], -1),
                  np.stack([fy * xyc, fy * (s + ty * ty * cc), -fy * ty * wd], -1)], -2)
    T = J @ vm[:, :3]
    C2 = T @ S @ T.transpose(0, 2, 1)
    det_orig = C2[:, 0, 0] * C2[:, 1, 1] - C2[:, 0, 1] ** 2
    a, b, c_ = C2[:, 0, 0] + dt(0.3), C2[:, 0, 1], C2[:, 1, 1] + dt(0.3)
    det = a * c_ - b * b
    valid = det != 0
    dets = np.where(valid, det, dt(1.0))
    comp = np.sqrt(np.maximum(dt(0.0), det_orig / dets))
    conics = np.stack([c_ / dets, -b / dets, a / dets], -1)
    mid = dt(0.5) * (a + c_)
    disc = np.sqrt(np.maximum(dt(0.1), mid * mid - det))
    radius = dt(3.0) * np.sqrt(np.maximum(mid + disc, mid - disc))
    rad = np.ceil(radius)

    xy = np.stack([fx * s * tx + cx - dt(0.5), fy * s * ty + cy - dt(0.5)], -1)
    tiles = np.array([(W + bw - 1) // bw, (H + bw - 1) // bw])
    lo_f, hi_f = (xy - rad[:, None]) / dt(bw), (xy + rad[:, None]) / dt(bw)
    tmin = np.clip(np.trunc(np.clip(lo_f, -2.0, 1e9)), 0, tiles).astype(np.int64)
    tmax = np.clip(np.trunc(np.clip(hi_f + dt(1.0), -2.0, 1e9)), 0, tiles).astype(np.int64)
    area = (tmax - tmin).prod(axis=1)
    visible = front & valid & (area > 0)

    rel = lambda v, ref: np.abs(v - ref) <= eps * np.maximum(np.abs(v), abs(ref))  # noqa: E731
    alive = front & valid
    why = {
        "near_plane": rel(tz, clip),
        "radius": alive & (np.abs(radius - np.rint(radius)) <= eps * radius),
        "tile_edge": alive & (_near_integer(lo_f, eps, 0, tiles).any(axis=1)
                              | _near_integer(hi_f, eps, 0, tiles).any(axis=1)),
        "zero_area": alive & (_near_integer(hi_f, eps, 0, 0).any(axis=1)
                              | _near_integer(lo_f, eps, tiles, tiles).any(axis=1)),
    }
    ambiguous = np.zeros(n, bool)
    for m in why.values():
        ambiguous |= m

    def z(v):
        keep = visible.reshape((n,) + (1,) * (v.ndim - 1))
        return np.where(keep, v, 0)

    cov6 = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], -1)
    return dict(cov3d=z(cov6), xys=z(xy), depths=z(tz), radius=z(radius), radii=z(rad).astype(np.int64),
                conics=z(conics), compensation=z(comp), tile_min=z(tmin), tile_max=z(tmax),
                num_tiles_hit=z(area), visible=visible, clamped=np.zeros(n, bool), ambiguous=ambiguous, why=why,
                box_lo=lo_f, box_hi=hi_f, jacobian=J)


def _s_c_torch(tx, ty, tz):
    r2 = tx * tx + ty * ty
    z2 = tz * tz
    q = r2 / z2
    small = q < REF_SERIES_Q
    qs = torch.where(small, q, torch.zeros_like(q))
    s_ser = _series(qs, 0, lambda k: 1.0 / (2 * k + 1)) / tz
    c_ser = _series(qs, 1, lambda k: 2.0 * k / (2 * k + 1)) / (tz * z2)
    r2s = torch.where(small, torch.ones_like(r2), r2)  # (rows at and next to the axis stay out of autograd's 0/0)
    r = torch.sqrt(r2s)
    w = 1 / (r2 + z2)
    s_cl = torch.atan2(r, tz) / r
    c_cl = (tz * w - s_cl) / r2s
    return torch.where(small, s_ser, s_cl), torch.where(small, c_ser, c_cl), w


def project_vjp_fisheye_fp64(means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy, img_height,
                             img_width, compensation, v_xy, v_depth, v_conic, v_compensation, clip_thresh=0.01,
                             cov3d=None):
    """-> (v_mean3d, v_scale, v_quat) float64 numpy, or with `cov3d` [n,6] (and `scales` = `quats` = None)
    (v_mean3d, v_cov3d): torch float64 autograd through the rule above -- the same function forward and backward,
    no clamp.  Conventions as projection_reference.project_vjp_fp64: a cotangent that is None is zero, the quaternion
    is differentiated as the unit quaternion, the compensation's cotangent is scaled by 0.5 / (compensation + 1e-6)
    with the compensation handed in.  Rows with tz <= clip get zeros."""
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    fx, fy, cx, cy, glob_scale, clip = (_f32(v) for v in (fx, fy, cx, cy, glob_scale, clip_thresh))
    m = d(means3d).requires_grad_(True)
    vm = d(viewmat).reshape(-1, 4)[:3]
    if cov3d is None:
        s_ = d(scales).requires_grad_(True)
        q = d(quats)
        qn = (q / q.norm(dim=-1, keepdim=True)).detach().requires_grad_(True)
        M = _unit_rotation(qn) * (glob_scale * s_)[:, None, :]
        V = M @ M.transpose(1, 2)
        leaves = (m, s_, qn)
    else:
        assert scales is None and quats is None
        c6 = d(cov3d).requires_grad_(True)
        V = torch.stack([c6[:, [0, 1, 2]], c6[:, [1, 3, 4]], c6[:, [2, 4, 5]]], -2)
        leaves = (m, c6)
    Wr = vm[:, :3]
    t = m @ Wr.T + vm[:, 3]
    tx, ty, tz = t.unbind(-1)
    front = tz.detach() > clip
    tzs = torch.where(front, tz, torch.ones_like(tz))
    s, c, w = _s_c_torch(tx, ty, tzs)
    xyc = tx * ty * c
    J = torch.stack([torch.stack([fx * (s + tx * tx * c), fx * xyc, -fx * tx * w], -1),
                     torch.stack([fy * xyc, fy * (s + ty * ty * c), -fy * ty * w], -1)], -2)
    T = J @ Wr
    Cv = T @ V @ T.transpose(1, 2)
    a, b, c_ = Cv[:, 0, 0] + 0.3, Cv[:, 0, 1], Cv[:, 1, 1] + 0.3
    det = a * c_ - b * b
    conic = torch.stack([c_ / det, -b / det, a / det], -1)
    comp_sq = (Cv[:, 0, 0] * Cv[:, 1, 1] - Cv[:, 0, 1] ** 2) / det
    xy = torch.stack([fx * s * tx + cx - 0.5, fy * s * ty + cy - 0.5], -1)
    keep = front.to(torch.float64)
    loss = (m * 0.0).sum()
    if v_xy is not None:
        loss = loss + (xy * d(v_xy) * keep[:, None]).sum()
    if v_depth is not None:
        loss = loss + (tz * d(v_depth) * keep).sum()
    if v_conic is not None:
        loss = loss + (conic * d(v_conic) * keep[:, None]).sum()
    if v_compensation is not None:
        vcomp = d(v_compensation) * 0.5 / (d(compensation) + 1e-6)
        loss = loss + (comp_sq * vcomp * keep).sum()
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grads = [torch.zeros_like(x) if g_ is None else g_ for g_, x in zip(grads, leaves)]
    return tuple(g_.numpy() for g_ in grads)


def centre_jacobian_autograd_fp64(t, fx, fy):
    """d(xy)/dt [n,2,3] of the centre rule by float64 autograd, `atan2` directly (rows with r > 0 only): what the
    closed form of J is checked against."""
    t = torch.from_numpy(np.ascontiguousarray(t, np.float64)).requires_grad_(True)
    r = torch.sqrt(t[:, 0] ** 2 + t[:, 1] ** 2)
    s = torch.atan2(r, t[:, 2]) / r
    xy = torch.stack([fx * s * t[:, 0], fy * s * t[:, 1]], -1)
    rows = [torch.autograd.grad(xy[:, k].sum(), t, retain_graph=True)[0] for k in range(2)]
    return torch.stack(rows, 1).numpy()
