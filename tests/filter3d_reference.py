"""Restatements of the 3D smoothing filter (include/gsraster.h, gsr_filter3d_sampling / gsr_activate_filtered_*; DESIGN.md
section 4.22) and the case builders of tests/test_filter3d_host.py and tests/test_gpu_filter3d.py.

`sampling` is the sampling rule in NumPy, operation for operation in the order the header writes it; with float32 it
is what the kernel must produce bit for bit, with float64 the evaluation it is checked against on the host.
`activation` is the filtered activation and its gradients in the operation order of the kernel, in float64 (the
reference) or float32 (the twin that scales the error bound).
"""
from types import SimpleNamespace

import numpy as np

F32, F64 = np.float32, np.float64
VARIANCE, NEAR, MARGIN = 0.2, 0.2, 0.15
STRIDE = 20


def filter_constant(variance=VARIANCE):
    """k = float32(sqrt(variance))."""
    return F32(np.sqrt(F64(variance)))


def camera_table(cams) -> np.ndarray:
    """float32 [V,20]: what gs_fused.filter_cameras builds."""
    table = np.zeros((len(cams), STRIDE), F32)
    for v, c in enumerate(cams):
        table[v, :12] = np.asarray(c.viewmat, F32)[:3, :].reshape(12)
        table[v, 12:18] = [c.fx, c.fy, c.cx, c.cy, c.width, c.height]
    return table


def sampling(means, table, variance=VARIANCE, near=NEAR, margin=MARGIN, dtype=F32, seen_override=None):
    """-> dict(filter [N], nu [N], seen [N,V], z, u, w [N,V]) in `dtype`, every operation rounded on its own in the
    order of the rule.  `seen_override` (bool [N,V]): decisions taken from elsewhere, the values still from here."""
    t = dtype
    means, table = np.asarray(means).astype(t), np.asarray(table).astype(t)
    k = t(filter_constant(variance))
    near, margin = t(near), t(margin)
    n, nv = means.shape[0], table.shape[0]
    X, Y, Z = means[:, 0], means[:, 1], means[:, 2]
    nu = np.zeros(n, t)
    seen_all, zs, us, ws = (np.zeros((n, nv), dt) for dt in (bool, t, t, t))
    with np.errstate(all="ignore"):
        for v in range(nv):  # cameras in index order
            c = table[v]
            x = ((c[0] * X + c[1] * Y) + c[2] * Z) + c[3]
            y = ((c[4] * X + c[5] * Y) + c[6] * Z) + c[7]
            z = ((c[8] * X + c[9] * Y) + c[10] * Z) + c[11]
            fx, fy, cx, cy, W, H = c[12:18]
            u = (x / z) * fx + cx
            w = (y / z) * fy + cy
            mw, mh = margin * W, margin * H
            seen = (z > near) & (u >= -mw) & (u <= W + mw) & (w >= -mh) & (w <= H + mh)  # NaN: False
            if seen_override is not None:
                seen = seen_override[:, v]
            rate = fx / z
            nu = np.where(seen & (rate > nu), rate, nu).astype(t)
            seen_all[:, v], zs[:, v], us[:, v], ws[:, v] = seen, z, u, w
        positive = nu > 0
        if positive.any():
            filt = (k / np.where(positive, nu, nu[positive].min())).astype(t)
        else:
            filt = np.zeros(n, t)
    return {"filter": filt, "nu": nu, "seen": seen_all, "z": zs, "u": us, "w": ws}


def robust_pairs(ref64, table, near=NEAR, margin=MARGIN, rel=1e-4):
    """bool [N,V]: the pairs of a float64 evaluation whose decision does not hang on rounding -- z - near, and (where
    z is clear of near on the seen side) u and w against their two thresholds, further than `rel` of their scale away.
    A NaN centre is unseen in any arithmetic: robust."""
    z, u, w = ref64["z"], ref64["u"], ref64["w"]
    W, H = table[None, :, 16].astype(F64), table[None, :, 17].astype(F64)
    with np.errstate(all="ignore"):
        z_clear = np.abs(z - near) > rel * np.maximum(np.abs(z), near)
        u_clear = np.minimum(np.abs(u + margin * W), np.abs(u - (W + margin * W))) > rel * np.maximum(np.abs(u), W)
        w_clear = np.minimum(np.abs(w + margin * H), np.abs(w - (H + margin * H))) > rel * np.maximum(np.abs(w), H)
    return np.isnan(z) | (z_clear & ((z <= near) | (u_clear & w_clear)))


# ---- cases of the sampling pass ---------------------------------------------------------------------------------
def make_cameras(nv: int, seed: int):
    """`nv` cameras around the origin that differ in pose, focal length, image size and principal point."""
    from harness import scene as S

    rng = np.random.default_rng(1000 + seed)
    cams = []
    for v in range(nv):
        W, H = int(rng.integers(200, 640)), int(rng.integers(160, 480))
        base = S.make_camera(W, H, fov_x_deg=float(rng.uniform(40, 75)), yaw=float(rng.uniform(-0.25, 0.25)),
                             pitch=float(rng.uniform(-0.15, 0.15)), roll=float(rng.uniform(-0.1, 0.1)),
                             trans=tuple(rng.uniform(-0.3, 0.3, 3)))
        cams.append(SimpleNamespace(width=W, height=H, fx=float(base.fx * rng.uniform(0.9, 1.1)),
                                    fy=float(base.fy * rng.uniform(0.9, 1.1)),
                                    cx=float(W / 2 + rng.uniform(-12, 12)), cy=float(H / 2 + rng.uniform(-9, 9)),
                                    viewmat=np.asarray(base.viewmat, F32)))
    return cams


def _to_world(cam, p_cam):
    R, t = cam.viewmat[:3, :3].astype(F64), cam.viewmat[:3, 3].astype(F64)
    return (np.asarray(p_cam, F64) - t) @ R  # R^T (p - t)


def sampling_case(n: int, nv: int, seed: int = 0):
    """-> (means float32 [n,3], cameras).  From n >= 63 on the first six rows are, with respect to camera 0: behind it;
    in front but not beyond `near`; outside the image inside the margin band; outside the band; far off every camera's
    axis (seen by none: the fallback); a NaN centre.  The rest fill camera 0's frustum and its surroundings."""
    cams = make_cameras(nv, seed)
    rng = np.random.default_rng(seed)
    c0 = cams[0]
    z = rng.uniform(0.5, 8.0, n)
    u = rng.uniform(-0.3 * c0.width, 1.3 * c0.width, n)
    w = rng.uniform(-0.3 * c0.height, 1.3 * c0.height, n)
    z[rng.random(n) < 0.1] *= -1.0
    p = np.stack([(u - c0.cx) / c0.fx * z, (w - c0.cy) / c0.fy * z, z], axis=1)
    if n >= 63:
        at = lambda uu, ww, zz: [(uu - c0.cx) / c0.fx * zz, (ww - c0.cy) / c0.fy * zz, zz]  # noqa: E731
        p[0] = at(0.5 * c0.width, 0.5 * c0.height, -2.0)
        p[1] = at(0.5 * c0.width, 0.5 * c0.height, 0.5 * NEAR)
        p[2] = at(1.07 * c0.width, 0.5 * c0.height, 3.0)
        p[3] = at(0.5 * c0.width, -0.4 * c0.height, 3.0)
        p[4] = [2000.0, 0.0, 1.0]
    means = _to_world(c0, p).astype(F32)
    if n >= 63:
        means[5] = np.nan
    return means, cams


def unseen_case(n: int, nv: int, seed: int = 0):
    """A scene behind every camera."""
    cams = make_cameras(nv, seed)
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-60.0, -50.0, n)], axis=1)
    return _to_world(cams[0], p).astype(F32), cams


# ---- the filtered activation ------------------------------------------------------------------------------------
def activation(log_scales, raw_quats, logits, filt, v_scales=None, v_quats=None, v_opac=None, dtype=F64):
    """The filtered activations and their VJP in `dtype`, in the kernel's operation order (csrc/filter3d.hip).
    -> dict(scales, quats, opacities, v_log_scales, v_raw_quats, v_logits); a missing cotangent is zero.  Rows with
    filter == 0 take the unfiltered expressions."""
    t = dtype
    l, q, a, f = (np.asarray(x).astype(t) for x in (log_scales, raw_quats, logits, filt))
    a = a.reshape(-1)
    n = l.shape[0]
    vs = np.zeros((n, 3), t) if v_scales is None else np.asarray(v_scales).astype(t)
    vq = np.zeros((n, 4), t) if v_quats is None else np.asarray(v_quats).astype(t)
    vo = np.zeros(n, t) if v_opac is None else np.asarray(v_opac).astype(t).reshape(-1)
    one = t(1)
    with np.errstate(all="ignore"):
        s = np.exp(l).astype(t)
        o = (one / (one + np.exp(-a).astype(t))).astype(t)
        f2 = (f * f)[:, None]
        sp = np.sqrt(s * s + f2).astype(t)
        r = s / sp
        c = (r[:, 0] * r[:, 1]) * r[:, 2]
        tt = (f[:, None] / sp) * (f[:, None] / sp)
        on = f != 0
        scales = np.where(on[:, None], sp, s)
        opac = np.where(on, o * c, o)
        g_l = np.where(on[:, None], vs * (s * r) + ((vo * o) * c)[:, None] * tt, vs * s)
        g_a = np.where(on, ((vo * c) * o) * (one - o), (vo * o) * (one - o))
        inv = one / np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
        quats = q * inv[:, None]
        d = (((quats[:, 0] * vq[:, 0] + quats[:, 1] * vq[:, 1]) + quats[:, 2] * vq[:, 2]) + quats[:, 3] * vq[:, 3])
        g_q = (vq - quats * d[:, None]) * inv[:, None]
    return {"scales": scales.astype(t), "quats": quats.astype(t), "opacities": opac.astype(t)[:, None],
            "v_log_scales": g_l.astype(t), "v_raw_quats": g_q.astype(t), "v_logits": g_a.astype(t)[:, None]}


def activation_case(n: int, seed: int = 0):
    """Raw parameters, a filter and cotangents, float32: scales from exp(-12) to exp(2); filters 0 (a third of the rows
    from n >= 3 on) and 1e-4 ... 1, log-uniform -- f >> s, where c ~ (s / f)^3, included; logits in [-6, 6]."""
    rng = np.random.default_rng(seed)
    l = rng.uniform(-12.0, 2.0, (n, 3))
    f = np.exp(rng.uniform(np.log(1e-4), 0.0, n))
    if n >= 3:
        f[rng.permutation(n - 2)[: n // 3]] = 0.0
        l[n - 1], f[n - 1] = [-12.0, -12.0, 2.0], 1.0  # the corners of the ranges
        l[n - 2], f[n - 2] = [2.0, 2.0, 2.0], 1e-4
    return {"means": rng.normal(0, 2, (n, 3)).astype(F32), "log_scales": l.astype(F32),
            "raw_quats": rng.normal(0, 1, (n, 4)).astype(F32), "logits": rng.uniform(-6, 6, (n, 1)).astype(F32),
            "filter": f.astype(F32), "campos": np.array([0.3, -0.2, 5.0], F32),
            "v_scales": rng.normal(0, 1, (n, 3)).astype(F32), "v_quats": rng.normal(0, 1, (n, 4)).astype(F32),
            "v_opac": rng.normal(0, 1, (n, 1)).astype(F32)}


def rel_error(x, ref) -> float:
    """e(X) = max|X - X64| / max|X64| (0 for an all-zero reference matched exactly)."""
    x, ref = np.asarray(x, F64), np.asarray(ref, F64)
    top = np.abs(ref).max() if ref.size else 0.0
    err = np.abs(x - ref).max() if ref.size else 0.0
    return 0.0 if err == 0.0 else float(err / top)
