"""Float64 references and float32 yardsticks of the per-step kernels: adam.hip, activations.hip (activations and
densification statistics) and the photometric / depth heads of loss.hip.  Plain NumPy, no torch, no GPU.

Every function takes a `dt` (np.float64 or np.float32) and evaluates ONE expression in that type: with float64 it is
the reference, with float32 -- every operation rounded on its own, NumPy never contracts -- it is the yardstick `y32`
of what float32 arithmetic costs for that expression.  The tests hold a kernel to

    |hip - f64| <= 2 * |y32 - f64| + floor                                (elementwise, `ratio` below)

with a derived forward-error `floor` per quantity (stated at the test), so no tolerance is fitted to a kernel.
Inputs are float32 arrays (what the kernels read); both evaluations start from the same float32 values.
"""
import numpy as np

F32, F64 = np.float32, np.float64
EPS32 = float(np.finfo(F32).eps)  # 2^-23: the spacing of float32 at 1


def ulp32(x):
    """The spacing of float32 at |x| (of the subnormals below the smallest normal number), as float64."""
    a = np.abs(np.asarray(x, F64))
    a = np.minimum(a, float(np.finfo(F32).max))
    return np.spacing(a.astype(F32)).astype(F64)


def ratio(hip, f64, y32, floor):
    """The worst |hip - f64| / (2 |y32 - f64| + floor) over the elements (0 for an empty array).  A non-finite
    `hip` where the reference is finite is an infinite ratio."""
    hip, f64, y32 = (np.asarray(a, F64) for a in (hip, f64, y32))
    floor = np.broadcast_to(np.asarray(floor, F64), f64.shape)
    if f64.size == 0:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(hip - f64)
        bound = 2.0 * np.abs(y32 - f64) + floor
        r = np.where(err == 0.0, 0.0, err / bound)
    r = np.where(np.isfinite(hip) | ~np.isfinite(f64), r, np.inf)
    return float(np.nan_to_num(r, nan=np.inf).max())


# ---------------------------------------------------------------------------------------------------------- Adam
def adam_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, dt=F64):
    """One step of torch.optim.Adam (amsgrad=False, weight_decay=0, maximize=False) from a given state; `step` is
    the number of THIS step (counts from 1).  -> (p, m, v).  The bias corrections are Python floats, as in torch
    (`_single_tensor_adam`); in float32 the per-element operations are torch's, in torch's order:
    `denom = sqrt(v) / sqrt(bc2) + eps; p -= (lr / bc1) * (m / denom)`.  The learning rate is an input like the
    arrays: the float32 value the C ABI carries (`gsr_adam_tensor.lr`), in both types."""
    b1, b2, lr = float(betas[0]), float(betas[1]), float(F32(lr))
    p, g, m, v = (np.asarray(a, dt) for a in (p, g, m, v))
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    with np.errstate(under="ignore"):
        m = m * dt(b1) + g * dt(1.0 - b1)
        v = v * dt(b2) + (g * g) * dt(1.0 - b2)
        denom = np.sqrt(v) / dt(np.sqrt(bc2)) + dt(eps)
        p = p - dt(lr / bc1) * (m / denom)
    return p, m, v


# ---------------------------------------------------------------------------------------------------- activations
def activate_forward(means, log_scales, raw_quats, logits, campos, dt=F64):
    """-> (exp(log_scales), raw_quats / |raw_quats|, sigmoid(logits), normalised (means - campos) or None)."""
    ls, rq, lo = (np.asarray(a, dt) for a in (log_scales, raw_quats, logits))
    with np.errstate(over="ignore", under="ignore"):
        scales = np.exp(ls)
        quats = rq / np.sqrt((rq * rq).sum(-1, keepdims=True, dtype=dt))
        opac = dt(1) / (dt(1) + np.exp(-lo))
    dirs = None
    if campos is not None:
        d = np.asarray(means, dt) - np.asarray(campos, dt).reshape(1, 3)
        dirs = d / np.sqrt((d * d).sum(-1, keepdims=True, dtype=dt))
    return scales, quats, opac, dirs


def activate_vjp(log_scales, raw_quats, logits, v_scales, v_quats, v_opac, dt=F64):
    """The vector-Jacobian product of `activate_forward` w.r.t. (log_scales, raw_quats, logits); a None cotangent is
    zero.  v_log_scale = v_scale * scale;  v_raw = (v - q (q . v)) / |raw|;  v_logit = v_o * o * (1 - o), with
    scale, q, o the forward's values IN `dt` (the kernel reads its own float32 forward outputs)."""
    scales, quats, opac, _ = activate_forward(None, log_scales, raw_quats, logits, None, dt)
    rq = np.asarray(raw_quats, dt)
    g_s = np.zeros_like(scales) if v_scales is None else np.asarray(v_scales, dt) * scales
    if v_quats is None:
        g_q = np.zeros_like(quats)
    else:
        v = np.asarray(v_quats, dt)
        inv = dt(1) / np.sqrt((rq * rq).sum(-1, keepdims=True, dtype=dt))
        d = (quats * v).sum(-1, keepdims=True, dtype=dt)
        g_q = (v - quats * d) * inv
    g_o = np.zeros_like(opac) if v_opac is None else np.asarray(v_opac, dt) * opac * (dt(1) - opac)
    return g_s, g_q, g_o


def quat_grad_floor(raw_quats, v_quats):
    """8 eps32 (|v_k| + |q_k| |q . v|) / |raw|: the forward error of the difference v - q (q . v), which cancels where
    v is parallel to q -- each of its two terms carries a few roundings (q itself, the 4-term dot product, the
    product), none of which shrinks with the difference."""
    rq, v = np.asarray(raw_quats, F64), np.asarray(v_quats, F64)
    nrm = np.sqrt((rq * rq).sum(-1, keepdims=True))
    q = rq / nrm
    return 8.0 * EPS32 * (np.abs(v) + np.abs(q) * np.abs((q * v).sum(-1, keepdims=True))) / nrm


# ---------------------------------------------------------------------------------------- densification statistics
def densify_stats(xys_grad, radii, image_size, grad_norm, counts, max_size, first, dt=F64):
    """GaussianSplattingModel.after_train: -> new (grad_norm, counts, max_size).  `first`: every Gaussian starts
    with count 1, its own gradient norm (visible or not; 0 without gradients) and radius / image_size where the radius
    is positive, 0 elsewhere -- whatever the accumulators held.  Later: the rows with radius > 0 add their norm,
    count one more and take the maximum; the others are unchanged.  `xys_grad` None: the norms are not touched
    (zero on a first call)."""
    r = np.asarray(radii)
    n = r.shape[0]
    vis = r > 0
    inv = dt(F32(1.0 / float(image_size)))  # the binding hands the kernel a float32 reciprocal
    size = r.astype(dt) * inv
    norm = np.zeros(n, dt)
    if xys_grad is not None:
        g = np.asarray(xys_grad, dt)
        with np.errstate(under="ignore"):
            norm = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1])
    if first:
        return norm, np.ones(n, np.int32), np.where(vis, np.maximum(dt(0), size), dt(0))
    gn, ms = np.asarray(grad_norm, dt), np.asarray(max_size, dt)
    return (np.where(vis, gn + norm, gn), np.asarray(counts, np.int32) + vis.astype(np.int32),
            np.where(vis, np.maximum(ms, size), ms))


# ------------------------------------------------------------------------------------------------- L1, depth heads
def _masked(x, mask, dt):
    if mask is None:
        return x
    m = np.asarray(mask, dt)
    return x * m.reshape(m.shape + (1,) * (x.ndim - m.ndim))


def l1_head(pred, gt, weight=1.0, clamp_pred=False, mask=None, upstream=1.0, dt=F64):
    """weight * mean |x - y| with x = min(pred, 1) * mask, y = gt * mask (mask [H,W] for [H,W,3] images) and its
    gradient w.r.t. pred times `upstream`: weight * sign(x - y) * mask / n, zero where the clamp cuts.
    -> (loss, v_pred).  The mean is summed in `dt` too (NumPy's pairwise sum in float32)."""
    p, y = np.asarray(pred, dt), np.asarray(gt, dt)
    x = np.minimum(p, dt(1)) if clamp_pred else p
    x, y = _masked(x, mask, dt), _masked(y, mask, dt)
    d = x - y
    n = d.size
    loss = float(dt(F32(weight)) * (np.abs(d).sum(dtype=dt) / dt(n)))
    g = (dt(F32(upstream)) * dt(F32(weight)) / dt(n)) * np.sign(d)  # (the kernels take both as float32)
    g = _masked(g, mask, dt)
    if clamp_pred:
        g = np.where(p > dt(1), dt(0), g)
    return loss, g


def depth_head(depth, alpha, gt, mask=None, upstream=1.0, dt=F64):
    """pred = where(alpha > 0, depth / alpha, max(depth)); g = gt * mask, p = pred * mask; loss = the mean over ALL
    pixels of |g - p| where g > 0.  -> (loss, v_depth, v_alpha); the far value is a constant."""
    d, a, g = (np.asarray(t, dt).reshape(-1) for t in (depth, alpha, gt))
    n = d.size
    m = np.ones(n, dt) if mask is None else np.asarray(mask, dt).reshape(-1)
    cov = a > 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = dt(1) / np.where(cov, a, dt(1))
        pred = np.where(cov, d * inv, d.max())
        gm, pm = g * m, pred * m
        hit = gm > 0
        loss = float(np.where(hit, np.abs(gm - pm), dt(0)).sum(dtype=dt) / dt(n))
        vp = (dt(F32(upstream)) * np.sign(pm - gm) / dt(n)) * m
        use = hit & cov
        v_d = np.where(use, vp * inv, dt(0))
        v_a = np.where(use, -vp * pred * inv, dt(0))
    return loss, v_d, v_a


# ------------------------------------------------------------------------------------------------------------ SSIM
def ssim_window(dt=F64):
    """The normalised 11-tap Gaussian, sigma 1.5 (pytorch_msssim._fspecial_gauss_1d), rounded to `dt`."""
    k = np.arange(11, dtype=F64) - 5.0
    w = np.exp(-(k * k) / (2.0 * 1.5 * 1.5))
    return (w / w.sum()).astype(dt)


SSIM_C1, SSIM_C2 = 0.01 ** 2, 0.03 ** 2


def _blur_valid(a, w, axis):
    """11-tap VALID correlation along `axis` (0 or 1) of [H,W,C], taps accumulated in order in a's type."""
    n = a.shape[axis] - 10
    out = np.zeros_like(a[:n] if axis == 0 else a[:, :n])
    for k in range(11):
        out = out + w[k] * (a[k:k + n] if axis == 0 else a[:, k:k + n])
    return out


def _blur_transposed(a, w, axis):
    """The transpose of `_blur_valid`: [.., n, ..] -> [.., n + 10, ..], output i gathers inputs i - k with w[k]."""
    n = a.shape[axis]
    pad = [(0, 0)] * a.ndim
    pad[axis] = (10, 10)
    z = np.pad(a, pad)
    out = np.zeros_like(z[:n + 10] if axis == 0 else z[:, :n + 10])
    for k in range(11):
        s = 10 - k
        out = out + w[k] * (z[s:s + n + 10] if axis == 0 else z[:, s:s + n + 10])
    return out


def l1_ssim(pred, gt, ssim_lambda=0.2, clamp_pred=False, upstream=1.0, dt=F64, with_terms=False):
    """(1 - lambda) mean|x - y| + lambda (1 - SSIM(x, y)), x = min(pred, 1) under `clamp_pred`, and d / d pred times
    `upstream` -- the separable algorithm: a horizontal 11-tap pass of x, y, x^2, y^2, xy, then a vertical one; S and
    its partials per valid position; the transposed passes of the three derivative maps.  The means are summed in `dt`.
    -> (loss, l1, ssim, v_pred[, abs_terms]): `abs_terms` is, per pixel, |L1 term| + |k_ss| * sum over the taps of
    |w_k w_l| (|Dmu| + |2 x D11| + |y D12|), times |upstream| -- what the gradient's roundings scale with."""
    p, y = np.asarray(pred, dt), np.asarray(gt, dt)
    x = np.minimum(p, dt(1)) if clamp_pred else p
    H, W, _ = x.shape
    w = ssim_window(dt)
    lam = dt(F32(ssim_lambda))  # the kernels take a float32 lambda
    if dt is F32:  # 0.01f * 0.01f, 0.03f * 0.03f
        c1, c2 = F32(0.01) * F32(0.01), F32(0.03) * F32(0.03)
    else:
        c1, c2 = dt(SSIM_C1), dt(SSIM_C2)
    two = dt(2)
    blur = lambda a: _blur_valid(_blur_valid(a, w, 1), w, 0)  # noqa: E731
    mu1, mu2, e11, e22, e12 = blur(x), blur(y), blur(x * x), blur(y * y), blur(x * y)
    s11, s22, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
    A1, A2 = two * mu1 * mu2 + c1, two * s12 + c2
    B1, B2 = mu1 * mu1 + mu2 * mu2 + c1, s11 + s22 + c2
    inv = dt(1) / (B1 * B2)
    S = A1 * A2 * inv
    dA1, dA2, dB1, dB2 = A2 * inv, A1 * inv, -S / B1, -S / B2
    d_mu = dA1 * (two * mu2) + dB1 * (two * mu1) + dA2 * (-two * mu2) + dB2 * (-two * mu1)
    d11, d12 = dB2, two * dA2
    d = x - y
    l1 = np.abs(d).sum(dtype=dt) / dt(d.size)
    ssim = S.sum(dtype=dt) / dt(S.size)
    loss, l1, ssim = float((dt(1) - lam) * l1 + lam * (dt(1) - ssim)), float(l1), float(ssim)
    blur_t = lambda a: _blur_transposed(_blur_transposed(a, w, 1), w, 0)  # noqa: E731
    up = dt(F32(upstream))
    k_l1 = up * (dt(1) - lam) / (dt(3) * dt(H) * dt(W))
    k_ss = -up * lam / (dt(3) * dt(H - 10) * dt(W - 10))
    g = k_l1 * np.sign(d) + k_ss * (blur_t(d_mu) + two * x * blur_t(d11) + y * blur_t(d12))
    if clamp_pred:
        g = np.where(p > dt(1), dt(0), g)
    if not with_terms:
        return loss, l1, ssim, g
    wa = np.abs(w)
    blur_ta = lambda a: _blur_transposed(_blur_transposed(np.abs(a), wa, 1), wa, 0)  # noqa: E731
    terms = np.abs(k_l1 * np.sign(d)) + np.abs(k_ss) * (blur_ta(d_mu) + np.abs(two * x) * blur_ta(d11)
                                                         + np.abs(y) * blur_ta(d12))
    return loss, l1, ssim, g, terms
