"""Inputs of the edge tests of the per-step kernels (tests/test_gpu_fused_step_edges.py), built on the host so that
tests/test_fused_step_host.py can check what the GPU tests rely on (the share of near-tie pixels, the classes
present) without a GPU.  float32 NumPy arrays, deterministic."""
import numpy as np

F32 = np.float32

# ------------------------------------------------------------------------------------------------------------ Adam
ADAM_STEPS = (1, 2, 10, 1000, 30_000, 10 ** 6)
ADAM_LRS = (1.6e-4, 0.0025, 0.0025 / 20, 0.05, 0.005, 0.001, 1.6e-6)  # the toolkit's six + the decayed means' rate
ADAM_EPS = (1e-15, 1e-8)
ADAM_BETAS = ((0.9, 0.999), (0.0, 0.9))
ADAM_CLASSES = ("g_loguniform", "g_zero_live_state", "all_zero", "m_against_g", "v_large", "p_below_one_step",
                "p_zero", "p_near_1", "p_near_100")


def adam_elements(n, seed):
    """-> (p, g, m, v, cls): n elements, the classes of ADAM_CLASSES interleaved (cls[i] indexes ADAM_CLASSES)."""
    rng = np.random.default_rng(seed)
    k = len(ADAM_CLASSES)
    cls = (np.arange(n) + seed) % k
    sign = lambda: rng.choice([-1.0, 1.0], n)  # noqa: E731
    g = sign() * 10.0 ** rng.uniform(-20, 3, n)
    m = sign() * np.abs(g) * 10.0 ** rng.uniform(-2, 1, n)
    v = g * g * 10.0 ** rng.uniform(-2, 2, n)
    p = rng.standard_normal(n)
    is_ = lambda name: cls == ADAM_CLASSES.index(name)  # noqa: E731
    c = is_("g_zero_live_state")
    g[c] = 0.0
    m[c] = (sign() * 10.0 ** rng.uniform(-8, 0, n))[c]
    v[c] = (10.0 ** rng.uniform(-16, 0, n))[c]
    c = is_("all_zero")
    g[c] = m[c] = v[c] = 0.0
    c = is_("m_against_g")  # b1 m + (1 - b1) g cancels to a few per cent of either term at betas (0.9, 0.999)
    g[c] = (sign() * 10.0 ** rng.uniform(-6, 0, n))[c]
    m[c] = (-g * (0.1 / 0.9) * rng.uniform(0.9, 1.1, n))[c]
    v[c] = (g * g * rng.uniform(0.5, 2, n))[c]
    c = is_("v_large")
    g[c] = (sign() * 10.0 ** rng.uniform(0, 3, n))[c]
    m[c] = (sign() * 10.0 ** rng.uniform(0, 3, n))[c]
    v[c] = (10.0 ** rng.uniform(3, 6, n))[c]
    c = is_("p_below_one_step")  # |p| far below lr: the result is the update itself
    p[c] = (sign() * 10.0 ** rng.uniform(-12, -7, n))[c]
    p[is_("p_zero")] = 0.0
    c = is_("p_near_1")
    p[c] = (sign() * (1.0 + rng.uniform(-1e-3, 1e-3, n)))[c]
    c = is_("p_near_100")
    p[c] = (sign() * (100.0 + rng.uniform(-1e-1, 1e-1, n)))[c]
    with np.errstate(under="ignore"):
        return p.astype(F32), g.astype(F32), m.astype(F32), v.astype(F32), cls


PATH_SIZES = (1, 2, 3, 4, 5, 1023, 1025, 4095, 4096, 4097, 16_387)

# ----------------------------------------------------------------------------------------------------- activations
ACT_SIZES = (1, 255, 256, 257, 1000)
LOGITS = (0.0, -0.0, 1e-3, -1e-3, 10.0, -10.0, 17.0, -17.0, 88.0, -88.0, 104.0, -104.0)
COTANGENT_KINDS = ("parallel", "antiparallel", "orthogonal", "zero", "random")


def activation_inputs(n, seed):
    """-> dict(means, log_scales, raw_quats, logits, campos): the issue's edge values cycled over the rows."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    logits = np.array(LOGITS, F32)[i % len(LOGITS)].reshape(n, 1)
    log_scales = rng.uniform(-20, 10, (n, 3)).astype(F32)
    log_scales[i % 7 == 0] = np.array([-20.0, 10.0, 0.0], F32)
    norms = 10.0 ** rng.uniform(-3, 3, n)
    norms[i % 5 == 0] = 1e-3
    norms[i % 5 == 1] = 1e3
    q = np.zeros((n, 4))
    kind = i % 4
    axis = rng.integers(0, 4, n)
    for r in range(n):
        if kind[r] == 0:    # axis-aligned: three zeros
            q[r, axis[r]] = rng.choice([-1.0, 1.0])
        elif kind[r] == 1:  # one dominant component
            q[r] = rng.standard_normal(4) * 1e-4
            q[r, axis[r]] = 1.0
        elif kind[r] == 2:  # all equal
            q[r] = 0.5 * rng.choice([-1.0, 1.0])
        else:
            q[r] = rng.standard_normal(4)
    q = q / np.linalg.norm(q, axis=1, keepdims=True) * norms[:, None]
    campos = np.array([0.3, -1.7, 2.9], F32)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dist = np.where(i % 2 == 0, 1e-3, 1e4)
    means = (campos.astype(np.float64) + d * dist[:, None]).astype(F32)
    return dict(means=means, log_scales=log_scales, raw_quats=q.astype(F32), logits=logits, campos=campos)


def activation_cotangents(raw_quats, seed):
    """-> (v_scales, v_quats, v_opac): the quaternion cotangents cycle through COTANGENT_KINDS relative to q."""
    rng = np.random.default_rng(seed)
    n = raw_quats.shape[0]
    q = raw_quats.astype(np.float64)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    v = rng.standard_normal((n, 4))
    kind = np.arange(n) % len(COTANGENT_KINDS)
    amp = 10.0 ** rng.uniform(-3, 3, (n, 1))
    ortho = v - q * (q * v).sum(1, keepdims=True)
    v = np.where((kind == 0)[:, None], q * amp, v)
    v = np.where((kind == 1)[:, None], -q * amp, v)
    v = np.where((kind == 2)[:, None], ortho * amp, v)
    v = np.where((kind == 3)[:, None], 0.0, v)
    v_scales = (rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-6, 2, (n, 3))).astype(F32)
    v_opac = (rng.standard_normal((n, 1)) * 10.0 ** rng.uniform(-6, 2, (n, 1))).astype(F32)
    v_scales[np.arange(n) % 6 == 0] = 0.0
    v_opac[np.arange(n) % 6 == 1] = 0.0
    return v_scales, v.astype(F32), v_opac


def densify_inputs(n, seed):
    """-> (xys_grad [n,2], radii [n] int32 cycling through -1, 0, 1, 300)."""
    rng = np.random.default_rng(seed)
    radii = np.array([-1, 0, 1, 300], np.int32)[np.arange(n) % 4]
    g = rng.standard_normal((n, 2)) * 10.0 ** rng.uniform(-12, 2, (n, 1))
    return g.astype(F32), radii


# ------------------------------------------------------------------------------------------------------- L1 + SSIM
# (H, W): the forward kernel tiles the valid map (H-10) x (W-10) by 16 x 32 and the backward the image by 16 x 32, so
# W 11 / 32 / 33 / 42 / 43 and H 11 / 16 / 17 / 26 / 27 are one valid column/row, one image tile, one more pixel, one
# valid tile, one more valid position.
SSIM_SIZES = ((11, 11), (16, 32), (17, 33), (26, 42), (27, 43), (11, 43), (27, 11))


def _texture(rng, H, W, lo=0.05, hi=0.95):
    """A smooth image with every pixel different: low-frequency waves per channel plus a little noise."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.empty((H, W, 3))
    for c in range(3):
        fx, fy, ph = rng.uniform(0.05, 0.4), rng.uniform(0.05, 0.4), rng.uniform(0, 6.28)
        img[..., c] = 0.5 + 0.4 * np.sin(fx * xx + fy * yy + ph) + 0.02 * rng.standard_normal((H, W))
    return lo + (hi - lo) * np.clip(img, 0.0, 1.0)


def ssim_cases():
    """-> list of dicts(name, pred, gt, lam, clamp, up, equal): structured content at the sizes of SSIM_SIZES (cycled,
    every size used).  `equal`: pred == gt everywhere (the one kind of case where the near-tie share is not capped)."""
    rng = np.random.default_rng(20240)
    sizes = list(SSIM_SIZES)
    state = {"k": 0}
    out = []

    def size():
        s = sizes[state["k"] % len(sizes)]
        state["k"] += 1
        return s

    def add(name, pred, gt, lam=0.2, clamp=False, up=1.0, equal=False):
        out.append(dict(name=name, pred=np.ascontiguousarray(pred, F32), gt=np.ascontiguousarray(gt, F32), lam=lam,
                        clamp=clamp, up=up, equal=equal))

    for lam in (0.0, 0.2, 1.0):  # pred == gt exactly
        H, W = size()
        t = _texture(rng, H, W)
        add(f"equal_lam{lam}", t, t, lam=lam, equal=True, up=0.75 if lam == 0.2 else 1.0)
    for c1 in (0.0, 0.5, 1.0):  # constant pairs, black on black included
        for c2 in (0.0, 0.5, 1.0):
            H, W = size()
            add(f"const_{c1}_{c2}", np.full((H, W, 3), c1), np.full((H, W, 3), c2), equal=c1 == c2,
                clamp=(c1 == 1.0), lam=0.2 if c1 != 0.5 else 1.0)
    for bg_p, bg_g in ((0.30, 0.32), (0.0, 0.02), (1.0, 0.97)):  # flat background, one textured blob of <= 8 px
        H, W = size()
        pred, gt = np.full((H, W, 3), bg_p), np.full((H, W, 3), bg_g)
        y0, x0 = H // 2 - 1, W // 2 - 2
        pred[y0:y0 + 2, x0:x0 + 4] = rng.uniform(0.1, 0.9, (2, 4, 3))  # 8 px
        gt[y0:y0 + 2, x0:x0 + 3] = rng.uniform(0.1, 0.9, (2, 3, 3))
        add(f"blob_{bg_p}", pred, gt, up=-2.5 if bg_p == 0.0 else 1.0)
    for k in range(3):  # linear ramps, along x against along y / against another slope
        H, W = size()
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        pred = np.stack([xx / (W - 1), yy / (H - 1), (xx + yy) / (W + H - 2)], -1)
        gt = np.stack([0.83 * xx / (W - 1) + 0.0537, 0.31 + 0.0 * yy, 1.0 - (xx + 1.37 * yy) / (W + 1.37 * H)], -1)
        add(f"ramp_{k}", pred, gt, lam=(0.0, 0.2, 1.0)[k], up=(1.0, 0.37, 1.0)[k])
    for clamp in (False, True):  # pred up to 1.4; pred exactly 1.0 in a region (the clamp passes the gradient there)
        H, W = size()
        gt = _texture(rng, H, W, 0.05, 0.9)
        pred = gt * 1.4 + 0.011
        pred[2:6, 3:9] = 1.0
        pred[H - 3:, :4] = 1.4
        add(f"over_one_clamp{int(clamp)}", pred, gt, clamp=clamp, up=1.7)
    H, W = size()  # negative pred, no clamp
    gt = _texture(rng, H, W)
    add("negative_pred", gt - 0.35, gt, lam=0.2)
    H, W = size()  # saturated: both images sit at 0 / 1 over large regions, different ones
    gt = np.round(_texture(rng, H, W, 0.0, 1.0))
    pred = np.clip(1.3 * _texture(rng, H, W, 0.0, 1.0) - 0.15, 0.0, 1.0) * 0.98 + 0.01
    add("saturated", pred, gt, lam=0.2)
    assert state["k"] >= len(sizes)
    return out


def near_tie(pred, gt, clamp):
    """The pixels within 1e-6 of x == y (x = min(pred, 1) under the clamp): the L1 sign is ill-conditioned there."""
    x = np.minimum(pred, F32(1)) if clamp else pred
    return np.abs(x.astype(np.float64) - gt.astype(np.float64)) <= 1e-6


# ------------------------------------------------------------------------------------------------ L1, depth heads
# n = 3 H W: 3 (< 4), 6, 15, 105, 48 -- n % 4 = 3, 2, 3, 1, 0 -- and 4551: more than one workgroup forward (n / 4 > 1024)
L1_SHAPES = ((1, 1), (2, 1), (1, 5), (5, 7), (4, 4), (37, 41))


def l1_case(H, W, seed):
    """-> (pred, gt, mask): [H,W,3] images with pred == gt, pred == 1.0 and pred > 1 elements, a non-binary mask."""
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0, 1, (H, W, 3)).astype(F32)
    pred = (gt + rng.uniform(-0.3, 0.5, (H, W, 3))).astype(F32)
    flat_p, flat_g = pred.reshape(-1), gt.reshape(-1)
    n = flat_p.size
    flat_p[0::5] = flat_g[0::5]   # pred == gt
    flat_p[1::7] = 1.0            # exactly 1: the clamp passes
    if n > 2:
        flat_p[2::11] = 1.25      # cut by the clamp
    mask = rng.choice(np.array([0.0, 1.0, 0.5, 0.3], F32), (H, W)).astype(F32)
    return pred, gt, mask


def depth_case(n, seed, covered=True):
    """-> (depth, alpha, gt, mask), n pixels as [n,1]: alpha == 0 pixels, holes (gt == 0), a non-binary mask."""
    rng = np.random.default_rng(seed)
    alpha = rng.uniform(0.05, 1.0, (n, 1)).astype(F32)
    depth = (alpha * rng.uniform(0.5, 20.0, (n, 1))).astype(F32)
    gt = rng.uniform(0.5, 20.0, (n, 1)).astype(F32)
    if n > 1:
        alpha[0::3] = 0.0
        gt[1::4] = 0.0
        k = min(n - 1, 5)
        gt[k] = depth[k] / alpha[k] if alpha[k] > 0 else gt[k]  # pred == gt where covered
    if not covered:
        alpha[:] = 0.0
    mask = rng.choice(np.array([0.0, 1.0, 0.5, 0.25], F32), (n, 1)).astype(F32)
    return depth, alpha, gt, mask
