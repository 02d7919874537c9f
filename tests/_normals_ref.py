"""The rules of csrc/normals.hip (include/gsraster.h) restated as plain torch ops: float64 by
default, differentiable by autograd, and callable in float32 (`dtype=`) to measure what the same rule costs in single
precision.  tests/test_normals_host.py pins this file against analytic planes and central differences before
tests/test_gpu_normals.py holds the kernels to it.

Camera space is the projection's (x right, y down, z forward); the centre of pixel (row i, column j) is
(j + 0.5, i + 0.5)."""
import torch

F64 = torch.float64


def rotation(q):
    """[N,4] NORMALISED (w,x,y,z) -> [N,3,3], the projection's convention."""
    w, x, y, z = q.unbind(-1)
    return torch.stack([
        torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
        torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
        torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def smallest_axis(scales):
    """The index of the smallest of the three scales; a tie goes to the lowest index."""
    s0, s1, s2 = scales.unbind(-1)
    axis = torch.zeros(scales.shape[0], dtype=torch.int64, device=scales.device)
    sm = s0
    axis = torch.where(s1 < sm, torch.ones_like(axis), axis)
    sm = torch.where(s1 < sm, s1, sm)
    return torch.where(s2 < sm, torch.full_like(axis, 2), axis)


def gaussian_normals(quats, scales, means, viewmat, dtype=F64):
    """-> (normals [N,3], axis [N] int64, n . p_cam / |p_cam| before the flip [N])."""
    q, m, V = quats.to(dtype), means.to(dtype), viewmat.to(dtype)[:3]
    axis = smallest_axis(scales)  # (on the values as given: a cast up keeps the order)
    qn = q / q.norm(dim=-1, keepdim=True)
    R = rotation(qn)
    n_world = R.gather(2, axis[:, None, None].expand(-1, 3, 1))[..., 0]
    n_cam = n_world @ V[:, :3].T
    p_cam = m @ V[:, :3].T + V[:, 3]
    facing = (n_cam * p_cam).sum(-1)
    sign = torch.where(facing.detach() > 0, -torch.ones_like(facing), torch.ones_like(facing))
    return n_cam * sign[:, None], axis, facing.detach() / p_cam.detach().norm(dim=-1)


def _central(P, dim):
    """P[k+1] - P[k-1] along `dim` on the interior, zeros on the border."""
    n = P.shape[dim]
    out = torch.zeros_like(P)
    if n >= 3:
        out.narrow(dim, 1, n - 2).copy_(P.narrow(dim, 2, n - 2) - P.narrow(dim, 0, n - 2))
    return out


def _shift_all(ok):
    """ok of the pixel and of its four neighbours; False on the one-pixel border."""
    H, W = ok.shape
    out = torch.zeros_like(ok)
    if H >= 3 and W >= 3:
        out[1:-1, 1:-1] = ok[1:-1, 1:-1] & ok[:-2, 1:-1] & ok[2:, 1:-1] & ok[1:-1, :-2] & ok[1:-1, 2:]
    return out


def depth_normals(depth, alpha, fx, fy, cx, cy, dtype=F64):
    """-> (normals [H,W,3], exact zeros where invalid; valid [H,W] bool)."""
    D, a = depth.to(dtype), alpha.to(dtype)
    H, W = D.shape
    finite = torch.isfinite(D)
    ok = ~(a <= 0) & finite
    D = torch.where(finite, D, torch.ones_like(D))  # (never used where it matters: keeps NaN out of the autograd)
    jj = (torch.arange(W, dtype=dtype, device=D.device) + 0.5 - cx) / fx
    ii = (torch.arange(H, dtype=dtype, device=D.device) + 0.5 - cy) / fy
    P = torch.stack([jj[None, :] * D, ii[:, None] * D, D], -1)
    u, v = _central(P, 0), _central(P, 1)  # down - up, right - left
    c = torch.linalg.cross(u, v, dim=-1)
    l2 = (c * c).sum(-1)
    valid = _shift_all(ok) & (l2.detach() > 0) & torch.isfinite(l2.detach())
    n = c / torch.sqrt(torch.where(valid, l2, torch.ones_like(l2)))[..., None]
    return torch.where(valid[..., None], n, torch.zeros_like(n)), valid


def normal_consistency_loss(normals_img, depth, alpha, fx, fy, cx, cy, mask=None, dtype=F64):
    """mean over all pixels of m (1 - alpha <normals_img, n_d>); alpha is a weight (detached)."""
    n_d, _ = depth_normals(depth, alpha, fx, fy, cx, cy, dtype)
    a = alpha.detach().to(dtype)
    per = 1 - a * (normals_img.to(dtype) * n_d).sum(-1)
    if mask is not None:
        per = mask.to(dtype).reshape(per.shape) * per
    return per.mean()


def rel_err(x, x64):
    """e(X) = max |X - X64| / max |X64| (an all-zero X64: the absolute error)."""
    x, x64 = x.detach().to(F64), x64.detach().to(F64)
    if x64.numel() == 0:
        return 0.0
    top = float(x64.abs().max())
    return float((x - x64).abs().max()) / (top if top > 0 else 1.0)


# ---- seeded inputs shared by the GPU test, the bench and the host stand-in --------------------------------------------
def image_case(H, W, seed, masked):
    """Depth = plane + sinusoid + 1 % noise in [1, 5]; alpha in (0.2, 1] with 10 % zeros; normals_img in [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=F64)  # noqa: E731
    y, x = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    base = 3.0 + 0.8 * (x / max(W, 1) - 0.5) + 0.6 * (y / max(H, 1) - 0.5) + 0.5 * torch.sin(0.37 * x + 0.23 * y)
    depth = (base * (1 + 0.01 * (2 * r(H, W) - 1))).clamp(1.0, 5.0).float()
    alpha = (0.2 + 0.8 * (1 - r(H, W))).float()
    alpha = torch.where(r(H, W) < 0.1, torch.zeros_like(alpha), alpha)
    nimg = (2 * r(H, W, 3) - 1).float()
    mask = (r(H, W, 1) < 0.7).float() if masked else None
    f = 0.9 * max(W, H)
    return {"depth": depth, "alpha": alpha, "nimg": nimg, "mask": mask,
            "K": (f, 1.1 * f, 0.5 * W + 0.3, 0.5 * H - 0.2)}


def gaussian_case(n, seed, max_rounds=64):
    """Unnormalised quaternions with norms in [1e-3, 1e3], log- and exp'd scales mixed, a tenth of the rows with an
    exact tie of the two smallest scales.  A row on which the rule jumps -- |n . p| / |p| < 1e-3, or two smallest scales
    within 1e-3 relative of one another without being equal -- is drawn again.  -> (case, rounds used)."""
    g = torch.Generator().manual_seed(seed)
    yaw = 0.3
    V = torch.tensor([[torch.cos(torch.tensor(yaw)), 0.0, torch.sin(torch.tensor(yaw)), 0.1],
                      [0.0, 1.0, 0.0, -0.2],
                      [-torch.sin(torch.tensor(yaw)), 0.0, torch.cos(torch.tensor(yaw)), 4.0]], dtype=torch.float32)

    def draw(k):
        q = torch.randn(k, 4, generator=g, dtype=F64)
        q = q / q.norm(dim=-1, keepdim=True) * 10 ** (6 * torch.rand(k, 1, generator=g, dtype=F64) - 3)
        ls = torch.rand(k, 3, generator=g, dtype=F64) * 4 - 5  # log-scales in [-5, -1]
        s = torch.where(torch.rand(k, 1, generator=g) < 0.5, ls, ls.exp())  # per row: log-scales or exp'd
        m = torch.randn(k, 3, generator=g, dtype=F64)
        return q.float(), s.float(), m.float()

    def tie(s, rows):  # the two smallest of the row made exactly equal
        srt, idx = s[rows].sort(dim=-1)
        fixed = s[rows].clone()
        fixed.scatter_(1, idx[:, 1:2], srt[:, 0:1])
        s[rows] = fixed
        return s

    q, s, m = draw(n)
    tied = torch.arange(n) % 10 == 3
    s = tie(s, tied)
    for rounds in range(1, max_rounds + 1):
        _, _, facing = gaussian_normals(q, s, m, V)
        srt = s.double().sort(dim=-1).values
        near = ((srt[:, 1] - srt[:, 0]).abs() < 1e-3 * srt[:, :2].abs().amax(-1)) & (srt[:, 1] != srt[:, 0])
        bad = (facing.abs() < 1e-3) | near
        if not bool(bad.any()):
            return {"quats": q, "scales": s, "means": m, "viewmat": V, "tied": tied}, rounds
        k = int(bad.sum())
        q2, s2, m2 = draw(k)
        q[bad], s[bad], m[bad] = q2, s2, m2
        s = tie(s, tied)
    raise AssertionError(f"gaussian_case({n}, {seed}): rows on a jump of the rule were still drawn after {max_rounds} rounds")


def image_reference(case):
    """What the restatement returns for an `image_case`, with an upstream of 1: float64 `normals`, `valid`, `loss`,
    `v_nimg`, `v_depth`, `near_valid` (a pixel with a valid neighbour: where v_depth may be non-zero), and `e32`, the
    error e(X) of the same restatement run in float32, per output."""
    out = {}
    for dt in (F64, torch.float32):
        nimg = case["nimg"].to(dt).clone().requires_grad_(True)
        depth = case["depth"].to(dt).clone().requires_grad_(True)
        n_d, valid = depth_normals(case["depth"], case["alpha"], *case["K"], dtype=dt)
        loss = normal_consistency_loss(nimg, depth, case["alpha"], *case["K"], mask=case["mask"], dtype=dt)
        loss.backward()
        # (an image without an interior pixel: the loss does not hold the depth, autograd returns None for zeros)
        out[dt] = {"normals": n_d.detach(), "loss": loss.detach().reshape(1), "v_nimg": nimg.grad,
                   "v_depth": torch.zeros_like(depth) if depth.grad is None else depth.grad, "valid": valid}
    want = out[F64]
    v = want["valid"]
    near = torch.zeros_like(v)
    near[1:] |= v[:-1]
    near[:-1] |= v[1:]
    near[:, 1:] |= v[:, :-1]
    near[:, :-1] |= v[:, 1:]
    want["near_valid"] = near
    want["e32"] = {k: rel_err(out[torch.float32][k], want[k]) for k in ("normals", "loss", "v_nimg", "v_depth")}
    return want


def gaussian_reference(case, seed):
    """What the restatement returns for a `gaussian_case` and a seeded cotangent: float64 `normals`, `axis`, `v_quats`,
    the cotangent `v_normals` (float32) and `e32` per output."""
    g = torch.Generator().manual_seed(seed)
    v_normals = torch.randn(case["quats"].shape[0], 3, generator=g, dtype=F64).float()
    out = {}
    for dt in (F64, torch.float32):
        q = case["quats"].to(dt).clone().requires_grad_(True)
        n, axis, _ = gaussian_normals(q, case["scales"], case["means"], case["viewmat"], dtype=dt)
        (n * v_normals.to(dt)).sum().backward()
        out[dt] = {"normals": n.detach(), "axis": axis, "v_quats": q.grad}
    want = out[F64]
    want["v_normals"] = v_normals
    want["e32"] = {k: rel_err(out[torch.float32][k], want[k]) for k in ("normals", "v_quats")}
    return want
