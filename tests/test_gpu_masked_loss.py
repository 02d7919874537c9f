"""The masked loss heads (gs_fused.l1_ssim_loss / l1_loss / depth_l1_loss with `mask=`): against float64 golden
vectors, against the unmasked kernels fed `pred * m`, `gt * m`, and at the edges of the mask argument."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_golden_masked_loss import CASES, UNSTABLE, UNSTABLE_CAP, case_name  # noqa: E402


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "masked_loss.npz")))


@pytest.mark.parametrize("key,kind,clamp", CASES, ids=[case_name(*c) for c in CASES])
def test_masked_l1_ssim_vs_golden(golden, key, kind, clamp):
    """Bounds of test_loss_head.test_hip_vs_golden_and_oracle; the golden gradient is float64 autograd of the models'
    `pred * mask`, `gt * mask` lines.  Elements with 0 < |m (pred - gt)| <= 1e-6 may flip the sign term between the
    precisions and are left out -- at most 0.1 % of a case (the generator asserts the same of its inputs)."""
    import torch

    from gs_fused import l1_ssim_loss

    g, n = golden, case_name(key, kind, clamp)
    lam = float(g["lambda"])
    pred = torch.from_numpy(g[f"{key}_pred"]).cuda().requires_grad_(True)
    gt = torch.from_numpy(g[f"{key}_gt"]).cuda()
    mask = torch.from_numpy(g[f"{key}_mask_{kind}"]).cuda()
    loss, l1, ss = l1_ssim_loss(pred, gt, lam, return_terms=True, clamp_pred=clamp, mask=mask)
    print(n, float(loss) - float(g[f"{n}_loss"]), float(l1) - float(g[f"{n}_l1"]), float(ss) - float(g[f"{n}_ssim"]))
    assert abs(float(loss) - float(g[f"{n}_loss"])) < 1e-5
    assert abs(float(l1) - float(g[f"{n}_l1"])) < 1e-6
    assert abs(float(ss) - float(g[f"{n}_ssim"])) < 1e-5
    (3.0 * loss).backward()
    got = pred.grad.cpu().numpy() / 3.0
    ref = g[f"{n}_grad"]
    p64 = g[f"{key}_pred"].astype(np.float64)
    d = np.abs(g[f"{key}_mask_{kind}"].astype(np.float64)[..., None] * ((np.minimum(p64, 1.0) if clamp else p64)
                                                                         - g[f"{key}_gt"]))
    unstable = (d > 0) & (d <= UNSTABLE)
    assert unstable.mean() <= UNSTABLE_CAP
    err = np.abs(got - ref)[~unstable].max()
    print(n, "grad max err", err, "max ref", np.abs(ref).max())
    assert err < 1e-7 + 1e-4 * np.abs(ref).max()
    if kind == "zeros":
        assert float(loss) == 0.0 and not got.any()


def _images(H, W, seed, hi=1.4):
    import torch

    rng = np.random.default_rng(seed)
    gt = torch.from_numpy(rng.uniform(0, 1, (H, W, 3)).astype(np.float32)).cuda()
    base = torch.from_numpy(rng.uniform(0, hi, (H, W, 3)).astype(np.float32)).cuda()
    base[2:5, 3:6] = gt[2:5, 3:6]  # exact matches: sign(0) = 0 must survive the two multiplies
    m = rng.uniform(0, 1, (H, W))
    m = np.where(m < 0.3, 0.0, np.where(m > 0.6, 1.0, m)).astype(np.float32)  # zeros, ones and fractions
    return gt, base, torch.from_numpy(m).cuda()


@pytest.mark.parametrize("clamp", [False, True])
def test_masked_l1_ssim_equals_multiplies_around_unmasked(clamp):
    """l1_ssim_loss(p, g, mask=m) == l1_ssim_loss(p * m, g * m) (clamp: torch.clamp(p, max=1) * m), value and gradient:
    tolerances of test_loss_head.test_clamp_pred_equals_torch_clamp."""
    import torch

    from gs_fused import l1_ssim_loss

    gt, base, m = _images(97, 131, 5)
    a = base.clone().requires_grad_(True)
    b = base.clone().requires_grad_(True)
    m3 = m[..., None]
    la, l1a, sa = l1_ssim_loss(a, gt, 0.2, return_terms=True, clamp_pred=clamp, mask=m)
    lb, l1b, sb = l1_ssim_loss((torch.clamp(b, max=1.0) if clamp else b) * m3, gt * m3, 0.2, return_terms=True)
    print(float(la) - float(lb), float(l1a) - float(l1b), float(sa) - float(sb))
    assert abs(float(la) - float(lb)) < 1e-6 and abs(float(l1a) - float(l1b)) < 1e-6 and abs(float(sa) - float(sb)) < 1e-6
    la.backward()
    lb.backward()
    print(float((a.grad - b.grad).abs().max()))
    assert torch.allclose(a.grad, b.grad, rtol=1e-6, atol=1e-9)
    zero = (m == 0)[..., None].expand_as(base)
    assert int(zero.sum()) > 1000 and float(a.grad[zero].abs().max()) == 0.0
    if clamp:
        assert float(a.grad[base > 1].abs().max()) == 0.0 and int((base > 1).sum()) > 1000


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("H,W", [(5, 7), (16, 16), (33, 47)])
def test_masked_l1_equals_multiplies_around_unmasked(H, W, clamp):
    """The co-gs photometric head.  3 * 5 * 7 = 105 values: a tail behind the last float4, and pixels split across
    float4 borders at every phase."""
    import torch

    from gs_fused import l1_loss

    gt, base, m = _images(H, W, 11 + H)
    a = base.clone().requires_grad_(True)
    b = base.clone().requires_grad_(True)
    m3 = m[..., None]
    la = l1_loss(a, gt, 0.8, clamp_pred=clamp, mask=m)
    lb = l1_loss((torch.clamp(b, max=1.0) if clamp else b) * m3, gt * m3, 0.8)
    assert abs(float(la) - float(lb)) < 1e-6
    ref = 0.8 * ((torch.clamp(base, max=1.0) if clamp else base).double() * m3.double() - gt.double() * m3.double()).abs().mean()
    assert abs(float(la) - float(ref)) < 1e-6
    la.backward()
    lb.backward()
    assert torch.allclose(a.grad, b.grad, rtol=1e-6, atol=1e-9)
    zero = (m == 0)[..., None].expand_as(base)
    assert float(a.grad[zero].abs().max()) == 0.0
    assert float(a.grad[2:5, 3:6].abs().max()) == 0.0  # pred == gt


def test_masked_depth_l1_equals_torch_ops():
    """depth_l1_loss(..., mask=m) == the torch expression: g = gt * m, p = pred * m, |g * (g > 0) - p * (g > 0)|.mean()
    with pred = where(alpha > 0, depth / alpha, max depth); inputs and tolerances of
    test_loss_head.test_depth_l1_head_equals_torch_ops."""
    import torch

    from gs_fused import depth_l1_loss

    rng = np.random.default_rng(9)
    H, W = 120, 200
    alpha = np.clip(rng.uniform(-0.3, 1.0, (H, W, 1)), 0, 1).astype(np.float32)
    depth = (alpha * rng.uniform(1, 9, (H, W, 1))).astype(np.float32)
    gt = (rng.uniform(0.5, 10, (H, W)) * (rng.uniform(0, 1, (H, W)) > 0.2)).astype(np.float32)
    mk = rng.uniform(0, 1, (H, W))
    mk = np.where(mk < 0.3, 0.0, np.where(mk > 0.6, 1.0, mk)).astype(np.float32)
    d1, a1 = (torch.from_numpy(x).cuda().requires_grad_(True) for x in (depth, alpha))
    d2, a2 = (torch.from_numpy(x).cuda().requires_grad_(True) for x in (depth, alpha))
    g, m = torch.from_numpy(gt).cuda(), torch.from_numpy(mk).cuda()
    mine = depth_l1_loss(d1, a1, g, mask=m)
    pred = torch.where(a2 > 0, d2 / a2, d2.detach().max()).squeeze(-1)
    gm, pm = g * m, pred * m
    nz = gm > 0
    ref = torch.abs(gm * nz - pm * nz).mean()
    assert abs(float(mine) - float(ref)) < 1e-6 * max(1.0, float(ref))
    (2.5 * mine).backward()
    (2.5 * ref).backward()
    cov = a2.detach() > 0  # (alpha == 0: torch's 0 * inf = nan, here 0 -- as in the unmasked test)
    assert float(d1.grad[~cov].abs().max()) == 0.0 and float(a1.grad[~cov].abs().max()) == 0.0
    assert torch.allclose(d1.grad[cov], d2.grad[cov], rtol=1e-5, atol=1e-9)
    assert torch.allclose(a1.grad[cov], a2.grad[cov], rtol=1e-5, atol=1e-8)
    off = (m == 0)[..., None]
    assert float(d1.grad[off].abs().max()) == 0.0 and float(a1.grad[off].abs().max()) == 0.0
    assert float(d1.grad.abs().max()) > 0


def test_constant_masks():
    """All ones == the unmasked call; all zeros: L1 0, SSIM of two zero images 1, loss 0, gradient 0."""
    import torch

    from gs_fused import depth_l1_loss, l1_loss, l1_ssim_loss

    gt, base, _ = _images(40, 51, 3)
    ones, zeros = torch.ones(40, 51, device="cuda"), torch.zeros(40, 51, device="cuda")
    for fn in (lambda p, **k: l1_ssim_loss(p, gt, 0.2, clamp_pred=True, **k), lambda p, **k: l1_loss(p, gt, 0.8, **k)):
        a, b, c = (base.clone().requires_grad_(True) for _ in range(3))
        la, lb, lc = fn(a), fn(b, mask=ones), fn(c, mask=zeros)
        assert abs(float(la) - float(lb)) < 1e-6
        assert float(lc) == 0.0
        for l_ in (la, lb, lc):
            l_.backward()
        assert torch.allclose(a.grad, b.grad, rtol=1e-6, atol=1e-9)
        assert float(c.grad.abs().max()) == 0.0
    _, l1, ss = l1_ssim_loss(base, gt, 0.2, return_terms=True, mask=zeros)
    assert float(l1) == 0.0 and abs(float(ss) - 1.0) < 1e-6
    depth = (base[..., :1] * 5).contiguous()
    alpha = gt[..., :1].contiguous()
    gtd = (gt[..., 1] * 4).contiguous()
    a, b = depth.clone().requires_grad_(True), depth.clone().requires_grad_(True)
    la, lb = depth_l1_loss(a, alpha, gtd), depth_l1_loss(b, alpha, gtd, mask=ones)
    assert abs(float(la) - float(lb)) < 1e-6
    la.backward()
    lb.backward()
    assert torch.allclose(a.grad, b.grad, rtol=1e-6, atol=1e-9)
    assert float(depth_l1_loss(depth, alpha, gtd, mask=zeros)) == 0.0


def test_mask_argument_forms_and_errors():
    import torch

    from gs_fused import L1SSIMLoss, depth_l1_loss, l1_loss, l1_ssim_loss

    gt, base, _ = _images(20, 23, 4)
    mb = torch.from_numpy(np.random.default_rng(0).uniform(0, 1, (20, 23)) > 0.4).cuda()
    mf = mb.to(torch.float32)

    def run(fn, mask):
        p = base.clone().requires_grad_(True)
        loss = fn(p, mask)
        loss.backward()
        return float(loss), p.grad

    heads = (lambda p, m: l1_ssim_loss(p, gt, 0.2, mask=m), lambda p, m: L1SSIMLoss(0.2)(p, gt, mask=m),
             lambda p, m: l1_loss(p, gt, 1.0, mask=m),
             lambda p, m: depth_l1_loss(p[..., :1].contiguous(), gt[..., :1].contiguous(), gt[..., 2].contiguous(), mask=m))
    for fn in heads:
        want, gwant = run(fn, mf)
        for other in (mb, mb.to(torch.uint8), mf[..., None], mb[..., None]):
            got, ggot = run(fn, other)
            assert got == want and torch.equal(ggot, gwant)
        with pytest.raises(ValueError):
            fn(base, mf[:-1])                # wrong shape
        with pytest.raises(ValueError):
            fn(base, mf[..., None, None])
        with pytest.raises(RuntimeError):
            fn(base, mf.cpu())               # wrong device
        with pytest.raises((ValueError, RuntimeError)):
            fn(base, mf.double())            # wrong dtype
        with pytest.raises((ValueError, RuntimeError)):
            fn(base, mf.to(torch.int32))
    assert not mf.requires_grad


def test_mask_none_is_the_unmasked_call():
    import torch

    from gs_fused import depth_l1_loss, l1_loss, l1_ssim_loss

    gt, base, _ = _images(20, 23, 6)
    p = base.clone().requires_grad_(True)
    a = l1_ssim_loss(p, gt, 0.2, clamp_pred=True, mask=None)
    b = l1_ssim_loss(base, gt, 0.2, clamp_pred=True)
    assert float(a) == float(b)
    a.backward()
    assert torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0
    assert float(l1_loss(base, gt, 0.8, mask=None)) == float(l1_loss(base, gt, 0.8))
    d, al, g = base[..., :1].contiguous(), gt[..., :1].contiguous(), gt[..., 2].contiguous()
    assert float(depth_l1_loss(d, al, g, mask=None)) == float(depth_l1_loss(d, al, g))
