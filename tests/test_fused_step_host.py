"""Pins tests/fused_step_reference.py -- the float64 references and float32 yardsticks the GPU edge tests of adam.hip,
activations.hip and the loss heads compare with -- on independent implementations, on the CPU: torch.optim.Adam and
torch autograd in float64, the double-precision SSIM oracle (oracle/gsr_oracle.c).  Also checks what the GPU tests
assume about their own inputs (tests/fused_step_cases.py)."""
import numpy as np
import pytest
import torch

import fused_step_cases as K
import fused_step_reference as R
from oracle import oracle as O

F32, F64 = np.float32, np.float64


def t64(a, grad=False):
    return torch.from_numpy(np.asarray(a, F64).copy()).requires_grad_(grad)


# ------------------------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize("betas,eps", [((0.9, 0.999), 1e-15), ((0.0, 0.9), 1e-8)])
def test_adam_f64_is_torch_adam_over_steps_and_from_a_loaded_state(betas, eps):
    p0, g0, m0, v0, _ = K.adam_elements(360, 3)
    rng = np.random.default_rng(0)
    lr = float(F32(1.6e-4))  # (the reference takes the learning rate as the float32 the C ABI carries)
    for start in (0, 29_999):  # from nothing; from a checkpoint's state
        p = torch.nn.Parameter(t64(p0))
        opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps)
        mine = (p0.astype(F64), None, np.zeros(360), np.zeros(360))
        if start:
            opt.state[p] = {"step": torch.tensor(float(start)), "exp_avg": t64(m0), "exp_avg_sq": t64(v0)}
            mine = (p0.astype(F64), None, m0.astype(F64), v0.astype(F64))
        for k in range(4):
            g = g0.astype(F64) * rng.uniform(0.5, 2.0, 360)
            p.grad = t64(g)
            opt.step()
            pn, mn, vn = R.adam_step(mine[0], g, mine[2], mine[3], start + k + 1, lr, betas, eps)
            mine = (pn, None, mn, vn)
        st = opt.state[p]
        assert float(st["step"]) == start + 4
        for a, b in ((mine[0], p.detach()), (mine[2], st["exp_avg"]), (mine[3], st["exp_avg_sq"])):
            b = b.numpy()
            assert np.all(np.abs(a - b) <= 1e-13 * np.abs(b) + 1e-300), np.abs(a - b).max()


def test_adam_yardstick_is_the_float32_oracle_bit_for_bit():
    p, g, m, v, _ = K.adam_elements(900, 5)
    for step, lr, eps in ((1, 1.6e-4, 1e-15), (30_000, 0.05, 1e-8)):
        lr = float(F32(lr))
        a = R.adam_step(p, g, m, v, step, lr, (0.9, 0.999), eps, dt=F32)
        with np.errstate(under="ignore"):
            b = O.adam_step(p, g, m, v, step, lr, eps=eps)
        for x, y in zip(a, b):
            assert x.dtype == F32 and np.array_equal(x.view(np.int32), y.view(np.int32))


def test_adam_cases_hold_every_class():
    p, g, m, v, cls = K.adam_elements(4099, 1)
    assert set(cls) == set(range(len(K.ADAM_CLASSES)))
    z = cls == K.ADAM_CLASSES.index("all_zero")
    assert not g[z].any() and not m[z].any() and not v[z].any()
    live = cls == K.ADAM_CLASSES.index("g_zero_live_state")
    assert not g[live].any() and (m[live] != 0).all() and (v[live] > 0).all()
    against = cls == K.ADAM_CLASSES.index("m_against_g")
    assert (np.sign(m[against]) == -np.sign(g[against])).all()
    a = np.abs(g[g != 0])
    assert a.min() < 1e-18 and a.max() > 1e2 and v.max() > 1e5
    assert (np.abs(p[cls == K.ADAM_CLASSES.index("p_below_one_step")]) < 1.6e-6).all()


# ----------------------------------------------------------------------------------------------------- activations
def test_activations_f64_are_torch_autograd():
    n = 240
    x = K.activation_inputs(n, 2)
    vs, vq, vo = K.activation_cotangents(x["raw_quats"], 3)
    ls, rq, lo = t64(x["log_scales"], True), t64(x["raw_quats"], True), t64(x["logits"], True)
    scales, quats, opac = torch.exp(ls), rq / rq.norm(dim=-1, keepdim=True), torch.sigmoid(lo)
    d = t64(x["means"]) - t64(x["campos"])
    dirs = d / d.norm(dim=-1, keepdim=True)
    got = R.activate_forward(x["means"], x["log_scales"], x["raw_quats"], x["logits"], x["campos"])
    for a, b in zip(got, (scales, quats, opac, dirs)):
        b = b.detach().numpy()
        assert np.all(np.abs(a - b) <= 1e-14 * np.abs(b) + 1e-300)
    (scales * t64(vs)).sum().backward()
    (quats * t64(vq)).sum().backward()
    (opac * t64(vo)).sum().backward()
    g_s, g_q, g_o = R.activate_vjp(x["log_scales"], x["raw_quats"], x["logits"], vs, vq, vo)
    assert np.all(np.abs(g_s - ls.grad.numpy()) <= 1e-14 * np.abs(g_s))
    # where v is parallel to q the difference cancels; both float64 evaluations carry 1e-16 of its TERMS
    assert np.all(np.abs(g_q - rq.grad.numpy()) <= 1e-7 * R.quat_grad_floor(x["raw_quats"], vq) + 1e-300)
    # torch's sigmoid backward: the same o (1 - o), o within an ulp64 -> a relative 1e-16 / (1 - o) at most
    o = got[2]
    assert np.all(np.abs(g_o - lo.grad.numpy()) <= 1e-15 * np.abs(vo.astype(F64)) * o + 1e-300)
    none = R.activate_vjp(x["log_scales"], x["raw_quats"], x["logits"], None, None, None)
    assert all(not a.any() for a in none)


def test_densify_stats_reference_is_the_masked_update():
    n = 41
    g, radii = K.densify_inputs(n, 4)
    vis = radii > 0
    norm = np.linalg.norm(g.astype(F64), axis=1)
    gn, cnt, mx = R.densify_stats(g, radii, 1920, np.full(n, np.nan), np.full(n, -7, np.int32), np.full(n, np.nan), True)
    inv = float(F32(1.0 / 1920.0))
    assert np.allclose(gn, norm, rtol=1e-15) and (cnt == 1).all()
    assert np.array_equal(mx, np.where(vis, radii * inv, 0.0))
    gn2, cnt2, mx2 = R.densify_stats(g, radii, 1920, gn, cnt, np.full(n, 0.01), False)
    assert np.allclose(gn2, np.where(vis, 2 * norm, norm), rtol=1e-15)
    assert np.array_equal(cnt2, 1 + vis) and np.array_equal(mx2, np.where(vis, np.maximum(0.01, radii * inv), 0.01))
    gn3, cnt3, _ = R.densify_stats(None, radii, 1920, gn2, cnt2, mx2, False)
    assert np.array_equal(gn3, gn2) and np.array_equal(cnt3, cnt2 + vis)
    assert not R.densify_stats(None, radii, 1920, gn2, cnt2, mx2, True)[0].any()


# ----------------------------------------------------------------------------------------------------- loss heads
@pytest.mark.parametrize("clamp,masked", [(False, False), (True, False), (False, True), (True, True)])
def test_l1_head_f64_is_torch_autograd(clamp, masked):
    pred, gt, mask = K.l1_case(5, 7, 6)
    p = t64(pred, True)
    x = torch.clamp(p, max=1.0) if clamp else p
    y = t64(gt)
    if masked:
        m = t64(mask)[..., None]
        x, y = x * m, y * m
    w, up = float(F32(0.8)), float(F32(1.7))  # (the head takes float32 factors)
    loss = w * torch.abs(y - x).mean()
    (loss * up).backward()
    got, g = R.l1_head(pred, gt, 0.8, clamp, mask if masked else None, upstream=1.7)
    assert abs(got - float(loss.detach())) <= 1e-15
    # torch's clamp passes the gradient at pred == 1 (`pred <= max`), and so does the head
    assert np.allclose(g, p.grad.numpy(), rtol=1e-14, atol=0)


@pytest.mark.parametrize("masked", [False, True])
def test_depth_head_f64_is_torch_autograd(masked):
    depth, alpha, gt, mask = K.depth_case(57, 8)
    d, a = t64(depth, True), t64(alpha, True)
    pred = torch.where(a > 0, d / torch.where(a > 0, a, torch.ones_like(a)), d.detach().max())
    g = t64(gt)
    if masked:
        g, pred = g * t64(mask), pred * t64(mask)
    hit = (g > 0).double()
    loss = torch.abs(g * hit - pred * hit).mean()
    (loss * float(F32(0.6))).backward()
    got, v_d, v_a = R.depth_head(depth, alpha, gt, mask if masked else None, upstream=0.6)
    assert abs(got - float(loss.detach())) <= 1e-14
    assert np.allclose(v_d, d.grad.numpy().reshape(-1), rtol=1e-14, atol=0)
    assert np.allclose(v_a, a.grad.numpy().reshape(-1), rtol=1e-14, atol=0)
    assert not v_d[alpha.reshape(-1) == 0].any() and not v_d[gt.reshape(-1) == 0].any()


SSIM_CASES = K.ssim_cases()


def test_ssim_cases_cover_the_sizes_and_cap_the_near_ties():
    assert {c["pred"].shape[:2] for c in SSIM_CASES} == set(K.SSIM_SIZES)
    assert {c["lam"] for c in SSIM_CASES} == {0.0, 0.2, 1.0} and any(c["up"] != 1.0 for c in SSIM_CASES)
    for c in SSIM_CASES:
        share = float(K.near_tie(c["pred"], c["gt"], c["clamp"]).mean())
        if c["equal"]:
            assert np.array_equal(c["pred"], c["gt"])
        else:
            assert share < 0.01, (c["name"], share)
    over = [c for c in SSIM_CASES if c["name"].startswith("over_one")]
    assert {c["clamp"] for c in over} == {False, True}
    assert all((c["pred"] == 1.0).any() and c["pred"].max() > 1.39 for c in over)
    assert any(c["pred"].min() < 0 for c in SSIM_CASES)


@pytest.mark.parametrize("case", SSIM_CASES, ids=[c["name"] for c in SSIM_CASES])
def test_ssim_reference_and_yardstick_against_the_oracle(case):
    """The separable float64 restatement equals the oracle's direct 121-tap double sums; the float32 restatement is
    within the SSIM gradient floor of the GPU test (32 eps32 sum |terms|) of it at every pixel, and its three scalars
    within a few float32 roundings of the oracle's doubles."""
    pred, gt, lam, clamp, up = case["pred"], case["gt"], case["lam"], case["clamp"], case["up"]
    x = np.minimum(pred, F32(1)) if clamp else pred
    loss, l1, ssim, v = O.l1_ssim_loss(x, gt, lam)  # the oracle knows neither the clamp nor an upstream factor
    up = float(F32(up))
    v = up * np.where((pred > 1) & clamp, 0.0, v.astype(F64))
    r_loss, r_l1, r_ssim, r_v, terms = R.l1_ssim(pred, gt, lam, clamp, up, with_terms=True)
    assert abs(r_l1 - l1) <= 1e-14 and abs(r_ssim - ssim) <= 1e-12 and abs(r_loss - loss) <= 1e-12
    keep = ~K.near_tie(pred, gt, clamp)
    # (the oracle hands its gradient out as float32)
    assert np.all(np.abs(r_v - v)[keep] <= (abs(up) * R.ulp32(v / up) + 1e-12 * terms)[keep])
    y_loss, y_l1, y_ssim, y_v = R.l1_ssim(pred, gt, lam, clamp, up, dt=F32)
    assert y_v.dtype == F32
    floor = 32 * R.EPS32 * terms
    worst = float((np.abs(y_v - r_v)[keep] / np.maximum(floor[keep], 1e-300)).max()) if keep.any() else 0.0
    print(f"{case['name']}: float32 yardstick at {worst:.3f} of the gradient floor; ssim off by {abs(y_ssim - ssim):.2e}")
    assert worst <= 1.0
    assert abs(y_l1 - l1) <= 4 * R.EPS32 * max(l1, 1e-30)
    # a sanity cap on the yardstick's own SSIM mean, not a bound on anything: it is 6.5e-6 off at the most (blob_0.3),
    # and a mistake in the float32 restatement (a wrong tap, a swapped constant) would move it by 1e-3 and more
    assert abs(y_ssim - ssim) <= 1e-4
