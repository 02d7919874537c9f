"""Host: the float64 restatement of the three monocular-depth terms of the co-gs loss (tests/mono_depth_reference.py)
against the values the reference's own code produced (tests/golden/cogs_losses.npz, cases c0-c2: torch CPU float32), its
gradient formulas against central differences and against float64 autograd of `harness.cogs_losses`, the NaN patterns
the heads must reproduce, and the measurement the GPU tests' tolerances are built on: the error
of `harness.cogs_losses` run in float32 on the CPU against the restatement over the three golden cases, losses relative,
gradients relative to the largest float64 entry.  Measured (recomputed on every run):

    term            r_loss     r_grad
    local Pearson   5.04e-8    2.74e-7
    log-depth       8.72e-8    3.22e-7
    TV              3.51e-8    4.54e-8
"""
import os

import numpy as np
import pytest
import torch

import mono_depth_reference as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cogs_losses.npz")
CASES = ("c0", "c1", "c2")
# measured by test_reference_float32_error_is_what_the_gpu_tolerances_assume (recomputed there on every run)
R = {"local_pearson": (5.04e-8, 2.74e-7), "log_depth": (8.72e-8, 3.22e-7), "tv": (3.51e-8, 4.54e-8)}


def _case(c):
    z = np.load(GOLDEN)
    return {k[len(c) + 1:]: z[k] for k in z.files if k.startswith(c + "_")}


def _terms64(d):
    """The restatement's (loss, gradient) of the three terms on one golden case."""
    box = int(d["box_pcorr"][0])
    return {"local_pearson": M.local_pearson(d["pred"], d["gt"], box, d["patch_rows"], d["patch_cols"]),
            "log_depth": M.log_depth(d["pred"], d["gt"], d["img"], *d["scale_shift"]),
            "tv": M.tv(d["pred"])}


def _torch_terms(d, dtype):
    """`harness.cogs_losses` on one golden case in `dtype` on the CPU -> {term: (loss, gradient)} as float64."""
    from harness import cogs_losses as CL

    box = int(d["box_pcorr"][0])
    gt, img = torch.from_numpy(d["gt"]).to(dtype), torch.from_numpy(d["img"]).to(dtype)
    corners = (torch.from_numpy(d["patch_rows"]), torch.from_numpy(d["patch_cols"]))
    scale, shift = (float(v) for v in d["scale_shift"])
    fns = {"local_pearson": lambda p: CL.local_pearson_loss(p, gt, box, 0.5, corners=corners),
           "log_depth": lambda p: CL.scaled_log_depth_loss(p, gt, img, scale, shift),
           "tv": CL.tv_loss}
    out = {}
    for name, fn in fns.items():
        p = torch.from_numpy(d["pred"]).to(dtype).requires_grad_(True)
        loss = fn(p)
        loss.backward()
        out[name] = (float(loss.detach()), p.grad.double().numpy())
    return out


def reference_errors():
    """-> {term: (r_loss, r_grad)} over the golden cases."""
    r = {k: [0.0, 0.0] for k in R}
    for c in CASES:
        d = _case(c)
        want, got = _terms64(d), _torch_terms(d, torch.float32)
        for k in R:
            r[k][0] = max(r[k][0], abs(got[k][0] - want[k][0]) / abs(want[k][0]))
            r[k][1] = max(r[k][1], float(np.abs(got[k][1] - want[k][1]).max() / np.abs(want[k][1]).max()))
    return {k: tuple(v) for k, v in r.items()}


def test_the_heads_exist_and_have_no_cpu_path():
    import gs_fused

    p, img = torch.ones(4, 5), torch.ones(4, 5, 3)
    idx = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        gs_fused.local_pearson_loss(p, p, 2, idx, idx)
    with pytest.raises(RuntimeError):
        gs_fused.log_depth_loss(p, p, img)
    with pytest.raises(RuntimeError):
        gs_fused.tv_loss(p)
    from harness import cogs_losses as CL

    class Cfg:
        use_pearson_depth = use_scaled_est_depth = use_depth_regularization = False
        using_tv_loss = True
        local_patch_size, depth_loss_stop_iteration = 2, 100

    assert set(CL.optional_depth_terms(Cfg, 0, p, p, img)) == {"tv_loss"}       # fused=False: as before, on the CPU
    with pytest.raises(RuntimeError):
        CL.optional_depth_terms(Cfg, 0, p, p, img, fused=True)                   # no quiet fall-back
    with pytest.raises(ValueError):
        CL.optional_depth_terms(Cfg, 0, p, p, img, mask=torch.ones(4, 5))


def test_restatement_equals_what_the_references_code_produced():
    for c in CASES:
        d = _case(c)
        t = _terms64(d)
        assert t["local_pearson"][0] == pytest.approx(float(d["local_pearson"]), rel=1e-6), c
        assert t["log_depth"][0] == pytest.approx(float(d["log_depth"]), rel=1e-6), c
        assert t["tv"][0] == pytest.approx(float(d["tv"]), rel=1e-6), c
        box = int(d["box_pcorr"][0])
        loop = M.local_pearson_loop(d["pred"], d["gt"], box, d["patch_rows"], d["patch_cols"])
        assert t["local_pearson"][0] == pytest.approx(loop, rel=1e-13), c    # closed form against the literal loop
        assert len(d["patch_rows"]) == int(d["box_pcorr"][1] * (d["pred"].shape[0] // box) * (d["pred"].shape[1] // box))


def test_reference_float32_error_is_what_the_gpu_tolerances_assume():
    r = reference_errors()
    for k, (r_loss, r_grad) in r.items():
        print(f"{k}: r_loss {r_loss:.3e}  r_grad {r_grad:.3e}  (2^-24 = {2.0 ** -24:.3e})")
    for k, (r_loss, r_grad) in r.items():
        assert r_loss == pytest.approx(R[k][0], rel=0.01) and r_grad == pytest.approx(R[k][1], rel=0.01), k


def test_gradients_equal_float64_autograd_of_the_torch_restatement():
    for c in CASES:
        d = _case(c)
        want, got = _terms64(d), _torch_terms(d, torch.float64)
        for k in R:
            assert got[k][0] == pytest.approx(want[k][0], rel=1e-13), (c, k)
            assert np.abs(got[k][1] - want[k][1]).max() <= 1e-13 * np.abs(want[k][1]).max(), (c, k)


def _small():
    pred, gt, img = M.smooth_noise(12, 14, 3)
    rows, cols = np.array([0, 3, 8, 3, 5]), np.array([0, 2, 10, 2, 6])   # overlapping, one twice, the last valid corner
    return pred.astype(np.float64), gt.astype(np.float64), img, rows, cols


@pytest.mark.parametrize("masked", [False, True])
def test_gradient_formulas_against_central_differences(masked):
    pred, gt, img, rows, cols = _small()
    mask = None
    if masked:
        mask = np.random.default_rng(5).uniform(0.2, 1.5, pred.shape)
    # (float64 throughout: here the products are formed in float64, which `products` would round to float32)
    at = (lambda p: p) if mask is None else (lambda p: p * mask)
    g_ = gt if mask is None else gt * mask
    fns = {"local_pearson": lambda p: M.local_pearson(at(p), g_, 4, rows, cols, mask),
           "log_depth": lambda p: M.log_depth(at(p), g_, img, 0.9, 0.15, mask),
           "tv": lambda p: M.tv(at(p), mask)}
    h = 1e-6
    for name, fn in fns.items():
        _, grad = fn(pred)
        worst = 0.0
        for i in np.ndindex(pred.shape):
            up, down = pred.copy(), pred.copy()
            up[i] += h
            down[i] -= h
            worst = max(worst, abs((fn(up)[0] - fn(down)[0]) / (2 * h) - grad[i]))
        # h^2 truncation + cancellation in losses of ~1; no |.| changes sign within h (smooth + noise)
        assert worst <= 1e-7 * np.abs(grad).max(), (name, worst / np.abs(grad).max())


def test_nan_patterns():
    pred, gt, img, _, _ = _small()
    # no patches: 0 / 0
    loss, grad = M.local_pearson(pred, gt, 4, np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert np.isnan(loss) and np.isnan(M.local_pearson_loop(pred, gt, 4, [], []))
    # one constant 8x8 patch among others: NaN on exactly its 64 pixels, as float64 autograd of the torch restatement
    from harness import cogs_losses as CL

    p, g, _ = M.smooth_noise(24, 24, 4)
    p = p.astype(np.float64)
    p[2:10, 3:11] = 2.5
    rows, cols = np.array([2, 14]), np.array([3, 12])
    loss, grad = M.local_pearson(p, g, 8, rows, cols)
    assert np.isnan(loss) and np.isnan(grad).sum() == 64 and np.isnan(grad[2:10, 3:11]).all()
    outside = np.ones((24, 24), bool)
    outside[2:10, 3:11] = outside[14:22, 12:20] = False
    assert (grad[14:22, 12:20] != 0).all() and not grad[outside].any()
    tp = torch.from_numpy(p).requires_grad_(True)
    CL.local_pearson_loss(tp, torch.from_numpy(g).double(), 8, 0.5,
                          corners=(torch.from_numpy(rows), torch.from_numpy(cols))).backward()
    auto = tp.grad.numpy()
    assert np.array_equal(np.isnan(auto), np.isnan(grad))
    assert np.abs(auto - grad)[np.isfinite(grad)].max() <= 1e-13 * np.abs(grad[np.isfinite(grad)]).max()
    # a constant TARGET patch: the same pattern
    g2 = g.astype(np.float64)
    g2[14:22, 12:20] = 1.0
    loss, grad = M.local_pearson(M.smooth_noise(24, 24, 4)[0], g2, 8, rows[1:], cols[1:])
    assert np.isnan(loss) and np.isnan(grad).sum() == 64 and np.isnan(grad[14:22, 12:20]).all()
    # box 1: n - 1 = 0
    loss, grad = M.local_pearson(pred, gt, 1, np.array([3]), np.array([4]))
    assert np.isnan(loss) and np.isnan(grad).sum() == 1 and np.isnan(grad[3, 4])
    # a corner outside the image: NaN loss, nothing else
    loss, grad = M.local_pearson(pred, gt, 4, np.array([0, 9, -1]), np.array([0, 5, 2]))
    assert np.isnan(loss) and np.isfinite(grad).all() and (grad[4:] == 0).all() and (grad[:4, :4] != 0).all()
    # one row / one column: the mean of an empty tensor
    assert np.isnan(M.tv(pred[:1])[0]) and np.isnan(M.tv(pred[:, :1])[0])
    assert np.isnan(M.log_depth(pred[:1], gt[:1], img[:1])[0]) and np.isnan(M.log_depth(pred[:, :1], gt[:, :1], img[:, :1])[0])
    assert np.isfinite(M.tv(pred[:1])[1]).all() and np.isfinite(M.log_depth(pred[:1], gt[:1], img[:1])[1]).all()
    assert np.isnan(float(CL.tv_loss(torch.ones(1, 5)))) and np.isnan(float(CL.tv_loss(torch.ones(5, 1))))


def test_exact_ties_have_gradient_zero():
    pred, gt, img, _, _ = _small()
    pred[4, 5] = pred[4, 6] = pred[5, 5]          # equal neighbours: sign(0) = 0
    _, grad = M.tv(pred)
    base = M.tv(pred)[1]
    assert np.isfinite(base).all()
    flat = np.full((3, 3), 2.0)
    assert not M.tv(flat)[1].any() and M.tv(flat)[0] == 0.0
    gt2 = gt.copy()
    gt2[7, 3] = 0.9 * pred[7, 3] + 0.15           # pred == gt after scale and shift
    e = 0.9 * pred[7, 3] + 0.15 - gt2[7, 3]
    assert e == 0.0
    _, grad = M.log_depth(pred, gt2, img, 0.9, 0.15)
    assert grad[7, 3] == 0.0 and (grad[:-1, :-1] != 0).sum() == grad[:-1, :-1].size - 1
