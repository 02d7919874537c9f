"""Host: the float64 restatement of the co-gs depth regularisation (tests/depth_reg_reference.py) against the values
the reference's own code produced (tests/golden/depth_reg.npz: torch CPU float32, `torch.autograd`), its gradient
formula against central differences, and the measurement of the reference's own float32 error that the GPU test's
tolerances are built on."""
import os

import numpy as np
import pytest

import depth_reg_reference as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_reg.npz")
# measured by test_reference_float32_error_is_what_the_gpu_tolerances_assume (recomputed there on every run)
R_LOSS, R_GRAD = 6.30e-8, 1.82e-7


def _cases():
    z = np.load(GOLDEN)
    return [(str(c), z[f"{c}_pred"], z[f"{c}_mask"], float(z[f"{c}_loss"]), z[f"{c}_grad"]) for c in z["cases"]]


def reference_errors():
    """-> (r_loss, r_grad): the largest |L_ref32 - L64| / L64 and |grad_ref32 - grad64| / max |grad64| over the
    fixtures (a case whose float64 value is 0 enters with its absolute error)."""
    r_loss = r_grad = 0.0
    for name, pred, mask, loss32, grad32 in _cases():
        loss, grad = D.depth_reg(pred, mask)
        r_loss = max(r_loss, abs(loss32 - loss) / (loss if loss > 0 else 1.0))
        top = np.abs(grad).max()
        r_grad = max(r_grad, float(np.abs(grad32 - grad).max() / (top if top > 0 else 1.0)))
    return r_loss, r_grad


def test_fixture_holds_the_cases_the_kernels_are_asked():
    cases = {c[0]: c for c in _cases()}
    assert set(cases) == {"canny_24x40", "canny_11x13", "random_24x40", "random_11x13", "dead_11x13", "nomask_24x40"}
    for name, pred, mask, loss32, grad32 in cases.values():
        assert pred.dtype == mask.dtype == grad32.dtype == np.float32 and pred.shape == mask.shape == grad32.shape
        assert set(np.unique(mask)) <= {0.0, 1.0}
    for name in ("canny_24x40", "random_24x40"):
        assert 0.05 < (cases[name][1] <= 0).mean() < 0.2       # about 10 % of the depths are not positive
    assert 0 < cases["canny_24x40"][2].mean() < 1 and 0 < cases["canny_11x13"][2].mean() < 1
    assert (cases["dead_11x13"][1] <= 0).all() and cases["dead_11x13"][3] == 0.0 and not cases["dead_11x13"][4].any()
    assert not cases["nomask_24x40"][2].any() and cases["nomask_24x40"][3] > 0
    assert os.path.getsize(GOLDEN) < 64 * 1024


def test_restatement_equals_what_the_references_code_produced():
    for name, pred, mask, loss32, grad32 in _cases():
        loss, grad = D.depth_reg(pred, mask)
        assert loss32 == pytest.approx(loss, rel=1e-6, abs=1e-12), name
        assert np.abs(grad32 - grad).max() <= 1e-6 * max(np.abs(grad).max(), 1e-30), name


def test_reference_float32_error_is_what_the_gpu_tolerances_assume():
    r_loss, r_grad = reference_errors()
    print(f"r_loss {r_loss:.3e}  r_grad {r_grad:.3e}  (2^-24 = {2.0 ** -24:.3e})")
    assert r_loss == pytest.approx(R_LOSS, rel=0.01) and r_grad == pytest.approx(R_GRAD, rel=0.01)


@pytest.mark.parametrize("name", ["random_11x13", "canny_11x13"])
def test_gradient_formula_against_central_differences(name):
    _, pred, mask, _, _ = {c[0]: c for c in _cases()}[name]
    pred = pred.astype(np.float64)
    _, grad = D.depth_reg(pred, mask)
    h = 1e-5
    worst, checked = 0.0, 0
    for i in np.ndindex(pred.shape):
        if abs(pred[i]) <= h:
            continue  # (the step would cross pred = 0, where the loss jumps: `pred > 0` is a constant)
        up, down = pred.copy(), pred.copy()
        up[i] += h
        down[i] -= h
        worst = max(worst, abs((D.depth_reg(up, mask)[0] - D.depth_reg(down, mask)[0]) / (2 * h) - grad[i]))
        checked += 1
    assert checked > 0.8 * pred.size and (pred <= 0).any()
    assert worst <= 1e-7 * np.abs(grad).max(), worst / np.abs(grad).max()   # (measured: 4e-10; h^2 truncation + cancellation)


def test_edge_shapes_and_padding():
    # a single pixel: near = pred * m / (m + 1e-8)
    loss, grad = D.depth_reg(np.array([[2.0]]), np.array([[1.0]]))
    assert loss == pytest.approx((2.0 / (1 + 1e-8) - 2.0) ** 2) and grad.shape == (1, 1)
    # constant positive depth, full mask: near = pred everywhere whatever the tap count at the border -> loss ~ 0
    loss, grad = D.depth_reg(np.full((5, 7), 3.0), np.ones((5, 7)))
    assert loss < 1e-14
    # mask 0 everywhere: near = 0, loss = mean pred^2 over the positive pixels
    p = np.array([[1.0, -2.0], [3.0, 0.0]])
    loss, grad = D.depth_reg(p, np.zeros((2, 2)))
    assert loss == pytest.approx((1 + 9) / 4) and np.allclose(grad, 2 * np.where(p > 0, p, 0) / 4)
