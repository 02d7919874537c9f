"""CPU: the float64 SH reference (tests/sh_reference.py) pinned before the HIP kernels are held to it
(test_gpu_sh.py).

1. The 25 basis functions are orthonormal on the sphere, by exact quadrature: Gauss-Legendre in z times a uniform
   grid in phi integrates every product of two functions of degree <= 4 (a polynomial of degree <= 8) exactly.  This
   proves band constants and signs without trusting any other file of the repository.
2. The reference agrees with the float32 oracle and with the SH goldens of the reference implementation, and the
   oracle's worst error in units of 2^-24 S (S: the element's conditioning sum, sh_reference.py) is measured on the
   inputs the GPU tests use and pinned: sh_reference.R_FWD / R_BWD.  Measured: r_fwd = 7.75 (degree 4),
   r_bwd = 4.755e4.  r_bwd is that large because |B_k| |v| does not see the cancellation inside a basis function
   (xx - yy, 3 xx - yy, ...: float32 loses |xx| + |yy| there, whatever is left of the difference), so the backward
   is also measured in units of A_k |v|, A_k the sum of the absolute monomials of B_k: r_bwd_cond = 8.84.  The GPU
   tests hold the kernels to four times each of the three.
3. The reference does not observe what the contract says is unused: poisoned bands above `use`, and a poisoned
   direction at use == 0, leave every result bit for bit the same.
4. The clamp test of test_gpu_sh.py excludes colours within the tolerance of 0; on its seeded inputs that is at most
   1 % of the channels.
"""
import os

import numpy as np
import pytest

import sh_reference as R
from oracle import oracle as O

DEGREES = [0, 1, 2, 3, 4]


def test_basis_is_orthonormal_on_the_sphere():
    zn, zw = np.polynomial.legendre.leggauss(8)  # exact to degree 15 in z
    nphi = 16                                     # exact for e^{i m phi}, |m| <= 15
    phi = np.arange(nphi) * (2 * np.pi / nphi)
    Z, P = np.meshgrid(zn, phi, indexing="ij")
    W = np.repeat(zw[:, None], nphi, 1) * (2 * np.pi / nphi)
    s = np.sqrt(1 - Z * Z)
    B, A = R.basis_unit(4, (s * np.cos(P)).ravel(), (s * np.sin(P)).ravel(), Z.ravel())
    gram = (B * W.ravel()[:, None]).T @ B
    assert np.abs(gram - np.eye(25)).max() < 1e-12
    assert np.all(A >= np.abs(B) * (1 - 1e-15))


def test_sign_convention_is_svox2():
    """degree 1 is (-y, z, -x) times sqrt(3 / 4 pi), the DC term is 1 / (2 sqrt(pi))."""
    B, _ = R.basis(1, 1, np.array([[0.0, 2.0, 0.0], [0.0, 0.0, 3.0], [0.5, 0.0, 0.0]]))
    c1 = np.sqrt(3 / (4 * np.pi))
    np.testing.assert_allclose(B, [[0.5 / np.sqrt(np.pi), -c1, 0, 0], [0.5 / np.sqrt(np.pi), 0, c1, 0],
                                   [0.5 / np.sqrt(np.pi), 0, 0, -c1]], rtol=1e-15, atol=1e-16)


def _ratios(deg, use, dirs, coeffs, v):
    n = len(dirs)
    ref, S = R.forward(deg, use, dirs, coeffs)
    got = O.compute_sh_forward(n, deg, use, dirs, coeffs)
    assert np.all(S > 0) and np.all(np.isfinite(got))
    rf = (np.abs(got - ref) / (R.U * S)).max()
    g, b, a = R.backward(deg, use, dirs, v)
    gotb = O.compute_sh_backward(n, deg, use, dirs, v)
    on = b > 0
    assert np.all(gotb[~on] == 0) and np.all(np.isfinite(gotb))
    assert not on[:, R.num_bases(use):].any() and np.all(g[:, R.num_bases(use):] == 0)
    e = np.abs(gotb - g)[on]
    return rf, (e / (R.U * b[on])).max(), (e / (R.U * a[on])).max()


def test_oracle_error_in_units_of_conditioning(golden_dir):
    """The oracle (float32, the same sums) against float64 on the inputs of the GPU tests and on the goldens' inputs:
    its worst ratio is what sh_reference.R_* record (rounded up); the GPU tolerances are 4 x those."""
    g = dict(np.load(os.path.join(golden_dir, "sh.npz")))
    worst = np.zeros(3)
    for deg in DEGREES:
        for use in range(deg + 1):
            for n in R.SIZES:
                I = R.make_inputs(deg, n)
                worst = np.maximum(worst, _ratios(deg, use, I["dirs"], I["coeffs"], I["v"]))
            worst = np.maximum(worst, _ratios(deg, use, g["viewdirs"], g[f"coeffs{deg}"], g[f"v_colors{deg}"]))
    print(f"oracle vs float64: r_fwd {worst[0]:.4g}, r_bwd {worst[1]:.4g}, r_bwd_cond {worst[2]:.4g}")
    for got, rec in zip(worst, (R.R_FWD, R.R_BWD, R.R_BWD_COND)):
        assert 0.95 * rec <= got <= rec, (got, rec)
    assert (R.TOL_FWD, R.TOL_BWD, R.TOL_BWD_COND) == (4 * R.R_FWD, 4 * R.R_BWD, 4 * R.R_BWD_COND)


@pytest.mark.parametrize("deg", DEGREES)
def test_reference_agrees_with_the_goldens(golden_dir, deg):
    """The goldens are float32 results of the reference implementation's own PyTorch code: within the tolerance the
    GPU kernels get."""
    g = dict(np.load(os.path.join(golden_dir, "sh.npz")))
    ref, S = R.forward(deg, deg, g["viewdirs"], g[f"coeffs{deg}"])
    assert np.all(np.abs(g[f"colors{deg}"] - ref) <= R.TOL_FWD * R.U * S)
    gr, b, a = R.backward(deg, deg, g["viewdirs"], g[f"v_colors{deg}"])
    assert np.all(np.abs(g[f"g_coeffs{deg}"] - gr) <= R.TOL_BWD_COND * R.U * a)


def test_heavy_cancellation_rows_exist():
    """the bound is exercised, not an absolute epsilon: on the tuned rows S exceeds |colour| by 1e4 and more"""
    for deg in (1, 2, 3, 4):
        I = R.make_inputs(deg, 257)
        for use in range(1, deg + 1):
            rows = [i for i in range(1, 257, 4) if 1 + (i // 4) % deg == use]
            col, S = R.forward(deg, use, I["dirs"][rows], I["coeffs"][rows])
            assert np.all(S > 1e4 * np.abs(col))
    d = np.linalg.norm(R.make_inputs(3, 4097)["dirs"].astype(np.float64), axis=1)
    assert d.min() < 1e-2 and d.max() > 1e2


@pytest.mark.parametrize("deg", DEGREES)
def test_reference_ignores_unused_bands_and_direction(deg):
    n = 65
    I = R.make_inputs(deg, n)
    for use in range(deg + 1):
        ku = R.num_bases(use)
        dirs = I["dirs"]
        if use == 0:
            dirs = dirs.copy()
            dirs[0::2] = np.nan
            dirs[1::2] = 0
        want = R.forward(deg, use, I["dirs"], I["coeffs"])
        got = R.forward(deg, use, dirs, R.poison(I["coeffs"], ku))
        assert all(np.array_equal(a, b) for a, b in zip(want, got)) and np.all(np.isfinite(got[0]))
        dc, rest = I["coeffs"][:, 0], I["coeffs"][:, 1:]
        want = R.split_forward(deg, use, I["dirs"], dc, rest, 0.5, True)
        got = R.split_forward(deg, use, dirs, dc, R.poison(rest, ku - 1), 0.5, True)
        assert all(np.array_equal(a, b) for a, b in zip(want, got))
        assert np.array_equal(want[0], np.maximum(R.forward(deg, use, I["dirs"], I["coeffs"], 0.5)[0], 0))
        want = R.backward(deg, use, I["dirs"], I["v"])
        got = R.backward(deg, use, dirs, I["v"])
        assert all(np.array_equal(a, b) for a, b in zip(want, got)) and np.all(got[0][:, ku:] == 0)
    if deg <= 3:
        means, msg = R.make_view_inputs(deg, n, 3)
        means = means.copy()
        means[5] = msg[1, 3 * n:]  # a Gaussian exactly at a camera position
        out, bound, _ = R.views_backward(deg, 0, means, msg[:, 3 * n:], msg[:, :3 * n].reshape(3, n, 3), 0.25)
        assert np.all(np.isfinite(out)) and np.all(out[:, 1:] == 0)
        np.testing.assert_allclose(out[:, 0], 0.25 * R.basis(0, 0, None, 1)[0][0, 0]
                                   * msg[:, :3 * n].reshape(3, n, 3).astype(np.float64).sum(0), rtol=1e-12, atol=1e-15)


def test_views_backward_is_the_sum_of_single_views():
    deg, n, V = 3, 63, 3
    means, msg = R.make_view_inputs(deg, n, V)
    campos, v = msg[:, 3 * n:], msg[:, :3 * n].reshape(V, n, 3)
    for use in range(deg + 1):
        want = sum(R.backward(deg, use, means.astype(np.float64) - campos[r].astype(np.float64), v[r])[0] for r in range(V))
        got, bound, cond = R.views_backward(deg, use, means, campos, v, 0.5)
        np.testing.assert_allclose(got, 0.5 * want, rtol=1e-15, atol=0)
        assert np.all(bound >= np.abs(got) * (1 - 1e-12)) and np.all(cond >= bound * (1 - 1e-12))


@pytest.mark.parametrize("deg", [1, 2, 3])
def test_clamp_exclusion_share(deg):
    """Channels whose float64 colour lies within the float32 tolerance of 0 (sign undecided): at most 1 %; and the
    inputs do put colours on both sides of the cut."""
    for n in R.SIZES:
        dirs, dc, rest, v = R.make_clamp_inputs(deg, n)
        for use in range(deg + 1):
            col, S = R.forward(deg, use, dirs, np.concatenate([dc[:, None], rest], 1), 0.5)
            undecided = np.abs(col) <= R.TOL_FWD * R.U * S
            assert undecided.mean() <= 0.01
            if n >= 63:
                assert 0.05 < (col < 0).mean() < 0.95
