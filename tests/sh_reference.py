"""Float64 NumPy reference of the SH colour operations of csrc/sh.hip -- the yardstick of test_sh_host.py and
test_gpu_sh.py -- plus the seeded inputs those tests share.  A helper module, not a test.

Independent of sh.hip and of oracle/gsr_oracle.c: the band constants are built from their closed forms, every basis
function is a table of monomials in the unit direction (x, y, z), svox2 sign convention, coefficient layout
[n, K, 3] with K = (degree + 1)^2.  test_sh_host.py proves constants and signs by quadrature (orthonormality of the
25 functions on the sphere) before anything is held to this file.

What is observed: only the bands k < (use + 1)^2 of the coefficients, and the direction only when use >= 1.  The
unused bands and (at use == 0) the direction may hold anything.

Error budget: every function returns, next to its result, the conditioning sum of each output element: the sum of the
absolute values of the terms float32 has to add up,  S = sum_k |B_k| |c_k| (+ |shift|)  for a colour and  |B_k| |v|
(summed over the views, times |scale|) for a gradient element.  A float32 implementation is judged in units of
2^-24 S of the element's own S.
"""
import functools
import math

import numpy as np

U = 2.0 ** -24  # unit round-off of float32

# measured by test_sh_host.py::test_oracle_error_in_units_of_conditioning (the float32 oracle doing the same sums on
# the shared inputs below, worst element over all degrees, `use` and sizes) and pinned there; the GPU tests allow
# four times as much (test_gpu_sh.py header)
R_FWD = 7.8
R_BWD = 4.76e4
R_BWD_COND = 8.9
TOL_FWD, TOL_BWD, TOL_BWD_COND = 4 * R_FWD, 4 * R_BWD, 4 * R_BWD_COND

SIZES = (1, 63, 64, 65, 255, 256, 257, 4097)  # wave boundary +-1, workgroup boundary +-1, one ragged multi-workgroup


def num_bases(degree):
    return (degree + 1) ** 2


_pi = math.pi
_C = (
    [0.5 * math.sqrt(1 / _pi)],
    [-math.sqrt(3 / (4 * _pi)), math.sqrt(3 / (4 * _pi)), -math.sqrt(3 / (4 * _pi))],
    [0.5 * math.sqrt(15 / _pi), -0.5 * math.sqrt(15 / _pi), 0.25 * math.sqrt(5 / _pi), -0.5 * math.sqrt(15 / _pi),
     0.25 * math.sqrt(15 / _pi)],
    [-0.25 * math.sqrt(35 / (2 * _pi)), 0.5 * math.sqrt(105 / _pi), -0.25 * math.sqrt(21 / (2 * _pi)),
     0.25 * math.sqrt(7 / _pi), -0.25 * math.sqrt(21 / (2 * _pi)), 0.25 * math.sqrt(105 / _pi),
     -0.25 * math.sqrt(35 / (2 * _pi))],
    [0.75 * math.sqrt(35 / _pi), -0.75 * math.sqrt(35 / (2 * _pi)), 0.75 * math.sqrt(5 / _pi),
     -0.75 * math.sqrt(5 / (2 * _pi)), 3 / 16 * math.sqrt(1 / _pi), -0.75 * math.sqrt(5 / (2 * _pi)),
     3 / 8 * math.sqrt(5 / _pi), -0.75 * math.sqrt(35 / (2 * _pi)), 3 / 16 * math.sqrt(35 / _pi)],
)
# polynomial of each basis function on the unit sphere: [(factor, (px, py, pz)), ...], times the band constant
_POLY = (
    [[(1, (0, 0, 0))]],
    [[(1, (0, 1, 0))], [(1, (0, 0, 1))], [(1, (1, 0, 0))]],
    [[(1, (1, 1, 0))], [(1, (0, 1, 1))], [(2, (0, 0, 2)), (-1, (2, 0, 0)), (-1, (0, 2, 0))], [(1, (1, 0, 1))],
     [(1, (2, 0, 0)), (-1, (0, 2, 0))]],
    [[(3, (2, 1, 0)), (-1, (0, 3, 0))], [(1, (1, 1, 1))], [(4, (0, 1, 2)), (-1, (2, 1, 0)), (-1, (0, 3, 0))],
     [(2, (0, 0, 3)), (-3, (2, 0, 1)), (-3, (0, 2, 1))], [(4, (1, 0, 2)), (-1, (3, 0, 0)), (-1, (1, 2, 0))],
     [(1, (2, 0, 1)), (-1, (0, 2, 1))], [(1, (3, 0, 0)), (-3, (1, 2, 0))]],
    [[(1, (3, 1, 0)), (-1, (1, 3, 0))], [(3, (2, 1, 1)), (-1, (0, 3, 1))], [(7, (1, 1, 2)), (-1, (1, 1, 0))],
     [(7, (0, 1, 3)), (-3, (0, 1, 1))], [(35, (0, 0, 4)), (-30, (0, 0, 2)), (3, (0, 0, 0))],
     [(7, (1, 0, 3)), (-3, (1, 0, 1))], [(7, (2, 0, 2)), (-1, (2, 0, 0)), (-7, (0, 2, 2)), (1, (0, 2, 0))],
     [(1, (3, 0, 1)), (-3, (1, 2, 1))], [(1, (4, 0, 0)), (-6, (2, 2, 0)), (1, (0, 4, 0))]],
)


def basis_unit(deg, x, y, z):
    """-> (B, A) [..., (deg+1)^2] float64 at unit directions: the basis values and, per function, the sum of the
    absolute values of its monomials (the basis function's own conditioning)."""
    x, y, z = (np.asarray(t, np.float64) for t in (x, y, z))
    B = np.empty(x.shape + (num_bases(deg),), np.float64)
    A = np.empty_like(B)
    k = 0
    for band in range(deg + 1):
        for c, poly in zip(_C[band], _POLY[band]):
            terms = [f * x ** px * y ** py * z ** pz for f, (px, py, pz) in poly]
            B[..., k] = c * sum(terms)
            A[..., k] = abs(c) * sum(np.abs(t) for t in terms)
            k += 1
    return B, A


def basis(degree, use, dirs, n=None):
    """-> (B, A) [n, K(degree)] with the bands above `use` exactly zero; `dirs` [n, 3] (any length > 0) is read only
    when use >= 1."""
    K = num_bases(degree)
    if use == 0:
        n = len(dirs) if n is None else n
        B = np.zeros((n, K), np.float64)
        B[:, 0] = _C[0][0]
        return B, B.copy()
    d = np.asarray(dirs, np.float64)
    d = d / np.sqrt((d * d).sum(-1, keepdims=True))
    Bu, Au = basis_unit(use, d[:, 0], d[:, 1], d[:, 2])
    B = np.zeros((len(d), K), np.float64)
    A = np.zeros_like(B)
    B[:, :Bu.shape[1]], A[:, :Bu.shape[1]] = Bu, Au
    return B, A


def forward(deg, use, dirs, coeffs, shift=0.0):
    """-> (colours [n, 3], S [n, 3]): sum over the bands in use of B_k c_k (+ shift)."""
    ku = num_bases(use)
    c = np.asarray(coeffs[:, :ku, :], np.float64)
    B = basis(deg, use, dirs, len(c))[0][:, :ku, None]
    return (B * c).sum(1) + shift, (np.abs(B) * np.abs(c)).sum(1) + abs(shift)


def backward(deg, use, dirs, v):
    """-> (v_coeffs [n, K, 3], |B_k| |v|, A_k |v|)"""
    v = np.asarray(v, np.float64)
    B, A = basis(deg, use, dirs, len(v))
    return B[:, :, None] * v[:, None, :], np.abs(B)[:, :, None] * np.abs(v)[:, None, :], A[:, :, None] * np.abs(v)[:, None, :]


def split_forward(deg, use, dirs, dc, rest, shift=0.0, clamp_zero=False):
    """-> (colours, cut, S): cut = the channels the clamp cut (sh + shift < 0), stored as zero."""
    ku = num_bases(use)
    full = np.concatenate([np.asarray(dc).reshape(-1, 1, 3), np.asarray(rest)[:, :ku - 1, :]], 1)
    col, S = forward(use, use, dirs, full, shift)
    cut = (col < 0) if clamp_zero else np.zeros(col.shape, bool)
    return np.where(cut, 0.0, col), cut, S


def split_backward(deg, use, dirs, v, cut_mask=None):
    """-> (v_dc [n, 3], v_rest [n, K-1, 3], bound_dc, bound_rest), the cotangent blocked where cut_mask is set."""
    v = np.asarray(v, np.float64)
    if cut_mask is not None:
        v = np.where(cut_mask, 0.0, v)
    g, b, _ = backward(deg, use, dirs, v)
    return g[:, 0], g[:, 1:], b[:, 0], b[:, 1:]


def views_backward(deg, use, means, campos, v, scale):
    """scale * sum_r B_k(normalize(means - campos[r])) v[r] -> (v_coeffs [n, K, 3], bound, bound from A_k)."""
    means = np.asarray(means, np.float64)
    out = bound = cond = 0.0
    for r in range(len(campos)):
        d = (means - np.asarray(campos[r], np.float64)) if use >= 1 else means
        g, b, a = backward(deg, use, d, v[r])
        out, bound, cond = out + g, bound + b, cond + a
    return scale * out, abs(scale) * bound, abs(scale) * cond


# ---- shared seeded inputs ---------------------------------------------------------------------------------------
POISON = np.array([np.nan, np.inf, -np.inf, 3e38], np.float32)


def poison(a, start_band):
    """a [n, K', 3]: bands >= start_band filled with a rotating pattern of NaN, +Inf, -Inf, 3e38 (a copy)."""
    a = a.copy()
    tail = a[:, start_band:, :]
    tail[...] = POISON[np.arange(tail.size) % 4].reshape(tail.shape)
    return a


@functools.lru_cache(maxsize=None)
def make_inputs(deg, n):
    """-> dict of float32 arrays (read-only): dirs [n, 3] un-normalised with magnitudes 1e-3..1e3, coeffs [n, K, 3]
    (degree >= 1: every fourth row 1e3 times larger with its DC term tuned so that the colour at one `use` >= 1
    nearly cancels: S >> |colour|), v [n, 3]."""
    rng = np.random.default_rng([20, deg, n])
    K = num_bases(deg)
    dirs = rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 1))
    dirs = dirs.astype(np.float32)
    coeffs = rng.standard_normal((n, K, 3))
    coeffs[1::4] *= 1e3
    coeffs = coeffs.astype(np.float32)
    for i in range(1, n, 4) if deg else ():
        use = 1 + (i // 4) % deg
        col, _ = forward(deg, use, dirs[i:i + 1], coeffs[i:i + 1])
        coeffs[i, 0] = (coeffs[i, 0].astype(np.float64) - col[0] / _C[0][0]).astype(np.float32)
    v = rng.standard_normal((n, 3)).astype(np.float32)
    out = dict(dirs=dirs, coeffs=coeffs, v=v)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def make_view_inputs(deg, n, views):
    """-> means [n, 3], msg [V, 3 n + 3] (one gathered message: view r's cotangents, then its camera position).
    Every Gaussian sits at 1e-3..1e3 from the camera (r = its index mod V)."""
    rng = np.random.default_rng([21, deg, n, views])
    campos = rng.uniform(4, 6, (views, 3)).astype(np.float32)
    u = rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 1))
    means = (campos[np.arange(n) % views].astype(np.float64) + u).astype(np.float32)
    msg = rng.standard_normal((views, 3 * n + 3)).astype(np.float32)
    msg[:, 3 * n:] = campos
    means.setflags(write=False)
    msg.setflags(write=False)
    return means, msg


@functools.lru_cache(maxsize=None)
def make_clamp_inputs(deg, n):
    """-> dirs, dc, rest, v for the clamp epilogue at shift 0.5: plain normal coefficients, colours on both sides of 0."""
    rng = np.random.default_rng([22, deg, n])
    K = num_bases(deg)
    out = (rng.standard_normal((n, 3)).astype(np.float32) * 3, rng.standard_normal((n, 3)).astype(np.float32) * 3,
           rng.standard_normal((n, K - 1, 3)).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32))
    for a in out:
        a.setflags(write=False)
    return out
