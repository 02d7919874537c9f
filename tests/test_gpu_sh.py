"""GPU: every kernel family of csrc/sh.hip against the float64 reference of tests/sh_reference.py, through the C ABI.

Tolerances (not tuned against the kernels): an element may be off by  tol * 2^-24 * S  of its own conditioning sum S
(sh_reference.py).  tol = 4 x r, r = the worst ratio of the float32 oracle on the same inputs, measured and pinned by
test_sh_host.py::test_oracle_error_in_units_of_conditioning:
    forward   r_fwd      = 7.75   (recorded 7.8)    -> tol 31.2      S = sum_k |B_k| |c_k| (+ |shift|)
    backward  r_bwd      = 4.755e4 (recorded 4.76e4) -> tol 1.904e5   S = |B_k| |v|
    backward  r_bwd_cond = 8.84   (recorded 8.9)    -> tol 35.6      S = A_k |v|, A_k = sum of |monomials| of B_k
The factor 4 covers rsqrtf where the oracle divides by sqrtf, FMA contraction and the different association of the
band sums.  |B_k| |v| is blind to the cancellation inside a basis function (the oracle itself is 4.8e4 units off
where xx - yy nearly vanishes), which makes that bound loose everywhere else: the backward is held to both it and the
A_k one, and the A_k one is what bites.  An element with S == 0 (a band above `use`) must be exactly zero.

Sizes: the wave boundary +-1, the workgroup boundary +-1, one ragged multi-workgroup size, and 1.  Every input and
output sits inside a larger allocation with 256 guard rows on both sides (a whole workgroup of rows: every access
stays inside the allocation): input guards hold NaN (or, for the comparison, something else), output guards a
sentinel bit pattern that must survive the call.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import sh_reference as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = torch.float32
SENTINEL = 0x7FA5C3A5  # (as a float: a NaN, so that an element the kernel failed to write cannot pass either)
GUARD = 256            # rows
CUT = 0x80000000       # -0.0: a channel the clamp cut (include/gsraster.h)
SMALL = (1, 63, 65, 257)


def _abi():
    from rasterizer.cuda import _call, _ptr, _stream
    return _call, _ptr, _stream


class Arena:
    """Device arrays with guards around them."""

    def __init__(self, fill=float("nan")):
        self.fill, self.outs = fill, []

    @staticmethod
    def _guard(row):
        return -(-GUARD * row // 4) * 4  # whole float4s: the body's alignment is the offset's

    def inp(self, a, row, offset=0):
        a = np.array(a, np.float32).reshape(-1)
        g = self._guard(row)
        buf = torch.full((offset + 2 * g + a.size + 4,), self.fill, dtype=F32, device=DEV)
        body = buf[offset + g:offset + g + a.size]
        body.copy_(torch.from_numpy(a))
        assert (body.data_ptr() % 16 == 0) == (offset % 4 == 0)
        return body

    def out(self, size, row, offset=0):
        g = self._guard(row)
        buf = torch.full((offset + 2 * g + size + 4,), SENTINEL, dtype=torch.int32, device=DEV)
        self.outs.append((buf, offset + g, size))
        body = buf[offset + g:offset + g + size].view(F32)
        assert (body.data_ptr() % 16 == 0) == (offset % 4 == 0)
        return body

    def check(self):
        torch.cuda.synchronize()
        for buf, start, size in self.outs:
            assert bool((buf[:start] == SENTINEL).all()) and bool((buf[start + size:] == SENTINEL).all()), \
                "a kernel wrote outside its rows"


def _u(v):
    return C.c_uint(int(v))


def gpu_joint(deg, use, dirs, coeffs, v, offset=0, fill=float("nan")):
    """gsr_sh_forward and gsr_sh_backward -> (colours [n, 3], v_coeffs [n, K, 3]); `offset` floats move the
    coefficient buffers off 16-byte alignment (K = 16: the generic kernels instead of sh16_*)."""
    call, ptr, stream = _abi()
    n, K = len(dirs), R.num_bases(deg)
    A = Arena(fill)
    d, c, vv = A.inp(dirs, 3), A.inp(coeffs, 3 * K, offset), A.inp(v, 3)
    col, g = A.out(3 * n, 3), A.out(3 * K * n, 3 * K, offset)
    call("gsr_sh_forward", _u(n), _u(deg), _u(use), ptr(d), ptr(c), ptr(col), stream(DEV))
    call("gsr_sh_backward", _u(n), _u(deg), _u(use), ptr(d), ptr(vv), ptr(g), stream(DEV))
    A.check()
    return col.cpu().numpy().reshape(n, 3), g.cpu().numpy().reshape(n, K, 3)


def gpu_split(deg, use, dirs, dc, rest, v, shift=0.0, clamp=False, offset=0, fill=float("nan")):
    """gsr_sh_forward_split and gsr_sh_backward_split (degree 0 included: the DC-only kernels, which the Python
    wrapper never reaches) -> (colours, v_dc, v_rest); `offset` moves `rest` / `v_rest` off 16-byte alignment."""
    call, ptr, stream = _abi()
    n, K = len(dc), R.num_bases(deg)
    A = Arena(fill)
    d, c0, vv = A.inp(dirs, 3), A.inp(dc, 3), A.inp(v, 3)
    c1 = A.inp(rest, 3 * (K - 1), offset) if K > 1 else None
    col, g0 = A.out(3 * n, 3), A.out(3 * n, 3)
    g1 = A.out(3 * (K - 1) * n, 3 * (K - 1), offset) if K > 1 else None
    opt = lambda t: ptr(t) if t is not None else None  # noqa: E731
    call("gsr_sh_forward_split", _u(n), _u(deg), _u(use), ptr(d), ptr(c0), opt(c1), ptr(col), C.c_float(shift),
         C.c_int(int(clamp)), stream(DEV))
    call("gsr_sh_backward_split", _u(n), _u(deg), _u(use), ptr(d), ptr(vv), ptr(col) if clamp else None, ptr(g0),
         opt(g1), stream(DEV))
    A.check()
    return (col.cpu().numpy().reshape(n, 3), g0.cpu().numpy().reshape(n, 3),
            g1.cpu().numpy().reshape(n, K - 1, 3) if K > 1 else np.zeros((n, 0, 3), np.float32))


def gpu_views(deg, use, means, msg, scale, split, fill=float("nan")):
    """gsr_sh_backward_views on one gathered message [V, 3 n + 3] (strided views) -> v_coeffs [n, K, 3]"""
    call, ptr, stream = _abi()
    n, K, V = len(means), R.num_bases(deg), len(msg)
    A = Arena(fill)
    m, mm = A.inp(means, 3), A.inp(msg, 3)
    g0 = g1 = gj = None
    if split:
        g0 = A.out(3 * n, 3)
        g1 = A.out(3 * (K - 1) * n, 3 * (K - 1)) if K > 1 else None
    else:
        gj = A.out(3 * K * n, 3 * K)
    opt = lambda t: ptr(t) if t is not None else None  # noqa: E731
    call("gsr_sh_backward_views", _u(n), _u(deg), _u(use), _u(V), ptr(m), C.c_void_p(mm.data_ptr() + 12 * n),
         C.c_size_t(3 * n + 3), ptr(mm), C.c_size_t(3 * n + 3), C.c_float(scale), opt(g0), opt(g1), opt(gj), stream(DEV))
    A.check()
    if not split:
        return gj.cpu().numpy().reshape(n, K, 3)
    rest = g1.cpu().numpy().reshape(n, K - 1, 3) if K > 1 else np.zeros((n, 0, 3), np.float32)
    return np.concatenate([g0.cpu().numpy().reshape(n, 1, 3), rest], 1)


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


WORST = {}


def within(got, ref, S, tol, what):
    """|got - ref| <= tol 2^-24 S element by element (S == 0: exactly zero); NaN fails."""
    err = np.abs(got.astype(np.float64) - ref)
    ok = err <= tol * R.U * S
    ratio = np.nanmax(np.where(S > 0, err / np.where(S > 0, R.U * S, 1.0), 0.0)) if err.size else 0.0
    key = what.split(":")[0]
    WORST[key] = max(WORST.get(key, 0.0), float(ratio))
    assert ok.all(), (f"{what}: {(~ok).sum()} of {ok.size} elements beyond {tol} x 2^-24 S; worst ratio {ratio:.4g}, "
                      f"first at {np.argwhere(~ok)[0]}, NaN {np.isnan(got).sum()}")


def check_fwd(got, ref, what):
    assert np.isfinite(got).all(), what
    within(got, ref[0], ref[1], R.TOL_FWD, "forward:" + what)


def check_bwd(got, ref, what):
    within(got, ref[0], ref[1], R.TOL_BWD, "backward:" + what)
    within(got, ref[0], ref[2], R.TOL_BWD_COND, "backward_cond:" + what)


@functools.lru_cache(maxsize=None)
def ref_fwd(deg, use, n, shift=0.0):
    I = R.make_inputs(deg, n)
    return R.forward(deg, use, I["dirs"], I["coeffs"], shift)


@functools.lru_cache(maxsize=None)
def ref_bwd(deg, use, n):
    I = R.make_inputs(deg, n)
    return R.backward(deg, use, I["dirs"], I["v"])


@functools.lru_cache(maxsize=None)
def ref_views(deg, use, n, V, scale):
    means, msg = R.make_view_inputs(deg, n, V)
    return R.views_backward(deg, use, means, msg[:, 3 * n:], msg[:, :3 * n].reshape(V, n, 3), scale)


def report(name):
    print(f"{name}: worst ratios (units of 2^-24 S) " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items())))
    WORST.clear()


JOINT = [(0, 0), (1, 0), (2, 0), (3, 0), (3, 1), (4, 0)]  # (degree, offset); (3, 0): sh16_*, (3, 1): generic K = 16
SPLIT = [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1)]  # offset 0: float4 rows, 1: scalar rows
VIEWS = [(deg, split, V) for deg in (0, 1, 2, 3) for split in (False, True) for V in (1, 3)]


# ---- 1. every family, every use <= degree, against float64 ----------------------------------------------------------
@pytest.mark.parametrize("deg,offset", JOINT)
def test_joint_against_float64(deg, offset):
    for n in R.SIZES:
        I = R.make_inputs(deg, n)
        for use in range(deg + 1):
            col, g = gpu_joint(deg, use, I["dirs"], I["coeffs"], I["v"], offset)
            check_fwd(col, ref_fwd(deg, use, n), f"joint deg {deg} use {use} n {n} offset {offset}")
            check_bwd(g, ref_bwd(deg, use, n), f"joint deg {deg} use {use} n {n} offset {offset}")
    report(f"joint {deg}/{offset}")


@pytest.mark.parametrize("deg,offset", SPLIT)
def test_split_against_float64(deg, offset):
    for n in R.SIZES:
        I = R.make_inputs(deg, n)
        for use in range(deg + 1):
            col, g0, g1 = gpu_split(deg, use, I["dirs"], I["coeffs"][:, 0], I["coeffs"][:, 1:], I["v"], shift=0.25,
                                    offset=offset)
            what = f"split deg {deg} use {use} n {n} offset {offset}"
            check_fwd(col, ref_fwd(deg, use, n, 0.25), what)
            check_bwd(np.concatenate([g0[:, None], g1], 1), ref_bwd(deg, use, n), what)
    report(f"split {deg}/{offset}")


@pytest.mark.parametrize("deg,split,V", VIEWS)
def test_views_against_float64(deg, split, V):
    scale = 0.37
    for n in R.SIZES:
        means, msg = R.make_view_inputs(deg, n, V)
        for use in range(deg + 1):
            g = gpu_views(deg, use, means, msg, scale, split)
            check_bwd(g, ref_views(deg, use, n, V, scale), f"views deg {deg} use {use} n {n} V {V} split {split}")
    report(f"views {deg}/{split}/{V}")


# ---- 2. unused inputs must not reach outputs ------------------------------------------------------------------------
def _poisoned_dirs(dirs, use):
    """use == 0: NaN and zero directions (not observed at all).  Else unchanged."""
    if use > 0:
        return dirs
    d = dirs.copy()
    d[0::2], d[1::2] = np.nan, 0.0
    return d


def _broken_rows(dirs):
    """a zero and a NaN direction: at use >= 1 those rows are NaN in the bands in use (like the reference's x / norm)
    and must still be exact zeros in the others"""
    d = dirs.copy()
    d[0] = 0.0
    d[len(d) // 2] = np.nan
    return d, sorted({0, len(d) // 2})


@pytest.mark.parametrize("deg,offset", [c for c in JOINT if c[0] > 0])
def test_joint_unused_bands_and_direction_are_not_observed(deg, offset):
    for n in R.SIZES:
        I = R.make_inputs(deg, n)
        for use in range(deg + 1):
            ku = R.num_bases(use)
            dirs = _poisoned_dirs(I["dirs"], use)
            zeroed = I["coeffs"].copy()
            zeroed[:, ku:] = 0
            what = f"joint deg {deg} use {use} n {n} offset {offset}"
            col, g = gpu_joint(deg, use, dirs, R.poison(I["coeffs"], ku), I["v"], offset)
            check_fwd(col, ref_fwd(deg, use, n), what)
            col0, _ = gpu_joint(deg, use, dirs, zeroed, I["v"], offset)
            assert bits_equal(col, col0), what
            check_bwd(g, ref_bwd(deg, use, n), what)
            assert np.all(g[:, ku:] == 0), what
            if 1 <= use < deg:
                bad, rows = _broken_rows(I["dirs"])
                _, g = gpu_joint(deg, use, bad, zeroed, I["v"], offset)
                assert np.all(g[:, ku:] == 0) and np.isnan(g[rows, 1:ku]).all(), what
                keep = np.setdiff1d(np.arange(n), rows)
                check_bwd(g[keep], [a[keep] for a in ref_bwd(deg, use, n)], what)


@pytest.mark.parametrize("deg,offset", SPLIT)
def test_split_unused_bands_and_direction_are_not_observed(deg, offset):
    for n in R.SIZES:
        I = R.make_inputs(deg, n)
        dc, rest = I["coeffs"][:, 0], I["coeffs"][:, 1:]
        for use in range(deg + 1):
            ku = R.num_bases(use)
            dirs = _poisoned_dirs(I["dirs"], use)
            zeroed = rest.copy()
            zeroed[:, ku - 1:] = 0
            what = f"split deg {deg} use {use} n {n} offset {offset}"
            col, g0, g1 = gpu_split(deg, use, dirs, dc, R.poison(rest, ku - 1), I["v"], shift=0.25, offset=offset)
            check_fwd(col, ref_fwd(deg, use, n, 0.25), what)
            assert bits_equal(col, gpu_split(deg, use, dirs, dc, zeroed, I["v"], shift=0.25, offset=offset)[0]), what
            check_bwd(np.concatenate([g0[:, None], g1], 1), ref_bwd(deg, use, n), what)
            assert np.all(g1[:, ku - 1:] == 0), what
            if 1 <= use < deg:
                bad, rows = _broken_rows(I["dirs"])
                _, g0, g1 = gpu_split(deg, use, bad, dc, zeroed, I["v"], offset=offset)
                assert np.all(g1[:, ku - 1:] == 0) and np.isnan(g1[rows, :ku - 1]).all(), what


@pytest.mark.parametrize("deg,split,V", [c for c in VIEWS if c[0] > 0])
def test_views_a_gaussian_at_a_camera_reaches_only_the_bands_in_use(deg, split, V):
    scale = 0.37
    for n in R.SIZES:
        means, msg = R.make_view_inputs(deg, n, V)
        means = means.copy()
        at = 5 % n
        means[at] = msg[V - 1, 3 * n:]  # exactly at the last camera: a zero direction
        v = msg[:, :3 * n].reshape(V, n, 3)
        for use in range(deg):
            ku = R.num_bases(use)
            g = gpu_views(deg, use, means, msg, scale, split)
            what = f"views deg {deg} use {use} n {n} V {V} split {split}"
            assert np.all(g[:, ku:] == 0), what
            if use == 0:  # the direction is not observed: finite, and the value of the reference
                assert np.isfinite(g).all(), what
                check_bwd(g, R.views_backward(deg, 0, means, msg[:, 3 * n:], v, scale), what)
            else:
                assert np.isnan(g[at, 1:ku]).all(), what


# ---- 3. nothing outside rows [0, n) matters -------------------------------------------------------------------------
def test_guards_joint_split_views():
    """Results do not depend on what surrounds the arrays (NaN against a finite filler in every input guard), bit for
    bit; that the output guards survive is checked inside every call of this file (Arena.check)."""
    other = 12345.678
    for n in SMALL:
        for deg, offset in JOINT:
            I = R.make_inputs(deg, n)
            for use in {0, deg}:
                a = gpu_joint(deg, use, I["dirs"], I["coeffs"], I["v"], offset)
                b = gpu_joint(deg, use, I["dirs"], I["coeffs"], I["v"], offset, fill=other)
                assert all(bits_equal(x, y) for x, y in zip(a, b)), (deg, offset, use, n)
        for deg, offset in SPLIT:
            I = R.make_inputs(deg, n)
            for use in {0, deg}:
                args = (deg, use, I["dirs"], I["coeffs"][:, 0], I["coeffs"][:, 1:], I["v"], 0.5, True, offset)
                a, b = gpu_split(*args), gpu_split(*args, fill=other)
                assert all(bits_equal(x, y) for x, y in zip(a, b)), (deg, offset, use, n)
        for deg, split, V in VIEWS:
            means, msg = R.make_view_inputs(deg, n, V)
            a = gpu_views(deg, deg, means, msg, 0.37, split)
            b = gpu_views(deg, deg, means, msg, 0.37, split, fill=other)
            assert bits_equal(a, b), (deg, split, V, n)


# ---- 4. the clamp epilogue at the cut -------------------------------------------------------------------------------
@pytest.mark.parametrize("deg,offset", SPLIT)
def test_clamp_blocks_the_gradient_exactly_where_the_colour_is_negative(deg, offset):
    for n in R.SIZES:
        dirs, dc, rest, v = R.make_clamp_inputs(deg, n) if deg else R.make_clamp_inputs(1, n)
        rest = rest[:, :R.num_bases(deg) - 1]
        for use in range(deg + 1):
            what = f"clamp deg {deg} use {use} n {n} offset {offset}"
            col64, S = R.forward(deg, use, dirs, np.concatenate([dc[:, None], rest], 1), 0.5)
            decided = np.abs(col64) > R.TOL_FWD * R.U * S  # elsewhere float32 may land on either side of 0
            assert (~decided).mean() <= 0.01, what
            col, g0, g1 = gpu_split(deg, use, dirs, dc, rest, v, shift=0.5, clamp=True, offset=offset)
            cut = col.view(np.uint32) == CUT
            assert np.array_equal(cut[decided], (col64 < 0)[decided]), what
            assert np.all(col[cut] == 0) and np.all(col >= 0), what
            check_fwd(col, (np.where(cut, 0.0, col64), np.where(cut & ~decided, np.inf, S)), what)
            # the gradient: blocked (exact zeros in every band) where the stored colour is cut, passed elsewhere
            r0, r1, b0, b1 = R.split_backward(deg, use, dirs, v, cut)
            g = np.concatenate([g0[:, None], g1], 1)
            assert np.all(g[np.broadcast_to(cut[:, None, :], g.shape)] == 0), what
            assert np.all(g0[~cut] != 0), what
            _, _, a = R.backward(deg, use, dirs, np.where(cut, 0.0, v))
            check_bwd(g, (np.concatenate([r0[:, None], r1], 1), np.concatenate([b0[:, None], b1], 1), a), what)
    report(f"clamp {deg}/{offset}")
