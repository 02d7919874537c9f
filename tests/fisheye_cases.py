"""Seeded inputs for the equidistant fisheye projection, shared by tests/test_fisheye_host.py (CPU) and
tests/test_gpu_fisheye.py.  One camera: 96 x 64 pixels, tiles of 16 (6 x 4), fx = 36.7, fy = 35.1 (anamorphic),
cx = 47.3, cy = 32.6 (off-centre); fx * 75 degrees = half the width.  Gaussians come in named groups of at least 64
rows, each built in view space and mapped back through the inverse view in float64.

  main         the rotated, translated view of tests/projection_cases.py; every group but the exact ones, the
               near plane and the needles
  near_plane   tz within 1e-3 of clip, behind a view of the same rotation whose translation is 0.02 of main's.  These
               rows lie within 0.02 of the camera; behind main's view, 0.57 from the origin, their tz = 0.01 would be
               the sum of terms of 0.45 -- a float32 sum then holds 45 ulp of its result at best, and the forward
               test's floor of 1e-6 of the ROW's magnitude states nothing about it (for the pinhole cases
               projection_reference.forward_condition_fp64 measures the same amplification).  The kernel's sum is
               the pinhole kernel's, text unchanged; what this group is about is the cull and the large J
  needles      scale ratio 1 : 1000, behind main's view
  exact        the identity view, where tx = ty = 0 and tz == clip hold exactly in float32: rows on the axis, rows whose
               r^2 underflows in float32 (r / tz = 1e-20), r / tz = 1e-7, and tz == clip (culled: `<=`)
  precomputed  generic rows of axis ratio below 2 (`_generic`) with the covariances handed in
  blockedge-N  the first N generic rows, N = 255, 256, 257 (the launch's block of 256 lanes)"""
import functools
import math

import numpy as np

from projection_cases import Case, _cov3d, _projection, _view

W, H, BW = 96, 64, 16
FX, FY, CX, CY = 36.7, 35.1, 47.3, 32.6
CLIP = 0.01
KERNEL_SERIES_Q = 1.0 / 32.0  # GSR_FISHEYE_SERIES_Q of csrc/project.hip: r^2 / tz^2 below which the kernel takes the series
NEAR_AXIS = (1e-20, 1e-7, 1e-4, 1e-2, 0.99 * math.sqrt(KERNEL_SERIES_Q), 1.01 * math.sqrt(KERNEL_SERIES_Q))


def _polar(theta, phi, d):
    return np.stack([d * np.sin(theta) * np.cos(phi), d * np.sin(theta) * np.sin(phi), d * np.cos(theta)], -1)


def _cone(rng, n, half_deg):
    """Directions uniform on the sphere inside a cone around +z."""
    return np.arccos(1.0 - rng.uniform(0.0, 1.0, n) * (1.0 - math.cos(math.radians(half_deg)))), \
        rng.uniform(0.0, 2.0 * math.pi, n)


def _corner_phi(rng, n):
    """Azimuths within 3 degrees of the image's corners in the (fx theta cos, fy theta sin) plane: the only directions
    in which a polar angle near 90 degrees is still on this screen."""
    corners = np.array([[-CX / FX, -CY / FY], [(W - CX) / FX, -CY / FY], [-CX / FX, (H - CY) / FY],
                        [(W - CX) / FX, (H - CY) / FY]])
    c = corners[rng.integers(0, 4, n)]
    return np.arctan2(c[:, 1], c[:, 0]) + np.radians(rng.uniform(-3.0, 3.0, n))


def _build(name, rng, groups, identity_view=False, precomputed=False, view=None):
    """groups: [(label, p_cam [k,3], scales [k,3])] -> (Case, {label: slice})."""
    V = view if view is not None else \
        np.eye(4, dtype=np.float32) if identity_view else _view(0.21, -0.13, 0.08, (0.3, -0.2, 0.45))
    P = (_projection(0.001, 1000.0, 0.5 * W / FX, 0.5 * H / FY) @ V.astype(np.float64)).astype(np.float32)
    R, t = V[:3, :3].astype(np.float64), V[:3, 3].astype(np.float64)
    where, at = {}, 0
    for label, p, _ in groups:
        where[label] = slice(at, at + len(p))
        at += len(p)
    p_cam = np.concatenate([p for _, p, _ in groups])
    scales = np.concatenate([s for _, _, s in groups]).astype(np.float32)
    means = ((p_cam - t) @ R).astype(np.float32)
    n = len(means)
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q *= np.exp(rng.uniform(math.log(0.05), math.log(20.0), (n, 1)))  # raw, un-normalised
    case = Case(name, means, scales, q.astype(np.float32), V, P, FX, FY, CX, CY, W, H, BW, clip=CLIP,
                precomputed=precomputed)
    if precomputed:
        object.__setattr__(case, "cov3d", _cov3d(case))
    for a in (case.means3d, case.scales, case.quats, case.viewmat, case.projmat) + (() if case.cov3d is None else (case.cov3d,)):
        a.setflags(write=False)
    return case, where


def _generic(rng, n, round_=False):
    """Directions uniform in an 80 degree cone, depth 1 to 6, three independent log-scales uniform in [-4, -1.5] per
    Gaussian (axis ratios up to 12).
    `round_` (the case with covariances handed in): one log-scale per Gaussian, its three axes 0.7, 1.0 and 1.3 of it
    (each within 5 %) in random order, as in tests/projection_cases.py -- an axis ratio below 2.  A covariance that is
    handed in has no factor M, so its compensation is the plain C00 C11 - C01^2, whose terms are up to (ratio)^2 times
    their difference: from a ratio of 4 on, 16 x 3 roundings of 6e-8 pass the forward rule's floor of 1e-6 of the row,
    the rule is then "no further from float64 than 4 x ANOTHER float32 evaluation happens to be", and about one row in
    ten misses that whatever the kernel does."""
    theta, phi = _cone(rng, n, 80.0)
    p = _polar(theta, phi, rng.uniform(1.0, 6.0, n))
    if not round_:
        return p, np.exp(rng.uniform(-4.0, -1.5, (n, 3)))
    axes = rng.permuted(np.tile([0.7, 1.0, 1.3], (n, 1)), axis=1) * rng.uniform(0.95, 1.05, (n, 3))
    return p, np.exp(rng.uniform(-4.0, -1.5, (n, 1))) * axes


def _sized(rng, p, lo=0.02, hi=0.1):
    """Scales of lo..hi of the distance: a footprint of about fx * lo .. fx * hi pixels wherever the row is."""
    d = np.linalg.norm(p, axis=1)
    return d[:, None] * rng.uniform(lo, hi, (len(p), 1)) * rng.uniform(0.7, 1.3, (len(p), 3))


@functools.lru_cache(maxsize=None)
def cases():
    """-> {name: (Case, {group: slice})}, read-only."""
    out = {}
    rng = np.random.default_rng(2301)
    groups = []
    groups.append(("generic",) + _generic(rng, 640))
    z = rng.uniform(1.0, 6.0, 64)
    p = np.stack([np.zeros(64), np.zeros(64), z], -1)
    groups.append(("on_axis", p, _sized(rng, p)))
    for ratio in NEAR_AXIS:
        z, phi = rng.uniform(1.0, 6.0, 64), rng.uniform(0.0, 2.0 * math.pi, 64)
        p = np.stack([ratio * z * np.cos(phi), ratio * z * np.sin(phi), z], -1)
        groups.append((f"near_axis_{ratio:.4g}", p, _sized(rng, p)))
    theta = np.radians(rng.uniform(85.0, 89.9, 64))
    tz = rng.uniform(0.05, 0.5, 64)
    p = _polar(theta, _corner_phi(rng, 64), tz / np.cos(theta))
    groups.append(("edge", p, _sized(rng, p)))
    theta, phi = _cone(rng, 64, 80.0)
    p = _polar(theta, phi, rng.uniform(0.05, 5.0, 64)) * np.array([1.0, 1.0, -1.0])
    groups.append(("behind", p, _sized(rng, p)))
    out["main"] = _build("fisheye-main", rng, groups)

    rng = np.random.default_rng(2302)
    groups = []
    z = rng.uniform(1.0, 6.0, 64).astype(np.float32).astype(np.float64)
    p = np.stack([np.zeros(64), np.zeros(64), z], -1)
    groups.append(("on_axis", p, _sized(rng, p)))
    for ratio in (1e-20, 1e-7):
        z, phi = rng.uniform(1.0, 6.0, 64), rng.uniform(0.0, 2.0 * math.pi, 64)
        p = np.stack([ratio * z * np.cos(phi), ratio * z * np.sin(phi), z], -1)
        groups.append((f"near_axis_{ratio:.4g}", p, _sized(rng, p)))
    theta, phi = _cone(rng, 64, 45.0)
    tz = np.full(64, float(np.float32(CLIP)))  # 0 x + 0 y + 1 z + 0 is exact in any precision
    p = np.stack([tz * np.tan(theta) * np.cos(phi), tz * np.tan(theta) * np.sin(phi), tz], -1)
    groups.append(("tz_is_clip", p, _sized(rng, p)))
    out["exact"] = _build("fisheye-exact", rng, groups, identity_view=True)

    rng = np.random.default_rng(2305)
    theta, phi = _cone(rng, 128, 45.0)
    tz = CLIP + rng.uniform(-1e-3, 1e-3, 128)
    p = _polar(theta, phi, tz / np.cos(theta))
    out["near_plane"] = _build("fisheye-near-plane", rng, [("near_plane", p, _sized(rng, p))],
                               view=_view(0.21, -0.13, 0.08, (0.006, -0.004, 0.009)))

    rng = np.random.default_rng(2306)
    theta, phi = _cone(rng, 64, 50.0)
    p = _polar(theta, phi, rng.uniform(1.0, 6.0, 64))
    # 1 : 1000 in space, half a pixel to three pixels long on the screen: cov2d + 0.3 I then has a condition number
    # below 30.  A needle tens of pixels long makes the conic the inverse of a matrix of condition 1000, where every
    # float32 evaluation is 1e-4 of the row from float64 and neither the forward's rule (whose floor is 1e-6 of the
    # row) nor the backward's 1e-3 (tests/projection_cases.py keeps such rows out of the pinhole's bar as well) can
    # tell a right kernel from a wrong one
    long_ = np.linalg.norm(p, axis=1) * rng.uniform(0.015, 0.08, 64)
    s = rng.permuted(np.stack([long_, long_ / 1000.0, long_ / 1000.0], -1), axis=1)
    out["needles"] = _build("fisheye-needles", rng, [("needles", p, s)])

    rng = np.random.default_rng(2303)
    out["precomputed"] = _build("fisheye-precomputed", rng, [("generic",) + _generic(rng, 300, round_=True)], precomputed=True)
    for n in (255, 256, 257):
        rng = np.random.default_rng(2304)
        out[f"blockedge-{n}"] = _build(f"fisheye-blockedge-{n}", rng, [("generic",) + _generic(rng, n)])
    assert all(c.n <= 1600 for c, _ in out.values())
    return out


def case(name):
    return cases()[name]


def names():
    return list(cases())


def reference_args(c):
    """The positional arguments of fisheye_reference.project_forward_fisheye_fp64 (cov3d by keyword)."""
    sq = (None, None) if c.precomputed else (c.scales, c.quats)
    return (c.means3d, sq[0], c.glob_scale, sq[1], c.viewmat[:3], c.projmat, c.fx, c.fy, c.cx, c.cy, c.H, c.W, c.bw,
            c.clip)
