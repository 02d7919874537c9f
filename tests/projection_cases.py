"""Seeded projection inputs off the one camera family of `harness.scene` (fy = fx, centred principal point,
glob_scale 1, clip 0.01 with everything far beyond it, unit quaternions, centres inside the frustum): shared by
tests/test_projection_host.py (CPU) and tests/test_gpu_projection.py, and by tests/golden/make_golden_project.py.

Every case is built directly (no `make_scene`), holds at most 4096 Gaussians, uses a rotated and translated view
matrix (the 16 `tz == clip` rows apart: they need an identity view for the equality to be exact), and states what
share of its rows must come out visible -- and, where the guard band is the point, with the 1.3x clamp active -- so
that a change of the generator cannot quietly turn a case into one that tests nothing."""
import functools
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np


@dataclass(frozen=True)
class Case:
    name: str
    means3d: np.ndarray            # [n,3] float32
    scales: np.ndarray             # [n,3] float32
    quats: np.ndarray              # [n,4] float32 (w,x,y,z)
    viewmat: np.ndarray            # [4,4] float32
    projmat: np.ndarray            # [4,4] float32, P @ V
    fx: float
    fy: float
    cx: float
    cy: float
    W: int
    H: int
    bw: int
    glob_scale: float = 1.0
    clip: float = 0.01
    precomputed: bool = False      # hand `cov3d` in, scales and quats absent
    cov3d: Optional[np.ndarray] = None  # [n,6] float32: M M^T of the above in float64, rounded (precomputed cases)
    min_visible: float = 0.0       # share of the rows that must have radii > 0 ...
    max_visible: float = 1.0       # ... and that may
    min_clamped_visible: float = 0.0  # share of the rows that must be visible with the 1.3x clamp active
    in_golden: bool = False        # the reference's torch code can run it (tests/golden/project.npz)

    @property
    def n(self):
        return len(self.means3d)

    def forward_args(self):
        """(num_points, means3d, scales, glob_scale, quats, viewmat[:3], projmat, fx, fy, cx, cy, H, W, bw, clip):
        the positional arguments of project_gaussians_forward (oracle and rasterizer.cuda); scales / quats None where
        the case hands cov3d in (`cov3d_precomp=case.cov3d`)."""
        sq = (None, None) if self.precomputed else (self.scales, self.quats)
        return (self.n, self.means3d, sq[0], self.glob_scale, sq[1], self.viewmat[:3], self.projmat, self.fx, self.fy,
                self.cx, self.cy, self.H, self.W, self.bw, self.clip)


def _view(yaw, pitch, roll, trans):
    cy_, sy_, cp, sp, cr, sr = (f(a) for a in (yaw, pitch, roll) for f in (math.cos, math.sin))
    Ry = np.array([[cy_, 0, sy_], [0, 1, 0], [-sy_, 0, cy_]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    V = np.eye(4)
    V[:3, :3] = Rz @ Rx @ Ry
    V[:3, 3] = trans
    return V.astype(np.float32)


def _projection(znear, zfar, tanx, tany):
    # the OpenGL-style matrix of the reference (gs_toolkit/utils/comms.py:103-123): symmetric frustum, w_clip = z_view
    return np.array([[1.0 / tanx, 0, 0, 0], [0, 1.0 / tany, 0, 0],
                     [0, 0, (zfar + znear) / (zfar - znear), -zfar * znear / (zfar - znear)], [0, 0, 1, 0]])


def _case(name, rng, n, W, H, bw, *, fy_ratio=1.0, centre=(0.5, 0.5), identity_view=False, ratios=None, z=None,
          z_range=(2.0, 10.0), scale=(0.02, 0.2), quat_norms=None, **kw):
    """`ratios` [n,2]: (tx/tz) / tan_fovx and (ty/tz) / tan_fovy of the centres (default: uniform in +-0.95);
    `z` [n]: view-space depths (default: uniform in `z_range`); `scale`: (lo, hi) of the sizes, numbers or [n] each."""
    fx = W / (2.0 * math.tan(math.radians(30.0)))
    fy = fy_ratio * fx
    tanx, tany = 0.5 * W / fx, 0.5 * H / fy
    V = np.eye(4, dtype=np.float32) if identity_view else _view(0.21, -0.13, 0.08, (0.3, -0.2, 0.45))
    P = (_projection(0.001, 1000.0, tanx, tany) @ V.astype(np.float64)).astype(np.float32)
    if ratios is None:
        ratios = rng.uniform(-0.95, 0.95, (n, 2))
    if z is None:
        z = rng.uniform(*z_range, n)
    p_cam = np.stack([ratios[:, 0] * tanx * z, ratios[:, 1] * tany * z, z], -1)
    R, t = V[:3, :3].astype(np.float64), V[:3, 3].astype(np.float64)
    means = ((p_cam - t) @ R).astype(np.float32)  # R^T (p - t)
    # Sizes log-uniform per Gaussian; the three axes are 0.7, 1.0 and 1.3 of the size (each within 5 %), in random
    # order.  Every covariance is then well conditioned (axis ratio below 2) and none is nearly a sphere: on a sphere
    # v_quat vanishes, and next to one it is the small difference of large terms, where no fp32 evaluation holds 1e-5
    # of the row -- the bar the oracle's VJP is held to against float64 (tests/test_projection_host.py) is one for
    # well-conditioned rows; needles are held to float64 by tests/test_gpu_heldout.py under its own rule
    # Every case keeps its smallest splat above ~0.2 px (compensation > 0.1, which the host test asserts as the
    # well-conditioned test of tests/test_project_fp64.py does: the compensation's cotangent is divided by it).
    lo, hi = (np.broadcast_to(np.asarray(v, float), (n,)) for v in scale)
    axes = rng.permuted(np.tile([0.7, 1.0, 1.3], (n, 1)), axis=1) * rng.uniform(0.95, 1.05, (n, 3))
    scales = (np.exp(rng.uniform(np.log(lo), np.log(hi)))[:, None] * axes).astype(np.float32)
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    if quat_norms is not None:
        q *= np.exp(rng.uniform(math.log(quat_norms[0]), math.log(quat_norms[1]), (n, 1)))
    case = Case(name, means, scales, q.astype(np.float32), V, P, fx, fy, centre[0] * W, centre[1] * H, W, H, bw, **kw)
    if case.precomputed:
        object.__setattr__(case, "cov3d", _cov3d(case))
    return case


def _cov3d(case):
    q = case.quats.astype(np.float64)
    w, x, y, z = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                  np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                  np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)
    M = R * (float(np.float32(case.glob_scale)) * case.scales.astype(np.float64))[:, None, :]
    S = M @ M.transpose(0, 2, 1)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], -1).astype(np.float32)


def _thirds(rng, n):
    """|ratio| in thirds from [0, 1), [1, 1.3) and (1.3, 3], random sign, shuffled."""
    k = n // 3
    r = np.concatenate([rng.uniform(0.0, 1.0, k), rng.uniform(1.0, 1.3, k), rng.uniform(1.3001, 3.0, n - 2 * k)])
    return rng.permutation(r * rng.choice([-1.0, 1.0], n))


def _guard_ratios(rng, n):
    """One axis by thirds, the other inside the frustum; the first half of the rows has x outside, the second y."""
    out = np.stack([_thirds(rng, n), rng.uniform(-0.9, 0.9, n)], -1)
    out[n // 2:] = out[n // 2:, ::-1]
    return out


def _outside(ratios, outer, inner):
    """[n]: `outer` for the rows beyond the 1.3x guard band, `inner` for the others."""
    return np.where((np.abs(ratios) > 1.3).any(axis=1), outer, inner)


def _near_depths(rng, n, clip):
    """A quarter behind the camera, a quarter between 0 and the threshold, the rest beyond it."""
    k = n // 4
    return rng.permutation(np.concatenate([rng.uniform(-5.0, -0.05, k), rng.uniform(0.02 * clip, 0.98 * clip, k),
                                           rng.uniform(1.02 * clip, clip + 8.0, n - 2 * k)]))


@functools.lru_cache(maxsize=None)
def cases():
    """-> tuple of Case, in a fixed order (read-only: they are shared by every test of a run)."""
    out = []
    rng = lambda seed: np.random.default_rng(seed)  # noqa: E731  (a generator per case: adding one moves no other)
    # anamorphic: fy = 0.6 fx, W != H -- an fx/fy or W/H swap anywhere changes the answer
    out.append(_case("anamorphic-317x203-bw16", rng(101), 600, 317, 203, 16, fy_ratio=0.6, min_visible=0.95,
                     in_golden=True))
    out.append(_case("anamorphic-97x61-bw5", rng(102), 600, 97, 61, 5, fy_ratio=0.6, min_visible=0.95, scale=(0.06, 0.4),
                     in_golden=True))
    # off-centre principal point (the frustum of the projection matrix stays symmetric: cx, cy enter in ndc -> pixel)
    # the centres cover the image, which lies at ratios [-0.62, 1.38] x [-1.28, 0.72] of this frustum
    r = rng(103)
    out.append(_case("offcentre", r, 600, 211, 134, 16, centre=(0.31, 0.64), min_visible=0.95, in_golden=True,
                     ratios=np.stack([r.uniform(-0.6, 1.29, 600), r.uniform(-1.27, 0.7, 600)], -1)))
    for g, seed in ((0.37, 104), (2.5, 105)):
        out.append(_case(f"globscale-{g}", rng(seed), 600, 200, 120, 16, glob_scale=g, min_visible=0.95,
                         scale=(0.02 / g, 0.2 / g), in_golden=True))
    for clip, seed in ((0.2, 106), (3.0, 107)):
        r = rng(seed)
        n = 800
        # the half beyond the threshold is in the frustum and visible; nothing of the other half may be
        out.append(_case(f"nearplane-{clip}", r, n, 200, 120, 16, clip=clip, z=_near_depths(r, n, clip),
                         scale=(0.02, 0.1), min_visible=0.45, max_visible=0.5))
        # tz == clip exactly: identity view, z = clip in float32 (0 * x + 0 * y + 1 * z + 0 is exact in any precision)
        out.append(_case(f"nearplane-{clip}-exact", r, 16, 200, 120, 16, clip=clip, identity_view=True,
                         z=np.full(16, float(np.float32(clip))), scale=(0.01, 0.1), max_visible=0.0))
    # guard band: a third of the rows beyond 1.3x the frustum on one axis, large enough (3-sigma radius of
    # ~ 3 fx s / z = 50..400 px at 317 px width) that many of them still reach the image: the outer third's centres lie
    # 0.15..1 image widths outside it.  At least a quarter of that third (1/12 of all rows) must be visible and clamped.
    # The rows inside the band -- the only ones the backward is comparable on -- come in all sizes from a fifth of a pixel
    r = rng(108)
    ratios = _guard_ratios(r, 900)
    out.append(_case("guardband", r, 900, 317, 203, 16, ratios=ratios, z_range=(2.0, 6.0),
                     scale=(_outside(ratios, 0.3, 0.011), _outside(ratios, 1.0, 0.1)), min_visible=0.6, min_clamped_visible=1.0 / 12))
    out.append(_case("rawquats", rng(109), 600, 200, 120, 16, quat_norms=(0.05, 20.0), min_visible=0.95,
                     in_golden=True))
    out.append(_case("precomputed", rng(110), 600, 200, 120, 16, precomputed=True, min_visible=0.95))
    for n in (1, 255, 256, 257):
        # (sizes around a pixel: the compensation's VJP is comparable on most rows, on the one of n = 1 too)
        out.append(_case(f"blockedge-{n}", rng(111), n, 200, 120, 16, scale=(0.02, 0.05), min_visible=0.9))
    # (visible: the half beyond the near plane, of which the third inside the frustum is on screen whatever its size,
    #  1/6 of the rows; the others reach the image where they are large enough)
    # everything at once (1789 rows: 6 full blocks and one of 253 lanes)
    for name, seed, pre in (("everything", 112, False), ("everything-precomputed", 112, True)):
        r = rng(seed)
        n = 1789
        ratios = _guard_ratios(r, n)
        out.append(_case(name, r, n, 317, 203, 5 if pre else 16, fy_ratio=0.6, centre=(0.31, 0.64), glob_scale=0.37,
                         clip=0.2, ratios=ratios, z=_near_depths(r, n, 0.2), scale=(_outside(ratios, 0.3, 0.04), _outside(ratios, 2.5, 0.3)),
                         quat_norms=(0.05, 20.0), precomputed=pre, in_golden=not pre,
                         min_visible=0.2, max_visible=0.5, min_clamped_visible=1.0 / 24))
    assert len({c.name for c in out}) == len(out) and all(c.n <= 4096 for c in out)
    for c in out:
        for a in (c.means3d, c.scales, c.quats, c.viewmat, c.projmat) + (() if c.cov3d is None else (c.cov3d,)):
            a.setflags(write=False)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


def names(**where):
    """Names of the cases whose attributes equal `where` (for pytest.mark.parametrize)."""
    return [c.name for c in cases() if all(getattr(c, k) == v for k, v in where.items())]


def cotangents(case_, seed=5):
    """-> (v_xy, v_depth, v_conic, v_compensation), float32 standard normal."""
    rng = np.random.default_rng(seed)
    n = case_.n
    return tuple(rng.standard_normal(s).astype(np.float32) for s in ((n, 2), (n,), (n, 3), (n,)))
