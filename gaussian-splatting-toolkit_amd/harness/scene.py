"""Synthetic scenes and cameras with the reference's conventions.

Camera: rasterizer convention (x right, y down, z forward), pinhole (or, `model="fisheye"`, equidistant), the
projection matrix of ``gs_toolkit/utils/comms.py:103-123`` (OpenGL-style,
``w_clip = z_view``).  Scene statistics follow SURVEY.md section 8(d):
``z ~ U(2,10)``, ``x,y ~ U(-1,1) * 1.1 * tan(fov/2) * z`` (about 10 % of the
splats fall outside the frustum), log-uniform scales in [0.005, 0.05],
random unit quaternions, opacity ~ U(0.1, 0.9), SH dc ~ U(-1,1)*0.5/C0,
higher bands ~ N(0, 0.1^2).  Everything is generated with numpy from a seed so
that CPU oracle and GPU see bit-identical inputs.
"""
import math
from dataclasses import dataclass
from typing import Dict

import numpy as np

SH_C0 = 0.28209479177387814
BACKGROUND = (0.1490, 0.1647, 0.2157)


def projection_matrix(znear: float, zfar: float, fovx: float, fovy: float) -> np.ndarray:
    t = znear * math.tan(0.5 * fovy)
    b = -t
    r = znear * math.tan(0.5 * fovx)
    l = -r
    n, f = znear, zfar
    return np.array(
        [
            [2 * n / (r - l), 0.0, (r + l) / (r - l), 0.0],
            [0.0, 2 * n / (t - b), (t + b) / (t - b), 0.0],
            [0.0, 0.0, (f + n) / (f - n), -1.0 * f * n / (f - n)],
            [0.0, 0.0, 1.0, 0.0],
        ],
        dtype=np.float32,
    )


@dataclass
class Camera:
    width: int
    height: int
    fx: float
    fy: float
    cx: float
    cy: float
    viewmat: np.ndarray  # [4,4] world->camera, row-major
    projmat: np.ndarray  # [4,4] P @ V
    model: str = "pinhole"  # or "fisheye": equidistant, pixel = f * theta (gs_fused.project_gaussians_fisheye)

    @property
    def campos(self) -> np.ndarray:
        R, t = self.viewmat[:3, :3], self.viewmat[:3, 3]
        return (-R.T @ t).astype(np.float32)


def make_camera(width: int, height: int, fov_x_deg: float = 60.0, yaw: float = 0.0,
                pitch: float = 0.0, roll: float = 0.0, trans=(0.0, 0.0, 0.0), model: str = "pinhole") -> Camera:
    fovx = math.radians(fov_x_deg)
    if model == "fisheye":  # pixel = f * theta: half the width at half the field of view (which may pass 180 degrees)
        fx = width / fovx
        fovx = 2.0 * math.atan(width / (2.0 * fx))  # (the projection matrix of these intrinsics: the fisheye never reads it)
    elif model != "pinhole":
        raise ValueError(f"unknown camera model {model!r}")
    else:
        fx = width / (2.0 * math.tan(fovx / 2.0))
    fy = fx
    fovy = 2.0 * math.atan(height / (2.0 * fy))
    cy_, sy_ = math.cos(yaw), math.sin(yaw)
    cp, sp = math.cos(pitch), math.sin(pitch)
    cr, sr = math.cos(roll), math.sin(roll)
    Ry = np.array([[cy_, 0, sy_], [0, 1, 0], [-sy_, 0, cy_]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    V = np.eye(4, dtype=np.float32)
    V[:3, :3] = (Rz @ Rx @ Ry).astype(np.float32)
    V[:3, 3] = np.asarray(trans, dtype=np.float32)
    P = projection_matrix(0.001, 1000.0, fovx, fovy) @ V
    return Camera(width, height, fx, fy, width / 2.0, height / 2.0, V, P.astype(np.float32), model)


def num_sh_bases(degree: int) -> int:
    return {0: 1, 1: 4, 2: 9, 3: 16}.get(degree, 25)


def make_scene(n: int, cam: Camera, sh_degree: int = 3, seed: int = 42,
               scale_lo: float = 0.005, scale_hi: float = 0.05,
               z_lo: float = 2.0, z_hi: float = 10.0, longtail: bool = False) -> Dict[str, np.ndarray]:
    """Random Gaussian cloud in front of `cam`.  longtail: half of the
    Gaussians are concentrated on 16 square patches that together cover 10 % of the
    frame, so ~10 % of the tiles hold ~10x the list depth of the rest (same total)."""
    rng = np.random.default_rng(seed)
    tanx = 0.5 * cam.width / cam.fx
    tany = 0.5 * cam.height / cam.fy
    z = rng.uniform(z_lo, z_hi, n)
    ux, uy = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    if longtail:
        patches, hs = 16, math.sqrt(0.10 * 4.0 / 16) / 2  # normalised frame = [-1,1]^2, area 4
        centres = rng.uniform(-1 + hs, 1 - hs, (patches, 2))
        which = rng.integers(0, patches, n)
        clustered = rng.uniform(0, 1, n) < 0.5
        ux = np.where(clustered, centres[which, 0] + rng.uniform(-hs, hs, n), ux)
        uy = np.where(clustered, centres[which, 1] + rng.uniform(-hs, hs, n), uy)
    x = ux * 1.1 * tanx * z
    y = uy * 1.1 * tany * z
    p_cam = np.stack([x, y, z], -1)
    R, t = cam.viewmat[:3, :3].astype(np.float64), cam.viewmat[:3, 3].astype(np.float64)
    means = (p_cam - t) @ R  # R^T (p - t)
    scales = np.exp(rng.uniform(math.log(scale_lo), math.log(scale_hi), (n, 3)))
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    opac = rng.uniform(0.1, 0.9, (n, 1))
    K = num_sh_bases(sh_degree)
    sh = np.empty((n, K, 3))
    sh[:, 0, :] = rng.uniform(-1, 1, (n, 3)) * 0.5 / SH_C0
    if K > 1:
        sh[:, 1:, :] = rng.standard_normal((n, K - 1, 3)) * 0.1
    f32 = np.float32
    return dict(means3d=means.astype(f32), scales=scales.astype(f32), quats=q.astype(f32),
                opacities=opac.astype(f32), sh_coeffs=sh.astype(f32))


HELDOUT_KINDS = ("room", "floaters", "needles")


def make_heldout_scene(kind: str, n: int, cam: Camera, sh_degree: int = 3, seed: int = 7) -> Dict[str, np.ndarray]:
    """Scene families shaped like what captures produce and NOT used to fit any dispatch constant (VERDICT r5 item 3;
    rasterizer/cuda/_tuning.py was fitted on the uniform / long-tail clouds, the trainer's ball and object scenes and
    the model config 3 trains).  Same dictionary as `make_scene`.
      room      a few thousand large, flat, nearly opaque splats on the walls of a box around the camera (every tile's
                list ends in them) behind dense small detail on ~40 object surfaces: a spatially correlated heavy tail
      floaters  the uniform cloud with 300 near-camera, faint, screen-filling splats in front of it (each covers
                hundreds of tiles and heads their lists; nothing saturates behind them)
      needles   axis ratio 1:20 to 1:60, random orientation: long thin footprints whose 3-sigma boxes hit many tiles
                that the exact reach test then drops"""
    if kind not in HELDOUT_KINDS:
        raise ValueError(f"unknown held-out scene {kind!r}")
    rng = np.random.default_rng(seed)
    tanx, tany = 0.5 * cam.width / cam.fx, 0.5 * cam.height / cam.fy
    R, t = cam.viewmat[:3, :3].astype(np.float64), cam.viewmat[:3, 3].astype(np.float64)
    unit = lambda q: q / np.linalg.norm(q, axis=-1, keepdims=True)  # noqa: E731
    if kind == "room":
        n_wall = min(max(n // 100, 500), 4000)
        n_obj = n - n_wall
        # walls of the box x = +-6, y = +-3.5, z = 11 (camera space), flat splats lying in the wall
        which = rng.integers(0, 5, n_wall)
        u, v = rng.uniform(-1, 1, n_wall), rng.uniform(-1, 1, n_wall)
        pw = np.empty((n_wall, 3))
        qw = np.empty((n_wall, 4))
        c45 = math.sqrt(0.5)
        for w_, (pos, quat) in enumerate((
                (lambda u_, v_: (6 * u_, 3.5 * v_, np.full_like(u_, 11.0)), (1, 0, 0, 0)),          # back wall (normal z)
                (lambda u_, v_: (np.full_like(u_, -6.0), 3.5 * v_, 5.5 + 5.5 * u_), (c45, 0, c45, 0)),  # left (normal x)
                (lambda u_, v_: (np.full_like(u_, 6.0), 3.5 * v_, 5.5 + 5.5 * u_), (c45, 0, c45, 0)),   # right
                (lambda u_, v_: (6 * u_, np.full_like(u_, 3.5), 5.5 + 5.5 * v_), (c45, c45, 0, 0)),     # floor (normal y)
                (lambda u_, v_: (6 * u_, np.full_like(u_, -3.5), 5.5 + 5.5 * v_), (c45, c45, 0, 0)))):  # ceiling
            m = which == w_
            x_, y_, z_ = pos(u[m], v[m])
            pw[m] = np.stack([x_, y_, z_], -1)
            qw[m] = quat
        sw = np.stack([rng.uniform(0.25, 0.8, n_wall), rng.uniform(0.25, 0.8, n_wall), np.full(n_wall, 0.01)], -1)
        ow = rng.uniform(0.85, 0.995, (n_wall, 1))
        # objects: small splats on sphere surfaces in front of the walls
        n_cl = 40
        cz = rng.uniform(3.0, 8.0, n_cl)
        centres = np.stack([rng.uniform(-0.9, 0.9, n_cl) * tanx * cz, rng.uniform(-0.9, 0.9, n_cl) * tany * cz, cz], -1)
        rad = rng.uniform(0.2, 0.7, n_cl)
        cl = rng.integers(0, n_cl, n_obj)
        d = unit(rng.standard_normal((n_obj, 3)))
        po = centres[cl] + d * rad[cl, None]
        so = np.exp(rng.uniform(math.log(0.004), math.log(0.025), (n_obj, 3)))
        so[:, 2] *= 0.3  # flattened, as surface splats end up
        qo = unit(rng.standard_normal((n_obj, 4)))
        oo = rng.uniform(0.4, 0.99, (n_obj, 1))
        p_cam, scales, q, opac = np.concatenate([pw, po]), np.concatenate([sw, so]), np.concatenate([qw, qo]), np.concatenate([ow, oo])
    elif kind == "floaters":
        n_fl = min(300, max(n // 20, 1))
        base = make_scene(n - n_fl, cam, sh_degree=0, seed=seed + 1, scale_lo=0.0025, scale_hi=0.025)
        pb = base["means3d"].astype(np.float64) @ R.T + t
        z = rng.uniform(0.25, 0.9, n_fl)
        pf = np.stack([rng.uniform(-1, 1, n_fl) * tanx * z, rng.uniform(-1, 1, n_fl) * tany * z, z], -1)
        sf = (rng.uniform(0.03, 0.09, (n_fl, 1)) * z[:, None]) * rng.uniform(0.6, 1.4, (n_fl, 3))
        p_cam = np.concatenate([pf, pb])
        scales = np.concatenate([sf, base["scales"].astype(np.float64)])
        q = np.concatenate([unit(rng.standard_normal((n_fl, 4))), base["quats"].astype(np.float64)])
        opac = np.concatenate([rng.uniform(0.03, 0.25, (n_fl, 1)), base["opacities"].astype(np.float64)])
    else:  # needles
        z = rng.uniform(2.0, 10.0, n)
        p_cam = np.stack([rng.uniform(-1, 1, n) * 1.1 * tanx * z, rng.uniform(-1, 1, n) * 1.1 * tany * z, z], -1)
        long_ = np.exp(rng.uniform(math.log(0.04), math.log(0.4), n))
        ratio = rng.uniform(20.0, 60.0, (n, 2))
        scales = np.stack([long_, long_ / ratio[:, 0], long_ / ratio[:, 1]], -1)
        q = unit(rng.standard_normal((n, 4)))
        opac = rng.uniform(0.1, 0.9, (n, 1))
    means = (p_cam - t) @ R
    K = num_sh_bases(sh_degree)
    sh = np.empty((n, K, 3))
    sh[:, 0, :] = rng.uniform(-1, 1, (n, 3)) * 0.5 / SH_C0
    if K > 1:
        sh[:, 1:, :] = rng.standard_normal((n, K - 1, 3)) * 0.1
    f32 = np.float32
    return dict(means3d=means.astype(f32), scales=scales.astype(f32), quats=q.astype(f32),
                opacities=opac.astype(f32), sh_coeffs=sh.astype(f32))


def make_cotangents(cam: Camera, seed: int = 43):
    rng = np.random.default_rng(seed)
    v_img = rng.uniform(-1, 1, (cam.height, cam.width, 3)).astype(np.float32)
    v_alpha = rng.uniform(-1, 1, (cam.height, cam.width)).astype(np.float32)
    return v_img, v_alpha


def viewdirs_for(scene: Dict[str, np.ndarray], cam: Camera) -> np.ndarray:
    d = scene["means3d"] - cam.campos[None]
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)


def algorithmic_bytes(n: int, num_intersects: int, pixels: int, tiles: int, sh_bases: int):
    """Compulsory HBM traffic per fwd+bwd, per kernel."""
    N, I, P, T, K = n, num_intersects, pixels, tiles, sh_bases
    per = {
        "project_fwd": 100 * N,
        "sh_fwd": (12 + 12 * K) * N + 12 * N,
        # binning as the reference organises it (scan, map, sort, bin edges) ...
        "scan": 8 * N,
        "map": 20 * N + 12 * I,
        "sort": 24 * I,
        "bin_edges": 8 * I + 8 * T,
        "raster_fwd": 40 * I + 20 * P,
        "raster_bwd": 40 * I + 24 * P + 36 * I,
        "project_bwd": 188 * N,
        "sh_bwd": 24 * N + 12 * K * N,
    }
    # ... and grouped the way the fused pipeline launches it (same formula)
    per["depth_order"] = per["scan"]
    per["bin_sorted"] = per["map"] + per["sort"] + per["bin_edges"]
    # not in SURVEY's formula (the reference has no such pass): reads xys, radii, conics,
    # opacity (28 B), writes a count and a 32-byte record per Gaussian
    per["count_reach"] = 64 * N
    per["total"] = sum(v for k, v in per.items() if k not in ("depth_order", "bin_sorted", "count_reach"))
    return per


def built_pipeline_bytes(n: int, list_entries: int, tiles: int):
    """Compulsory HBM traffic of the list construction AS BUILT, which is
    not the reference's organisation that `algorithmic_bytes` prices (scan / map / 64-bit sort /
    bin edges):
      count_reach  60 N              reads xys, radii, conics, opacity (28 B), writes one 32-B record
      depth_order  12 N              reads depth + radius (8 B), writes the order (4 B)
      bin_sorted   36 N + 24 I' + 8 T   two-level partition: order + record per Gaussian, 8 B written
                                     + 14 B read + 4 B written per list entry (rounded up to 24
                                     with the chunk tables), tile_bins
    I' = list entries after the exact reach test."""
    N, I, T = n, list_entries, tiles
    return {"count_reach": 60 * N, "depth_order": 12 * N, "bin_sorted": 36 * N + 24 * I + 8 * T}
