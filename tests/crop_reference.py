"""Host restatements of the oriented crop box, for tests/test_crop_host.py and tests/test_gpu_crop.py.

Two of them, on purpose:

* `crop_values` / `within_f32` -- the project's rule (csrc/gsr_common.h, `gsr_crop_inside`) in numpy.float32: the
  world->box matrix is the float64 inverse of [[R, T], [0, 1]] rounded once, q_k = ((A_k0 x + A_k1 y) + A_k2 z) + A_k3
  with every operation rounded on its own, inside <=> -h_k < q_k < h_k strictly.  The kernels must equal this bit for
  bit.
* `within_reference` -- `OrientedBox.within` as the reference writes it (gs_toolkit/data/scene_box.py:83-96): a
  float32 ``torch.inverse`` of H, a homogeneous matmul, ``pts > -S / 2`` and ``pts < S / 2``.  The reference module
  itself cannot be imported here: it imports ``viser`` and ``jaxtyping`` at its top, and neither is installed.  Its
  arithmetic order differs from the rule's (another inverse, a matmul's summation order), so the two may disagree
  within a few float32 spacings of a face; `margin_points` draws points that stay 1e-3 away from every face (|q| and
  h are of order one here: one spacing is ~1e-7, the two orders differ by a few times 1e-6 at most).
"""
import functools
import math

import numpy as np
import torch

f32 = np.float32


def rpy_matrix(roll, pitch, yaw):
    """Rz(yaw) Ry(pitch) Rx(roll) in float64: viser's ``SO3.from_rpy_radians`` (scene_box.py:98-108)."""
    cr, sr, cp, sp, cy, sy = (math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch), math.cos(yaw),
                              math.sin(yaw))
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]], np.float64)
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]], np.float64)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]], np.float64)
    return Rz @ Ry @ Rx


# the boxes of the tests, against means uniform in [-2, 2]^3: name -> (R, T, S)
BOXES = {
    "a": (np.eye(3), np.array([0.9, 0.0, 0.0]), np.array([2.2, 4.5, 4.5])),  # axis-aligned: x in (-0.2, 2): about half
    "b": (rpy_matrix(0.3, -0.7, 1.1), np.array([0.3, -0.2, 0.4]), np.array([1.5, 0.8, 2.5])),
    "c": (rpy_matrix(0.5, 0.2, -0.4) @ np.diag([1.0, 2.0, 0.5]), np.array([-0.2, 0.1, 0.3]),
          np.array([2.0, 1.5, 3.0])),  # a rotation times diag(1, 2, 0.5): not orthonormal
    "d": (np.eye(3), np.zeros(3), np.array([10.0, 10.0, 10.0])),  # everything
    "e": (np.eye(3), np.array([50.0, 50.0, 50.0]), np.array([1.0, 1.0, 1.0])),  # nothing
    "f": (np.eye(3), np.zeros(3), np.array([10.0, 0.0, 10.0])),  # S_y = 0: nothing
}


def crop_values(R, T, S):
    """float32[16]: A (3x4, row-major) | h | 0."""
    H = np.eye(4, dtype=np.float64)
    H[:3, :3] = np.asarray(R, np.float64)
    H[:3, 3] = np.asarray(T, np.float64)
    v = np.zeros(16, f32)
    v[:12] = np.linalg.inv(H)[:3].astype(f32).reshape(12)
    v[12:15] = (np.asarray(S, np.float64) / 2.0).astype(f32)
    return v


def q_f32(values, pts):
    """[N,3] float32: the box coordinates as the kernels evaluate them."""
    p = np.asarray(pts, f32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        cols = []
        for k in range(3):
            a = values[4 * k:4 * k + 4]
            cols.append(((a[0] * x + a[1] * y) + a[2] * z) + a[3])
    q = np.stack(cols, 1)
    assert q.dtype == f32
    return q


def within_f32(values, pts):
    q, h = q_f32(values, pts), values[12:15]
    with np.errstate(invalid="ignore"):
        return ((q > -h) & (q < h)).all(axis=1)


def q_reference(R, T, pts):
    """[N,3] float32 box coordinates by the reference's arithmetic (scene_box.py:83-96): the box frame as a float32
    4x4, inverted by ``torch.inverse`` in float32, applied to the homogeneous points [p, 1] as one matmul."""
    frame = np.eye(4, dtype=f32)
    frame[:3, :3] = np.asarray(R, np.float64).astype(f32)
    frame[:3, 3] = np.asarray(T, np.float64).astype(f32)
    to_box = torch.inverse(torch.from_numpy(frame))
    p = torch.from_numpy(np.asarray(pts, f32))
    homogeneous = torch.cat([p, torch.ones(p.shape[0], 1)], dim=1)
    return (to_box @ homogeneous.T).T[:, :3].numpy()


def within_reference(R, T, S, pts):
    """The mask of `OrientedBox.within` (scene_box.py:83-96), restated: `q_reference`, then strictly inside
    (-S / 2, S / 2) on every axis, the half extents in float32."""
    q = q_reference(R, T, pts)
    half = (torch.from_numpy(np.asarray(S, np.float64)).to(torch.float32) / 2).numpy()
    return ((q > -half) & (q < half)).all(axis=1)


def q_f64(R, T, S, pts):
    """(q [N,3], h [3]) in float64, from the float64 inverse."""
    H = np.eye(4, dtype=np.float64)
    H[:3, :3], H[:3, 3] = R, T
    A = np.linalg.inv(H)[:3]
    p = np.asarray(pts, np.float64)
    return p @ A[:, :3].T + A[:, 3], np.asarray(S, np.float64) / 2.0


def uniform_means(n, seed):
    return np.random.default_rng(seed).uniform(-2.0, 2.0, (n, 3)).astype(f32)


def margin_points(name, n, seed, margin=1e-3):
    """n float32 points uniform in [-2, 2]^3 with every | |q_k| - h_k | > margin (q in float64)."""
    R, T, S = BOXES[name]
    rng = np.random.default_rng(seed)
    out = np.zeros((0, 3), f32)
    while out.shape[0] < n:
        p = rng.uniform(-2.0, 2.0, (2 * n, 3)).astype(f32)
        q, h = q_f64(R, T, S, p)
        out = np.concatenate([out, p[(np.abs(np.abs(q) - h) > margin).all(axis=1)]])
    return out[:n]


def _search(values, k, target, rng, tries=40):
    """A float32 point whose q_k, evaluated as the kernels evaluate it, is exactly `target`, with the two other box
    coordinates well inside.  Starts from a point of the plane q_k = target (float64), rounds it, and looks among the
    13^3 float32 points within six spacings of it in every coordinate; a start without such a point (the partial sums
    of q_k may be coarser than the target) is dropped for another.  None when no start had one."""
    A = values[:12].astype(np.float64).reshape(3, 4)
    h = values[12:15].astype(np.float64)
    M = np.linalg.inv(A[:, :3])
    offs = np.arange(-6, 7).astype(f32)
    others = [i for i in range(3) if i != k]
    for _ in range(tries):
        q = rng.uniform(-0.8, 0.8, 3) * h
        q[k] = float(target)
        p = (M @ (q - A[:, 3])).astype(f32)
        axes = [p[c] + offs * np.spacing(np.abs(p[c])) for c in range(3)]
        grid = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3).astype(f32)
        qq = q_f32(values, grid)
        ok = (qq[:, k] == target) & (np.abs(qq[:, others[0]]) < 0.9 * h[others[0]]) \
            & (np.abs(qq[:, others[1]]) < 0.9 * h[others[1]])
        if ok.any():
            return grid[np.argmax(ok)].copy()
    return None  # (no float32 point evaluates to it: the last addition's spacing can step over a value)


def _neighbour(values, k, p, inward):
    """The float32 point next to `p` (which lies on a face of axis k) along the coordinate whose spacing moves q_k most:
    that coordinate moved by single spacings, inward or outward, until the float32 q_k leaves the face's value --
    one step, or a few where q_k is coarser than the coordinate."""
    A = values[:12].reshape(3, 4)
    j = int(np.argmax(np.abs(A[k, :3]) * np.spacing(np.abs(p))))  # (the coordinate whose one spacing moves q_k most)
    face = q_f32(values, p[None])[0, k]
    rise = (face < 0) == inward  # inward is towards zero: q_k rises from a negative face, falls from a positive one
    up = rise == (A[k, j] > 0)  # ... and the coordinate moves with it, or against it
    p = p.copy()
    for _ in range(64):
        p[j] = np.nextafter(p[j], f32(np.inf) if up else f32(-np.inf))
        if q_f32(values, p[None])[0, k] != face:
            return p
    raise AssertionError("q_k does not move")


@functools.lru_cache(maxsize=None)
def face_points(name):
    """For box `name` (extents > 0): 64 points exactly ON a face (q_k == +-h_k in float32: outside, the inequalities
    are strict), their 64 float32 neighbours just inside it and the 64 just outside (`_neighbour`: |q_k| within a few
    spacings of h_k, on the other side) -> (on, inside, outside, faces): float32 [64,3] each, and the (k, sign) of
    every row.  The faces cycle through k = 0, 1, 2 and both signs; a face whose value no float32 point evaluates to
    (a3 and the sum in front of it can be coarser than h_k) is left out -- at least three faces, of at least two
    axes, take part."""
    v = crop_values(*BOXES[name])
    rng = np.random.default_rng(sum(map(ord, name)) + 17)
    on, inside, outside, faces = [], [], [], []
    dead = set()
    i = 0
    while len(on) < 64:
        face = (i % 3, 1.0 if (i // 3) % 2 == 0 else -1.0)
        i += 1
        if face in dead:
            continue
        p = _search(v, face[0], f32(face[1]) * v[12 + face[0]], rng)
        if p is None:
            dead.add(face)
            assert len(dead) <= 3, "fewer than three faces can be hit exactly"
            continue
        on.append(p)
        inside.append(_neighbour(v, face[0], p, True))
        outside.append(_neighbour(v, face[0], p, False))
        faces.append(face)
    assert len({k for k, _ in faces}) >= 2
    return tuple(np.stack(a).astype(f32) for a in (on, inside, outside)) + (tuple(faces),)


@functools.lru_cache(maxsize=None)
def rule_points():
    """The point set of the exact-rule tests: 1000 uniform means, the face points of boxes a, b, c (on, and their float32 neighbours
    inside and outside), and a mean with a NaN in each coordinate -> float32 [N,3] (N is odd and no multiple
    of 256)."""
    parts = [uniform_means(1000, 3)]
    for name in ("a", "b", "c"):
        parts += list(face_points(name)[:3])
    nan = np.array([[np.nan, 0.1, 0.2], [0.1, np.nan, 0.2], [0.1, 0.2, np.nan]], f32)
    pts = np.concatenate(parts + [nan]).astype(f32)
    pts.setflags(write=False)
    return pts
