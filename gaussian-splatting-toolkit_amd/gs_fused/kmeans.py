"""Lloyd's k-means on csrc/kmeans.hip (the rule is stated in include/gsraster.h): what builds
the codebook of the spherical-harmonics rows of a compressed export (gs_io.compressed).

    kmeans_assign(points, centroids)                   -> (labels int32 [N], dist float32 [N])
    kmeans_update(points, labels, centroids, weights)  -> (centroids float32 [K,D], counts int32 [K])
    kmeans_inertia(points, centroids, labels, weights) -> 0-dim float64 tensor on the device
    kmeans(points, k, iters=10, seed=0, ...)           -> KMeansResult(centroids, labels, counts, inertia)

points are float32 [N,D] with 1 <= D <= 48, centroids float32 [K,D] with 1 <= K <= 65536.  The assignment is float32,
every operation rounded on its own in index order, ties to the lowest index: bit for bit what
tests/kmeans_reference.py restates.  The update and the inertia sum in float64 in a fixed order without atomics:
bit-reproducible from run to run.  CUDA tensors only (no CPU fallback); nothing is read back to the host.
"""
from typing import NamedTuple, Optional, Tuple

import torch
from torch import Tensor

_f32, _i32, _f64 = torch.float32, torch.int32, torch.float64
MAX_DIM = 48            # GSR_KMEANS_MAX_DIM
MAX_CLUSTERS = 65536    # GSR_KMEANS_MAX_CLUSTERS
TILE = 128              # GSR_KMEANS_TILE: centroid rows per LDS tile of the assignment
INERTIA_SHARE = 1024    # GSR_KMEANS_INERTIA_SHARE: points per workgroup, one float64 of workspace each


class KMeansResult(NamedTuple):
    centroids: Tensor  # float32 [K,D]
    labels: Tensor     # int32 [N]: exactly kmeans_assign(points, centroids)[0]
    counts: Tensor     # int32 [K]: members per cluster under `labels`
    inertia: Tensor    # float64 [iters+1]: after each assignment


def _matrix(t, op: str, name: str, cols: Optional[int] = None) -> None:
    if not isinstance(t, Tensor):
        raise ValueError(f"{op}: {name} must be a tensor")
    if not t.is_cuda:
        raise ValueError(f"{op}: {name} is a CPU tensor; this op runs on CUDA tensors only (no CPU fallback)")
    if t.dtype != _f32 or t.dim() != 2 or (cols is not None and t.shape[1] != cols):
        want = "D" if cols is None else str(cols)
        raise ValueError(f"{op}: {name} must be float32 [*,{want}], got {t.dtype} {tuple(t.shape)}")


def _points(points, op: str) -> None:
    _matrix(points, op, "points")
    d = points.shape[1]
    if not 1 <= d <= MAX_DIM:
        raise ValueError(f"{op}: points have D = {d} columns; 1 <= D <= {MAX_DIM}")


def _centroids(centroids, points: Tensor, op: str) -> None:
    _matrix(centroids, op, "centroids", points.shape[1])
    k = centroids.shape[0]
    if k < 1:
        raise ValueError(f"{op}: K = {k}; need K >= 1")
    if k > MAX_CLUSTERS:
        raise ValueError(f"{op}: K = {k}; K <= {MAX_CLUSTERS}")
    if centroids.device != points.device:
        raise ValueError(f"{op}: centroids is on {centroids.device}, points on {points.device}")


def _vector(t, op: str, name: str, dtype, points: Tensor) -> None:
    if not isinstance(t, Tensor):
        raise ValueError(f"{op}: {name} must be a tensor")
    if not t.is_cuda:
        raise ValueError(f"{op}: {name} is a CPU tensor; this op runs on CUDA tensors only (no CPU fallback)")
    if t.dtype != dtype or tuple(t.shape) != (points.shape[0],):
        raise ValueError(f"{op}: {name} must be {dtype} [{points.shape[0]}], got {t.dtype} {tuple(t.shape)}")
    if t.device != points.device:
        raise ValueError(f"{op}: {name} is on {t.device}, points on {points.device}")


def _weights(weights, op: str, points: Tensor, validate: bool) -> Optional[Tensor]:
    """`validate`: the one read-back of a call from outside the loop (`kmeans` checks once, before it)."""
    if weights is None:
        return None
    _vector(weights, op, "weights", _f32, points)
    weights = weights.detach().contiguous()
    if validate and weights.numel() and not bool((torch.isfinite(weights) & (weights >= 0)).all()):
        raise ValueError(f"{op}: weights must be finite and >= 0")
    return weights


@torch.no_grad()
def kmeans_assign(points: Tensor, centroids: Tensor) -> Tuple[Tensor, Tensor]:
    """-> (labels int32 [N], dist float32 [N]): per row the nearest centroid under the float32 rule of
    include/gsraster.h and its squared distance; ties to the lowest index; a row whose distances are all NaN or +inf
    keeps label 0 and dist +inf.  One launch on the current stream (``gsr_kmeans_assign``); N = 0 launches nothing.

    ValueError, before the library is entered: CPU tensors, dtypes other than float32, wrong shapes, D > 48, K > 65536,
    K < 1, tensors on different devices."""
    op = "kmeans_assign"
    _points(points, op)
    _centroids(centroids, points, op)
    n, d = points.shape
    dev = points.device
    labels = torch.empty(n, dtype=_i32, device=dev)
    dist = torch.empty(n, dtype=_f32, device=dev)
    if n == 0:
        return labels, dist
    from rasterizer.cuda import _call, _stream

    with torch.cuda.device(dev):
        _call("gsr_kmeans_assign", n, d, centroids.shape[0], points.detach().contiguous(),
              centroids.detach().contiguous(), labels, dist, _stream(dev))
    return labels, dist


def _update(points: Tensor, labels: Tensor, centroids: Tensor, weights: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    from rasterizer.cuda import _call, _stream

    n, d = points.shape
    k, dev = centroids.shape[0], points.device
    with torch.cuda.device(dev):
        # plumbing: the stable sort of 0..N-1 by label and the segment starts (searchsorted: no read-back, and a label
        # outside [0, K) falls outside every segment)
        sorted_labels, order = torch.sort(labels, stable=True)
        offsets = torch.searchsorted(sorted_labels, torch.arange(k + 1, dtype=_i32, device=dev), out_int32=True)
        new = torch.empty_like(centroids)
        counts = torch.empty(k, dtype=_i32, device=dev)
        _call("gsr_kmeans_update", n, d, k, points, labels, order.to(_i32), offsets, weights, centroids, new, counts,
              _stream(dev))
    return new, counts


@torch.no_grad()
def kmeans_update(points: Tensor, labels: Tensor, centroids: Tensor, weights: Optional[Tensor] = None
                  ) -> Tuple[Tensor, Tensor]:
    """-> (centroids float32 [K,D], counts int32 [K]): per cluster the (weighted) mean of its members, summed in
    float64 in a fixed order and rounded to float32 once; a cluster without a member, or whose weights sum to zero,
    keeps the bits of its row of ``centroids``.  ``labels`` int32 [N] (a label outside [0, K) belongs to no cluster),
    ``weights`` float32 [N], finite and >= 0 (one read-back checks them).  A stable sort, a search and one launch on
    the current stream (``gsr_kmeans_update``); bit-reproducible.

    ValueError, before the library is entered: as `kmeans_assign`, labels that are not int32 [N], bad weights."""
    op = "kmeans_update"
    _points(points, op)
    _centroids(centroids, points, op)
    _vector(labels, op, "labels", _i32, points)
    weights = _weights(weights, op, points, validate=True)
    return _update(points.detach().contiguous(), labels.contiguous(), centroids.detach().contiguous(), weights)


def _inertia(points: Tensor, centroids: Tensor, labels: Tensor, weights: Optional[Tensor], out: Tensor) -> Tensor:
    from rasterizer.cuda import _call, _stream

    n, d = points.shape
    dev = points.device
    with torch.cuda.device(dev):
        workspace = torch.empty(max(1, -(-n // INERTIA_SHARE)), dtype=_f64, device=dev)
        _call("gsr_kmeans_inertia", n, d, centroids.shape[0], points, centroids, labels, weights, out, workspace,
              _stream(dev))
    return out


@torch.no_grad()
def kmeans_inertia(points: Tensor, centroids: Tensor, labels: Tensor, weights: Optional[Tensor] = None) -> Tensor:
    """-> 0-dim float64 tensor on the device: ``sum_i w_i |x_i - c_{l_i}|^2`` with every operation in float64, summed
    in a fixed order without atomics (bit-reproducible); not read back.  The quantity Lloyd's iteration decreases --
    the float32 ``dist`` of `kmeans_assign` is what chooses, this is what is measured.  Two launches
    (``gsr_kmeans_inertia``).  ValueError as `kmeans_update`."""
    op = "kmeans_inertia"
    _points(points, op)
    _centroids(centroids, points, op)
    _vector(labels, op, "labels", _i32, points)
    weights = _weights(weights, op, points, validate=True)
    out = torch.zeros(1, dtype=_f64, device=points.device)
    if points.shape[0] == 0:
        return out[0]
    return _inertia(points.detach().contiguous(), centroids.detach().contiguous(), labels.contiguous(), weights,
                    out)[0]


def initial_centroids(points: Tensor, k: int, seed: int = 0) -> Tensor:
    """``points[torch.randperm(N, generator=<CPU generator seeded with seed>)[:k]]``: the same rows on every device."""
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    pick = torch.randperm(points.shape[0], generator=gen)[:k]
    return points[pick.to(points.device)].contiguous()


@torch.no_grad()
def kmeans(points: Tensor, k: int, *, iters: int = 10, seed: int = 0, init: Optional[Tensor] = None,
           weights: Optional[Tensor] = None) -> KMeansResult:
    """Lloyd's iteration: (assign, update) ``iters`` times, then a final assign, so that ``labels`` are exactly
    ``kmeans_assign(points, centroids)[0]``; ``inertia[t]`` (float64, `kmeans_inertia`, with the weights) is recorded
    after each assign, ``counts`` are the members under the final labels.  ``k`` is cut to ``min(k, N)``.
    ``init`` float32 [k,D], or None: `initial_centroids` (distinct rows of ``points`` drawn by a seeded CPU generator).
    ``weights`` float32 [N], finite and >= 0, weigh the centroid means and the inertia, not the assignment.  The
    loop makes no host read-back (the weights are checked once, before it); bit-reproducible.  N = 0: empty results,
    no launch.

    ValueError, before the library is entered: as `kmeans_assign`; ``k < 1``, ``k > 65536``, ``iters < 0``, an ``init``
    that is not float32 [min(k, N), D] on the points' device, bad weights."""
    op = "kmeans"
    if int(k) != k or k < 1:
        raise ValueError(f"{op}: K = {k}; need K >= 1")
    if k > MAX_CLUSTERS:
        raise ValueError(f"{op}: K = {k}; K <= {MAX_CLUSTERS}")
    if int(iters) != iters or iters < 0:
        raise ValueError(f"{op}: iters = {iters}; need iters >= 0")
    _points(points, op)
    n, d = points.shape
    dev = points.device
    k, iters = min(int(k), n), int(iters)
    weights = _weights(weights, op, points, validate=True)
    if init is not None:
        _matrix(init, op, "init", d)
        if init.shape[0] != k or init.device != dev:
            raise ValueError(f"{op}: init must be float32 [{k},{d}] on {dev}, got {tuple(init.shape)} on {init.device}")
    if n == 0:
        return KMeansResult(torch.empty((0, d), dtype=_f32, device=dev), torch.empty(0, dtype=_i32, device=dev),
                            torch.empty(0, dtype=_i32, device=dev), torch.zeros(iters + 1, dtype=_f64, device=dev))
    points = points.detach().contiguous()
    centroids = initial_centroids(points, k, seed) if init is None else init.detach().contiguous().clone()
    inertia = torch.zeros(iters + 1, dtype=_f64, device=dev)
    for t in range(iters):
        labels, _ = kmeans_assign(points, centroids)
        _inertia(points, centroids, labels, weights, inertia[t:t + 1])
        centroids, _ = _update(points, labels, centroids, weights)
    labels, _ = kmeans_assign(points, centroids)
    _inertia(points, centroids, labels, weights, inertia[iters:iters + 1])
    counts = torch.searchsorted(torch.sort(labels).values, torch.arange(k + 1, dtype=_i32, device=dev),
                                out_int32=True).diff()
    return KMeansResult(centroids, labels, counts.to(_i32), inertia)


__all__ = ["KMeansResult", "MAX_CLUSTERS", "MAX_DIM", "TILE", "initial_centroids", "kmeans", "kmeans_assign",
           "kmeans_inertia", "kmeans_update"]
