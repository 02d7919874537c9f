"""k nearest neighbours among 3-D points on the GPU, and what the toolkit's models make of them: the initial scale of
every Gaussian is the log of the mean distance to its three nearest seeds (`populate_modules`, vanilla_gs.py:136-140,
through scikit-learn's `NearestNeighbors` in `k_nearest_sklearn`, :260-280).  The rule is stated in include/gsraster.h
(DESIGN.md section 4.9); HIP kernels behind `gsr_knn_build` / `gsr_knn_query` (csrc/knn.hip); torch for memory and
streams only; no CPU path.
"""
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from rasterizer.cuda import _check, _on, _stream, _typed

_f32, _i32 = torch.float32, torch.int32
GSR_ERANGE = -4
EXHAUSTIVE, SELF = 1, 2
MAX_K = 16
BYTES_TREE, BYTES_BUILD, BYTES_QUERY = range(3)


def _bytes(what: int, n: int, m: int, k: int = 1) -> int:
    b = _typed().gsr_knn_workspace_bytes(what, n, m, k)
    if b == 0:
        raise ValueError(f"{n} points / {m} queries / k = {k}: too large, or a size query failed (no device?)")
    return b


def _space(workspace: Optional[Tensor], nbytes: int, dev) -> Tensor:
    """A fresh workspace, or the one handed in (the tests hand in pre-filled ones)."""
    if workspace is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if workspace.numel() < nbytes or workspace.device != dev or workspace.dtype != torch.uint8:
        raise RuntimeError(f"workspace must hold {nbytes} bytes on {dev}")
    return workspace


def _points(t, name: str) -> Tensor:
    """float32 CUDA [n,3]; a non-contiguous view is copied."""
    if not isinstance(t, Tensor):
        raise RuntimeError(f"{name} must be a tensor")
    if t.dim() != 2 or t.size(1) != 3:
        raise RuntimeError(f"{name} must be [n,3]")
    return _check(t if t.is_contiguous() or not t.is_cuda else t.contiguous(), name, _f32)


class KNN:
    """Reference points (float32 [n,3]) built into a tree once and queried many times.  Points with a non-finite
    coordinate are left out and counted in `skipped_points`; `usable` are the rest.  n = 0 raises ValueError."""

    def __init__(self, points: Tensor, _tree: Optional[Tensor] = None, _workspace: Optional[Tensor] = None):
        points = _points(points, "points")
        n = points.size(0)
        if n == 0:
            raise ValueError("no reference points")
        self.points, self.device, self.num_points = points, points.device, n
        self.invalid_queries = None
        dev = self.device
        with _on(dev):
            self._tree = _space(_tree, _bytes(BYTES_TREE, n, 0), dev)
            ws = _space(_workspace, _bytes(BYTES_BUILD, n, 0), dev)
            state = torch.empty(4, dtype=_i32, device=dev)
            L = _typed()
            rc = L.gsr_knn_build(n, points, self._tree, self._tree.numel(), ws, ws.numel(), state, _stream(dev))
            if rc != 0:
                raise RuntimeError(f"gsr_knn_build failed ({rc}): {L.gsr_last_error().decode()}")
            self.usable, self.skipped_points = (int(v) for v in state[:2].tolist())

    def query(self, queries: Optional[Tensor] = None, k: int = 3, exhaustive: bool = False,
              _workspace: Optional[Tensor] = None, _out=None) -> Tuple[Tensor, Tensor]:
        """-> (dist float32 [m,k] ascending, idx int32 [m,k]).  `queries=None`: every reference point against the
        others (row i never returns i).  Ties in distance go to the smaller index.  A non-finite query gets NaN / -1;
        their number is left in `invalid_queries` (a device tensor: reading it synchronises).  Fewer than k usable
        reference points (k + 1 without queries) raise ValueError.  `exhaustive`: every query against every point
        instead of the tree walk -- the on-device cross-check, never chosen automatically."""
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
        self_mode = queries is None
        q = self.points if self_mode else _points(queries, "queries")
        if q.device != self.device:
            raise RuntimeError("queries and the reference points must be on one device")
        m, dev = q.size(0), self.device
        flags = (EXHAUSTIVE if exhaustive else 0) | (SELF if self_mode else 0)
        with _on(dev):
            if _out is not None:
                dist, idx = _out
            else:
                dist = torch.empty((m, k), dtype=_f32, device=dev)
                idx = torch.empty((m, k), dtype=_i32, device=dev)
            ws = None if exhaustive or m == 0 else _space(_workspace, _bytes(BYTES_QUERY, 0, m, k), dev)
            state = torch.zeros(4, dtype=_i32, device=dev)
            L = _typed()
            # (no queries: the three [m, ...] tensors are empty and go as NULL)
            rc = L.gsr_knn_query(self.num_points, self._tree, self._tree.numel(), self.usable, m,
                                 None if q.numel() == 0 else q, k, flags, ws, 0 if ws is None else ws.numel(),
                                 None if dist.numel() == 0 else dist, None if idx.numel() == 0 else idx, state,
                                 _stream(dev))
            if rc == GSR_ERANGE:
                raise ValueError(L.gsr_last_error().decode())
            if rc != 0:
                raise RuntimeError(f"gsr_knn_query failed ({rc}): {L.gsr_last_error().decode()}")
            self.invalid_queries = state[2]
        return dist, idx


def knn(points: Tensor, k: int = 3, queries: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """The one-call form: (dist [m,k], idx [m,k]) of `queries` (None: the points themselves, self left out)."""
    return KNN(points).query(queries, k)


def knn_mean_distance(points: Tensor, k: int = 3) -> Tensor:
    """float32 [n]: mean distance of every point to its k nearest others, formed in float32 as the reference forms
    it (`distances.mean(dim=-1)` on the float32 distances, vanilla_gs.py:139)."""
    return knn(points, k)[0].mean(dim=-1)


def initial_log_scales(points: Tensor, k: int = 3, floor: float = 0.0) -> Tensor:
    """float32 [n,3]: log(max(mean distance to the k nearest, floor)) on all three axes -- the scales `populate_modules`
    starts from.  With floor = 0 duplicate seeds give -inf, as in the reference."""
    avg = knn_mean_distance(points, k)
    if floor > 0:
        avg = avg.clamp_min(floor)
    return torch.log(avg)[:, None].repeat(1, 3)


def k_nearest(x: Tensor, k: int):
    """`k_nearest_sklearn`'s signature and return types (vanilla_gs.py:260-280): two float32 NumPy arrays [n,k], the
    distances and the indices (as float32, like the source).  `x` on any device; the search runs on the GPU."""
    dev = x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device())
    dist, idx = knn(x.detach().to(dev, _f32), k)
    return dist.cpu().numpy(), idx.cpu().numpy().astype(np.float32)
