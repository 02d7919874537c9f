"""Contribution-based pruning: per-Gaussian statistics of the blend weight over views, on csrc/contribution.hip
(the rule is stated in include/gsraster.h).  What RadSplat, LightGaussian and Mini-Splatting
score a Gaussian with:

    ContributionStats(n, device).accumulate(xys, depths, radii, conics, num_tiles_hit, opacities, H, W)
    view_contributions(xys, depths, radii, conics, num_tiles_hit, opacities, H, W)   -> the stats of one view
    prune_mask(stats, rule, threshold=None, keep=None, scales=None, power=0.1)       -> bool [N], True = keep
    prune_gaussians(params, moments, keep)                                           -> (new_params, new_moments)

With ``w = alpha T`` of a contributing (pixel, Gaussian) pair under the forward compositing's skip, clamp and stop rule:
``max_weight`` the largest w over pixels and views, ``weight_sum`` the sum of w (fixed point, 2^-24 units, truncated per
pair), ``hits`` the number of pairs, ``dominant`` the number of pixels in which the Gaussian has the largest w.  One walk
of its own over the tile lists the rasterizer's cache holds for the view, forward only, integer atomics only: every
array is bit-reproducible, deterministic mode included.  CUDA tensors and 16 x 16 tiles only; no CPU fallback for the
walk (``prune_mask`` and ``prune_gaussians`` are plain torch and take CPU tensors)."""
import math
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

_f32 = torch.float32
Q_ONE = float(1 << 24)  # one unit of `sum_q` is 2^-24
RULES = {"max_weight": 0.01, "weight_sum": None, "dominant": 1.0}  # rule -> default threshold (RadSplat's; a pixel)


class ContributionStats:
    """The four statistics [n] (zeros) and ``views``, the number of views accumulated."""

    def __init__(self, n: int, device):
        self.n, self.device, self.views = int(n), torch.device(device), 0
        self.max_w = torch.zeros(self.n, dtype=_f32, device=self.device)
        self.sum_q, self.hit_count, self.dominant_count = (
            torch.zeros(self.n, dtype=torch.int64, device=self.device) for _ in range(3))

    @torch.no_grad()
    def accumulate(self, xys: Tensor, depths: Tensor, radii: Tensor, conics: Tensor, num_tiles_hit: Tensor,
                   opacities: Tensor, img_height: int, img_width: int, block_width: int = 16) -> "ContributionStats":
        """Add the view whose projection outputs these are.  ``opacities`` is what the view's RGB pass composited with
        (for ``rasterize_mode="antialiased"``: the compensated ones).  Called after ``rasterize_gaussians`` for the same
        view, the tile lists are that call's (a cache hit).  A view with nothing on screen launches nothing and changes
        nothing but ``views``.

        ValueError, naming the op: ``block_width`` other than 16; CPU tensors; ``n`` that disagrees with the inputs."""
        if int(block_width) != 16:
            raise ValueError(f"ContributionStats.accumulate: block_width must be 16 (the walk is written for 16 x 16 "
                             f"tiles), got {block_width}")
        for name, t in (("xys", xys), ("depths", depths), ("radii", radii), ("conics", conics),
                        ("num_tiles_hit", num_tiles_hit), ("opacities", opacities)):
            if not isinstance(t, Tensor):
                raise RuntimeError(f"ContributionStats.accumulate: {name} must be a tensor")
            if not t.is_cuda:
                raise ValueError(f"ContributionStats.accumulate: {name} is a CPU tensor; the walk runs on CUDA tensors "
                                 f"only (no CPU fallback)")
        if not self.max_w.is_cuda:
            raise ValueError("ContributionStats.accumulate: the statistics are CPU tensors; the walk runs on CUDA "
                             "tensors only (no CPU fallback)")
        if xys.shape[0] != self.n or opacities.numel() != self.n:
            raise ValueError(f"ContributionStats.accumulate: n = {self.n}, but xys holds {xys.shape[0]} Gaussians and "
                             f"opacities {opacities.numel()} values")
        H, W = int(img_height), int(img_width)
        if H < 1 or W < 1:
            raise ValueError("ContributionStats.accumulate: empty image")
        import rasterizer.cuda as _C
        from rasterizer import rasterize as _R

        tile_bounds = ((W + 15) // 16, (H + 15) // 16, 1)
        xy, co, op = (t.detach().contiguous() for t in (xys, conics, opacities))

        def composite(ids, bins):
            # The view's own arrays: `composite_lists` walks lists that were sized on the device, or cached and then
            # found stale, a second time, and a walk that adds cannot be repeated.  The native entry itself adds in
            # place (rasterizer.cuda.contribution_accumulate, for callers that hold finished lists)
            max_w = torch.zeros(self.n, dtype=_f32, device=xy.device)
            counts = torch.zeros((3, self.n), dtype=torch.int64, device=xy.device)
            _C.contribution_accumulate(tile_bounds, (W, H, 1), ids, bins, xy, co, op, max_w, counts[0], counts[1],
                                       counts[2])
            return max_w, counts

        # single-segment lists, as gs_fused.depth_distortion takes them (two-segment lists are built again as one)
        # (the tensors as given: the cache recognises the RGB pass's inputs by identity)
        _, outputs = _R.composite_lists(xys, depths, radii, conics, num_tiles_hit, opacities, H, W, 16, composite,
                                        round1=None)
        if outputs is not None:  # (None: nothing on screen, no launch)
            max_w, counts = outputs
            torch.maximum(self.max_w, max_w, out=self.max_w)
            self.sum_q += counts[0]
            self.hit_count += counts[1]
            self.dominant_count += counts[2]
        self.views += 1
        return self

    @property
    def max_weight(self) -> Tensor:
        return self.max_w

    @property
    def weight_sum(self) -> Tensor:
        return self.sum_q.to(torch.float64) / Q_ONE

    @property
    def hits(self) -> Tensor:
        return self.hit_count

    @property
    def dominant(self) -> Tensor:
        return self.dominant_count


def view_contributions(xys: Tensor, depths: Tensor, radii: Tensor, conics: Tensor, num_tiles_hit: Tensor,
                       opacities: Tensor, img_height: int, img_width: int, block_width: int = 16) -> ContributionStats:
    """-> the `ContributionStats` of one view (see `ContributionStats.accumulate`)."""
    return ContributionStats(xys.shape[0], xys.device).accumulate(xys, depths, radii, conics, num_tiles_hit, opacities,
                                                                  img_height, img_width, block_width)


def _prune_score(stats, rule: str, scales: Optional[Tensor] = None, power: float = 0.1) -> Tensor:
    """The score [N] of a rule (larger = more important): the statistic in its own type (a threshold is compared in
    it: float32 0.01 is not below 0.01), float64 for "weight_sum"."""
    if rule not in RULES:
        raise ValueError(f"prune_mask: unknown rule {rule!r}; known: {sorted(RULES)}")
    if rule == "max_weight":
        return stats.max_weight
    if rule == "dominant":
        return stats.dominant
    if scales is None:
        raise ValueError("prune_mask: rule 'weight_sum' needs `scales` ([N,3], the world-space scales: exp of the "
                         "model's log-scales) for LightGaussian's volume factor")
    vol = scales.detach().to(torch.float64).prod(dim=-1)
    if vol.shape != stats.weight_sum.shape:
        raise ValueError(f"prune_mask: scales must be [N,3] with N = {stats.weight_sum.shape[0]}, got "
                         f"{tuple(scales.shape)}")
    # (the 90 % quantile as the value at rank ceil(0.9 N) of the sorted volumes: torch.quantile refuses large N)
    q90 = vol.sort().values[max(0, math.ceil(0.9 * vol.numel()) - 1)] if vol.numel() else vol.new_ones(())
    v = torch.clamp(vol / q90, 0.0, 1.0)
    return stats.weight_sum.to(v.device) * v ** power


def prune_mask(stats, rule: str = "max_weight", threshold: Optional[float] = None, keep: Optional[float] = None,
               scales: Optional[Tensor] = None, power: float = 0.1) -> Tensor:
    """-> bool [N], True where the Gaussian stays.  ``stats``: a `ContributionStats`, or anything with its four
    properties (CPU tensors too).  Rules and their scores:

        "max_weight"   max_weight (RadSplat); default threshold 0.01
        "weight_sum"   weight_sum * v^power, v = clamp(prod(scales) / q90(prod(scales)), 0, 1) (LightGaussian's volume
                       factor); needs ``scales``; no default threshold
        "dominant"     dominant (Mini-Splatting: the pixels a Gaussian wins); default threshold 1

    ``threshold`` removes ``score < threshold``; ``keep`` (a fraction in (0, 1]) keeps the ``ceil(keep N)`` best, ties
    going to the lower index (a stable sort), so the mask is a pure function of the statistics.  At most one of the two;
    neither: the rule's default threshold."""
    if threshold is not None and keep is not None:
        raise ValueError("prune_mask: give `threshold` or `keep`, not both")
    score = _prune_score(stats, rule, scales, power)
    if keep is not None:
        if not (0.0 < float(keep) <= 1.0):
            raise ValueError(f"prune_mask: keep must be a fraction in (0, 1], got {keep}")
        n = score.numel()
        k = min(n, math.ceil(float(keep) * n))
        order = torch.sort(score, descending=True, stable=True).indices
        mask = torch.zeros(n, dtype=torch.bool, device=score.device)
        mask[order[:k]] = True
        return mask
    if threshold is None:
        threshold = RULES[rule]
        if threshold is None:
            raise ValueError(f"prune_mask: rule {rule!r} has no default threshold; give `threshold` or `keep`")
    return score >= float(threshold)


def prune_gaussians(params: Dict[str, Tensor], moments: Optional[Dict[str, Tuple[Tensor, Tensor]]],
                    keep: Tensor) -> Tuple[Dict[str, Tensor], Dict[str, Tuple[Tensor, Tensor]]]:
    """The rows ``keep`` (bool [N]) of the six parameter tensors and of both Adam moments of each that has them ->
    ``(new_params, new_moments)``, the shapes `gs_fused.swap_parameters` installs.  A row gather by torch indexing: it
    runs a handful of times per training."""
    from .refine import PARAM_NAMES

    n = params["means"].shape[0]
    if keep.dtype != torch.bool or tuple(keep.shape) != (n,):
        raise ValueError(f"prune_gaussians: keep must be bool [{n}], got {keep.dtype} {tuple(keep.shape)}")
    with torch.no_grad():
        rows = torch.nonzero(keep.to(params["means"].device)).reshape(-1)
        new = {k: params[k].detach()[rows].contiguous() for k in PARAM_NAMES}
        new_moments = {k: tuple(m[rows].contiguous() for m in pair) for k, pair in (moments or {}).items()
                       if pair is not None}
    return new, new_moments
