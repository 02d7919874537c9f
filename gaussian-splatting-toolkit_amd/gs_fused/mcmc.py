"""MCMC densification -- relocation of dead Gaussians, growth to a cap, position noise and the two L1
regularisers of "3D Gaussian Splatting as Markov Chain Monte Carlo" (Kheradmand et al. 2024; gsplat's
``MCMCStrategy``) -- over ``gsr_mcmc_*`` (include/gsraster.h, csrc/mcmc.hip).

A refinement is two phases, as gsplat orders them: *relocate* (N unchanged, the parameter tensors and their Adam
moments modified in place) and *add* (``min(cap_max, int(grow_factor * N)) - N`` new rows, host arithmetic).  Each
phase is a plan (opacities, integer sampling weights, their uint64 prefix sums, the draws) and one streaming launch
over all tensors.  Nothing is read back: how many rows were dead stays in a device tensor that ``info`` reads when
asked.  fp32 CUDA tensors only; no CPU fallback.
"""
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from rasterizer.cuda import _call, _check, _stream, _typed

from .refine import KIND_COPY, KIND_LOG_SCALES, KIND_MOMENT, MAX_TENSORS, PARAM_NAMES, _RefineTensor

_f32 = torch.float32
KIND_OPACITIES = 4
RELOCATE, ADD = 0, 1
MAX_RATIO = 51


@dataclass
class MCMCConfig:
    """gsplat's ``MCMCStrategy`` defaults (and the two regularisers of its trainer)."""
    cap_max: int = 1_000_000
    noise_lr: float = 5e5
    refine_start_iter: int = 500
    refine_stop_iter: int = 25_000
    refine_every: int = 100
    min_opacity: float = 0.005
    opacity_reg: float = 0.01
    scale_reg: float = 0.01
    grow_factor: float = 1.05


def mcmc_branch(cfg: MCMCConfig, step: int) -> bool:
    """Does a refinement take place at `step`?  Host arithmetic only."""
    return cfg.refine_start_iter < step < cfg.refine_stop_iter and step % cfg.refine_every == 0


def mcmc_num_new(cfg: MCMCConfig, n: int) -> int:
    """Rows the add phase appends to a model of `n`: ``max(0, min(cap_max, int(grow_factor * n)) - n)``."""
    return max(0, min(int(cfg.cap_max), int(cfg.grow_factor * n)) - n)


class MCMCInfo:
    """What a refinement did.  ``n_in``, ``n_out`` and ``added`` are host numbers; ``dead`` and ``relocated`` are read
    from the device when first asked for (``info["dead"]``, or ``counts()``): that read is the only synchronisation,
    and nothing in the refinement needs it.  ``plans``: the device tensors of each phase that ran (``opac``,
    ``prefix``, ``dead_index``, ``draw_source``, ``row_source``, ``counts``, ``totals``)."""

    def __init__(self, n_in: int):
        self.n_in = self.n_out = n_in
        self.added = 0
        self.plans: Dict[str, Dict[str, Tensor]] = {}
        self._host = None

    def counts(self) -> Dict[str, int]:
        if self._host is None:
            dead = relocated = 0
            plan = self.plans.get("relocate")
            if plan is not None:
                total, dead = (int(v) for v in plan["totals"].tolist())
                relocated = dead if total > 0 else 0
            self._host = {"dead": dead, "relocated": relocated, "added": self.added}
        return dict(self._host)

    def __getitem__(self, key: str):
        if key in ("n_in", "n_out", "added"):
            return getattr(self, key)
        return self.counts()[key]


def _check_model(params, moments):
    n = params["means"].shape[0]
    for k in PARAM_NAMES:
        _check(params[k], k, _f32)
        if params[k].shape[0] != n:
            raise ValueError(f"{k} has {params[k].shape[0]} rows, means has {n}")
    if params["scales"].shape != (n, 3) or params["quats"].shape != (n, 4) or params["means"].shape != (n, 3) \
            or params["opacities"].numel() != n:
        raise ValueError("expected means [N,3], scales [N,3], quats [N,4], opacities [N,1]")
    if moments is not None:
        for k, pair in moments.items():
            if pair is None:
                continue
            for m in pair:
                _check(m, f"Adam state of {k}", _f32)
                if m.shape != params[k].shape:
                    raise ValueError(f"Adam state of {k} has shape {tuple(m.shape)}, parameter {tuple(params[k].shape)}")
    return n


def _phase(params, moments, cfg: MCMCConfig, step: int, seed: int, phase: int, n_new: int, info: MCMCInfo):
    n = _check_model(params, moments)
    dev = params["means"].device
    new_params, new_moments = dict(params), (None if moments is None else dict(moments))
    if n == 0 or (phase == ADD and n_new <= 0):
        return new_params, new_moments
    n_out = n + (n_new if phase == ADD else 0)
    with torch.cuda.device(dev):
        i32 = dict(dtype=torch.int32, device=dev)
        plan = {"opac": torch.empty(n, dtype=_f32, device=dev), "prefix": torch.empty(n, dtype=torch.int64, device=dev),
                "dead_index": torch.empty(n, **i32), "draw_source": torch.empty(n if phase == RELOCATE else n_new, **i32),
                "row_source": torch.empty(n, **i32), "counts": torch.empty(n, **i32),
                "totals": torch.empty(2, dtype=torch.int64, device=dev)}
        wbytes = int(_typed().gsr_mcmc_workspace_bytes(n))
        work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
        scratch = torch.empty(4 * n, dtype=_f32, device=dev)
        _call("gsr_mcmc_plan", n, n_new if phase == ADD else 0, phase, params["opacities"], cfg.min_opacity,
              int(step) & 0xFFFFFFFF, int(seed) & (2**64 - 1), plan["opac"], plan["prefix"], plan["dead_index"],
              plan["draw_source"], plan["row_source"], plan["counts"], plan["totals"], work, wbytes, _stream(dev))
        items = []  # (in, out, width, kind)
        kinds = {"scales": KIND_LOG_SCALES, "opacities": KIND_OPACITIES}
        for k in PARAM_NAMES:
            t = params[k]
            out = t if phase == RELOCATE else torch.empty((n_out,) + tuple(t.shape[1:]), dtype=_f32, device=dev)
            new_params[k] = out
            w = t.numel() // n
            items.append((t, out, w, kinds.get(k, KIND_COPY)))
            if moments is not None and moments.get(k) is not None:
                outs = []
                for m in moments[k]:
                    o = m if phase == RELOCATE else torch.empty_like(out)
                    outs.append(o)
                    items.append((m, o, w, KIND_MOMENT))
                new_moments[k] = tuple(outs)
        items = [it for it in items if it[2] > 0]  # (`features_rest` of an SH-degree-0 model is [N, 0, 3]: nothing moves)
        if len(items) > MAX_TENSORS:
            raise ValueError(f"at most {MAX_TENSORS} tensors move in one refinement")
        arr = (_RefineTensor * len(items))()
        for j, (a, b, w, kind) in enumerate(items):
            arr[j] = _RefineTensor(a.data_ptr(), b.data_ptr(), w, kind)
        _call("gsr_mcmc_apply", n, n_out, plan["opac"], params["scales"], cfg.min_opacity, plan["row_source"],
              plan["draw_source"], plan["counts"], scratch, len(items), arr, _stream(dev))
    info.plans["relocate" if phase == RELOCATE else "add"] = plan
    info.n_out = n_out
    if phase == ADD:
        info.added = n_new
    return new_params, new_moments


@torch.no_grad()
def mcmc_relocate(params: Dict[str, Tensor], moments: Optional[Dict[str, Tuple[Tensor, Tensor]]], cfg: MCMCConfig,
                  step: int, seed: int = 0, info: Optional[MCMCInfo] = None):
    """The relocate phase alone: the input tensors (and moments) are modified in place and returned."""
    info = MCMCInfo(params["means"].shape[0]) if info is None else info
    p, m = _phase(params, moments, cfg, step, seed, RELOCATE, 0, info)
    return p, m, info


@torch.no_grad()
def mcmc_add(params: Dict[str, Tensor], moments: Optional[Dict[str, Tuple[Tensor, Tensor]]], cfg: MCMCConfig,
             step: int, seed: int = 0, n_new: Optional[int] = None, info: Optional[MCMCInfo] = None):
    """The add phase alone: new tensors of ``N + n_new`` rows (``mcmc_num_new`` by default); with nothing to add the
    inputs themselves."""
    n = params["means"].shape[0]
    info = MCMCInfo(n) if info is None else info
    p, m = _phase(params, moments, cfg, step, seed, ADD, mcmc_num_new(cfg, n) if n_new is None else int(n_new), info)
    return p, m, info


@torch.no_grad()
def mcmc_refine(params: Dict[str, Tensor], moments: Optional[Dict[str, Tuple[Tensor, Tensor]]], cfg: MCMCConfig,
                step: int, seed: int = 0):
    """One refinement: relocate, then add (which plans again on the relocated model).

    params / moments: as for ``refine_gaussians`` (the six raw parameter tensors; name -> ``(exp_avg, exp_avg_sq)``).
    Returns ``(new_params, new_moments, info)``.  When N does not change the input tensors themselves are returned,
    modified in place; otherwise new tensors of ``info.n_out`` rows.  Sources and destinations have zero moments.
    Whether `step` refines at all is the caller's ``mcmc_branch``.  No host synchronisation."""
    info = MCMCInfo(params["means"].shape[0])
    p, m = _phase(params, moments, cfg, step, seed, RELOCATE, 0, info)
    p, m = _phase(p, m, cfg, step, seed, ADD, mcmc_num_new(cfg, info.n_in), info)
    return p, m, info


@torch.no_grad()
def relocation(opacities: Tensor, scales: Tensor, ratios: Tensor, min_opacity: float = 0.0, raw: bool = False):
    """The relocation rule on its own: opacities [n] in (0,1), scales [n,3], ratios [n] int32 (clamped to [1, 51]) ->
    (new opacities, new scales), or with `raw` their logit / log."""
    _check(opacities, "opacities", _f32), _check(scales, "scales", _f32), _check(ratios, "ratios", torch.int32)
    n = opacities.numel()
    if scales.shape != (n, 3) or ratios.numel() != n:
        raise ValueError("expected opacities [n], scales [n,3], ratios [n]")
    out_o, out_s = torch.empty_like(opacities), torch.empty_like(scales)
    with torch.cuda.device(opacities.device):
        _call("gsr_mcmc_relocation", n, opacities, scales, ratios, min_opacity, int(raw), out_o, out_s,
              _stream(opacities.device))
    return out_o, out_s


@torch.no_grad()
def mcmc_inject_noise_(means: Tensor, log_scales: Tensor, raw_quats: Tensor, logits: Tensor, scaler: float,
                       seed: int, step: int, noise: Optional[Tensor] = None) -> Tensor:
    """``means += Sigma (eps * gate * scaler)`` in place, after the optimiser step: Sigma the Gaussian's covariance,
    gate = 1 / (1 + exp(-100 ((1 - opacity) - 0.995))), `scaler` = the means' learning rate * ``noise_lr``.  eps:
    `noise` [N,3], or from the counter-based generator keyed on (seed; Gaussian index, step)."""
    n = means.shape[0]
    for t, name in ((means, "means"), (log_scales, "log_scales"), (raw_quats, "raw_quats"), (logits, "logits")):
        _check(t, name, _f32)
    if means.shape != (n, 3) or log_scales.shape != (n, 3) or raw_quats.shape != (n, 4) or logits.numel() != n:
        raise ValueError("expected means [N,3], log_scales [N,3], raw_quats [N,4], logits [N,1]")
    if noise is not None:
        _check(noise, "noise", _f32)
        if noise.shape != (n, 3):
            raise ValueError("noise must be [N,3]")
    with torch.cuda.device(means.device):
        _call("gsr_mcmc_noise", n, means, log_scales, raw_quats, logits, scaler, int(step) & 0xFFFFFFFF,
              int(seed) & (2**64 - 1), noise, _stream(means.device))
    return means


class _MCMCRegularizer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, log_scales, opacity_reg, scale_reg):
        _check(logits, "logits", _f32), _check(log_scales, "log_scales", _f32)
        n = logits.numel()
        if n < 1 or log_scales.shape != (n, 3):
            raise ValueError("expected logits [N,1] and log_scales [N,3], N >= 1")
        dev = logits.device
        with torch.cuda.device(dev):
            out = torch.empty(3, dtype=torch.float64, device=dev)
            wbytes = int(_typed().gsr_mcmc_reg_workspace_bytes())
            work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
            _call("gsr_mcmc_reg_forward", n, logits, log_scales, opacity_reg, scale_reg, out, work, wbytes,
                  _stream(dev))
        ctx.save_for_backward(logits, log_scales)
        ctx.regs = (float(opacity_reg), float(scale_reg))
        return out[0].clone()

    @staticmethod
    def backward(ctx, v):
        logits, log_scales = ctx.saved_tensors
        v = v.to(torch.float64).contiguous()
        v_logits, v_log_scales = torch.empty_like(logits), torch.empty_like(log_scales)
        with torch.cuda.device(logits.device):
            _call("gsr_mcmc_reg_backward", logits.numel(), logits, log_scales, ctx.regs[0], ctx.regs[1], v, v_logits,
                  v_log_scales, _stream(logits.device))
        return v_logits, v_log_scales, None, None


def mcmc_regularizer(logits: Tensor, log_scales: Tensor, opacity_reg: float = 0.01, scale_reg: float = 0.01) -> Tensor:
    """``opacity_reg * mean(sigmoid(logits)) + scale_reg * mean(exp(log_scales))`` as a float64 scalar (float64 terms,
    summed in a fixed order); the gradients are float32 like the parameters."""
    return _MCMCRegularizer.apply(logits, log_scales, float(opacity_reg), float(scale_reg))
