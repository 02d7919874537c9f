"""One render op: what ``GaussianSplattingModel.get_outputs`` does between the raw
parameters and the images, as a single autograd node.

The toolkit's models (gs_toolkit/models/vanilla_gs.py:765-857, depth_gs.py:225-363) run,
per view: exp / normalise / sigmoid, the view directions, ``torch.cat`` of the SH
features, ``project_gaussians``, ``spherical_harmonics``, ``clamp(+0.5)``,
``rasterize_gaussians`` (and a second one for depth) -- ~25 torch ops and four custom
autograd nodes, each with its own saved-tensor bookkeeping.  ``render_gaussians`` chains
the same native calls (include/gsraster.h) inside ONE ``torch.autograd.Function``:

  forward : gsr_activate_forward -> gsr_project_forward (_aa: `ViewSpec.rasterize_mode`; _crop: `crop=`) -> gsr_sh_forward_split (+0.5,
            clamp) -> count_reach / depth_order / bin_sorted_dev -> gsr_rasterize_forward
            (or _rgbd: RGB + depth from one compositing pass)
  backward: gsr_rasterize_backward(_rgbd) -> gsr_sh_backward_split -> gsr_project_backward
            -> gsr_activate_backward, and the densification statistics of ``after_train``
            (vanilla_gs.py:344-372) straight from the screen-space gradient.

Nothing in it reads device memory back: the tile lists are sized by ``capacity`` (the
caller's job: `ListCapacity` below keeps a running estimate and checks the real count one
view later), which makes the whole view -- forward, loss, backward -- capturable in a HIP
graph (`ViewGraph`).  Under ``rasterizer.rasterize.set_deterministic(True)`` the compositing backward is
``gsr_rasterize_backward_det`` (a fixed summation order instead of float atomics: bit-identical gradients from run to
run, about 1.4x its time, one more list build per view), still without a read-back.  Same values as the separate ops (tests/test_gpu_render.py): images
bit-identical, gradients equal up to the order of the float atomics.
fp32 CUDA tensors; 16x16 tiles; SH degree 0-3 storage (K = 1, 4, 9, 16).
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, Optional

import torch
from torch import Tensor
from torch.autograd import Function

import rasterizer.cuda as _C
from rasterizer.cuda import _call, _stream

_f32, _i32 = torch.float32, torch.int32
BLOCK = 16


def _deterministic() -> bool:
    from rasterizer.rasterize import is_deterministic  # (imported late: rasterizer.rasterize imports its siblings)

    return is_deterministic()


class _ViewDesc(C.Structure):  # gsr_view_desc (include/gsraster.h)
    _fields_ = ([(k, C.c_int) for k in ("num_points", "sh_degree", "sh_degree_to_use", "render_depth", "img_height",
                                        "img_width")]
                + [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "glob_scale", "clip_thresh")]
                + [(k, C.c_int) for k in ("capacity", "deep_tile_threshold")]
                + [(k, C.c_void_p) for k in ("means", "log_scales", "raw_quats", "logits", "features_dc", "features_rest",
                                             "viewmat", "projmat", "campos", "background", "scales", "quats", "opac",
                                             "dirs", "cov3d", "xys", "depths", "radii", "conics", "comp", "tiles",
                                             "colors", "reach_records", "counts", "order", "cum", "ids", "tile_bins",
                                             "count_out", "sort_ws")]
                + [("sort_ws_bytes", C.c_size_t), ("bin_ws", C.c_void_p), ("bin_ws_bytes", C.c_size_t)]
                + [(k, C.c_void_p) for k in ("out_img", "out_depth", "final_Ts", "final_idx", "out_alpha", "zero_ptr")]
                + [("zero_bytes", C.c_size_t), ("segments", C.c_int), ("segment_min_entries", C.c_int),
                   ("seg_ws", C.c_void_p), ("seg_ws_bytes", C.c_size_t)]
                + [("antialiased", C.c_int), ("opac_aa", C.c_void_p)])


class _ViewGrads(C.Structure):  # gsr_view_grads
    _fields_ = ([(k, C.c_void_p) for k in ("v_img", "v_alpha", "v_depth", "accumulators")]
                + [("accumulators_zeroed", C.c_int), ("stats_first", C.c_void_p), ("stats_inv_size", C.c_float)]
                + [(k, C.c_void_p) for k in ("xys_grad_norm", "vis_counts", "max_2dsize", "tmp_v_cov2d", "tmp_v_cov3d",
                                             "tmp_v_scales", "tmp_v_quats", "v_means", "v_log_scales", "v_raw_quats",
                                             "v_logits", "v_dc", "v_rest")]
                + [("accumulators_final", C.c_int), ("v_xy_abs", C.c_void_p)])


def _segments(spec, capacity, dev):
    """(segments, minimum entries, workspace tensor or None) of the view's compositing
    (rasterizer.cuda.depth_segments).  The workspace is scratch of ONE call; the caller keeps the tensor until the
    call has been issued."""
    tb = spec.tile_bounds
    return _C._forward_segments(capacity, tb[0] * tb[1], spec.height, spec.width, dev)


def _segments_backward(spec, capacity, dev):
    """The backward's runs (not capped by GSR_DEPTH_SEGMENTS_FWD) and its workspace of (runs - 1) maps per pixel."""
    tb = spec.tile_bounds
    segs, seg_min = _C.depth_segments(capacity, tb[0] * tb[1])
    if segs < 2:
        return 0, 0, None
    return segs, seg_min, torch.empty(((segs - 1) * spec.height * spec.width * 8,), dtype=torch.uint8, device=dev)


def _seg_fields(seg):
    segs, seg_min, ws = seg
    if ws is None:
        return 0, 0, None, 0
    return segs, seg_min, ws.data_ptr(), ws.numel()


_ws_bytes_cache = {}


def _workspace_bytes(n, capacity, tb):
    key = (n, capacity, tb[0], tb[1])
    v = _ws_bytes_cache.get(key)
    if v is None:
        lib = _C._typed()
        v = (int(lib.gsr_depth_order_workspace_bytes(n, 1)),
             int(lib.gsr_bin_sorted_workspace_bytes(n, capacity, tb[0], tb[1])),
             int(lib.gsr_reach_record_bytes()),
             not _C.lists_need_counts(n, capacity, tb, device_sized=True))
        if len(_ws_bytes_cache) > 64:
            _ws_bytes_cache.clear()
        _ws_bytes_cache[key] = v
    return v


@dataclass(frozen=True)
class ViewSpec:
    """The per-view scalars (baked into a captured graph: one graph per distinct spec)."""
    height: int
    width: int
    fx: float
    fy: float
    cx: float
    cy: float
    sh_degree_to_use: int
    render_depth: bool = False
    clip_thresh: float = 0.01
    glob_scale: float = 1.0
    # "classic", or "antialiased": the view composites sigmoid(logits) * compensation (vanilla_gs.py:96-104,815-816),
    # formed and differentiated inside the projection kernels (gsr_project_forward_aa / _backward_aa)
    rasterize_mode: str = "classic"
    # absgrad (AbsGS; include/gsraster.h, gsr_rasterize_backward_abs): the compositing backward also sums |dL/dxy| per
    # pixel into `DensifyStats.absgrad`, and `xys_grad_norm` accumulates THAT norm instead of the signed gradient's.
    # Needs a `DensifyStats` (render_gaussians(stats=...)).
    absgrad: bool = False

    def __post_init__(self):
        if self.rasterize_mode not in ("classic", "antialiased"):
            raise ValueError("Unknown rasterize_mode: %s" % self.rasterize_mode)

    @property
    def antialiased(self) -> bool:
        return self.rasterize_mode == "antialiased"

    @property
    def tile_bounds(self):
        return ((self.width + BLOCK - 1) // BLOCK, (self.height + BLOCK - 1) // BLOCK, 1)


class DensifyStats:
    """``xys_grad_norm`` / ``vis_counts`` / ``max_2dsize`` of after_train (vanilla_gs.py:344-372),
    updated by the backward of `render_gaussians` itself (one launch, no retain_grad)."""

    def __init__(self, n: int, device, max_dim: int):
        self.xys_grad_norm = torch.zeros(n, device=device)
        self.vis_counts = torch.zeros(n, device=device, dtype=_i32)
        self.max_2dsize = torch.zeros(n, device=device)
        # `ViewSpec.absgrad`: overwritten by every backward of such a view (never accumulated; allocated here, outside
        # any capture, so that a graph's backward node has a fixed address to write)
        self.absgrad = torch.zeros((n, 2), device=device)
        self.max_dim = int(max_dim)
        # 1 = the next update is the first after a refinement (vanilla_gs.py:354-356); kept on the
        # DEVICE so that a captured graph replays correctly across refinement boundaries
        self.first = torch.ones(1, device=device, dtype=_i32)
        self.enabled = True

    def as_tuple(self):
        return self.xys_grad_norm, self.vis_counts, self.max_2dsize

    def restart(self):
        self.first.fill_(1)


class _Render(Function):
    @staticmethod
    def forward(ctx, means, log_scales, raw_quats, logits, features_dc, features_rest, viewmat, projmat, campos,
                background, spec: ViewSpec, capacity: int, count_out: Tensor, stats: Optional[DensifyStats],
                sh_collector=None, crop: Optional[Tensor] = None):
        n = means.shape[0]
        dev = means.device
        H, W = spec.height, spec.width
        tb = spec.tile_bounds
        degree = {1: 0, 4: 1, 9: 2, 16: 3}[features_rest.shape[1] + 1]
        with torch.cuda.device(dev):
            e = lambda shape, dt=_f32: torch.empty(shape, dtype=dt, device=dev)
            scales, quats, opac, dirs = e((n, 3)), e((n, 4)), torch.empty_like(logits), e((n, 3))
            cov3d, xys, depths, radii = e((n, 6)), e((n, 2)), e((n,)), e((n,), _i32)
            conics, comp, tiles, colors = e((n, 3)), e((n,)), e((n,), _i32), e((n, 3))
            opac_aa = torch.empty_like(opac) if spec.antialiased else None
            sort_b, bin_b, rec_b, lean = _workspace_bytes(n, capacity, tb)
            recs = e((n, rec_b), torch.uint8)
            counts = None if lean else e((n,), _i32)
            cum = None if lean else e((n,), _i32)
            order, ids, bins = e((n,), _i32), e((capacity,), _i32), _C.alloc_tile_bins(tb, dev)
            sort_ws, bin_ws = e((max(sort_b, 1),), torch.uint8), e((max(bin_b, 1),), torch.uint8)
            img, Ts, idx, alpha = e((H, W, 3)), e((H, W)), e((H, W), _i32), e((H, W))
            dep = e((H, W)) if spec.render_depth else None
            # alpha = 1 - T and the backward's cleared accumulators come out of the compositing launch
            wants_grad = any(ctx.needs_input_grad[:6])
            # rasterizer.rasterize.set_deterministic(True): the compositing backward sums in a fixed order
            # (gsr_rasterize_backward_det) instead of with float atomics -- see below
            det = wants_grad and _deterministic()
            acc = _C.backward_accumulators(n, 4 if spec.render_depth else 3, dev) if wants_grad and not det else None
            p = lambda t: None if t is None else t.data_ptr()
            seg = _segments(spec, capacity, dev)
            desc = _ViewDesc(n, degree, spec.sh_degree_to_use, int(spec.render_depth), H, W, spec.fx, spec.fy, spec.cx,
                             spec.cy, spec.glob_scale, spec.clip_thresh, capacity,
                             _C.deep_arg(bins, capacity, tb[0] * tb[1], tile_bounds=tb),
                             p(means), p(log_scales), p(raw_quats), p(logits), p(features_dc), p(features_rest),
                             p(viewmat), p(projmat), p(campos), p(background), p(scales), p(quats), p(opac), p(dirs),
                             p(cov3d), p(xys), p(depths), p(radii), p(conics), p(comp), p(tiles), p(colors), p(recs),
                             p(counts), p(order), p(cum), p(ids), p(bins), p(count_out), p(sort_ws), sort_b,
                             p(bin_ws), bin_b, p(img), p(dep), p(Ts), p(idx), p(alpha), p(acc),
                             0 if acc is None else acc.numel() * 4, *_seg_fields(seg), int(spec.antialiased),
                             p(opac_aa))
            if crop is None:
                _call("gsr_view_forward", C.byref(desc), _stream(dev))
            else:  # the crop box rides next to the descriptor (whose layout is unchanged)
                _call("gsr_view_forward_crop", C.byref(desc), crop, _stream(dev))
            del seg
            ctx.det = None
            if det:
                # what gsr_rasterize_backward_det reduces along: the depth order, the scan of the per-band counts and
                # the inverse of the scatter, from the list builder that returns it (the banded single-pass scatter;
                # no read-back: capturable).  Its lists are the view's lists -- every builder emits a tile's entries
                # in depth order (tests/test_gpu_kernels.py::test_list_builders_agree_on_random_shapes) -- and the
                # backward walks them with the forward's final_Ts / final_idx.
                op = (opac_aa if opac_aa is not None else opac).view(n, 1)
                counts_b, recs_b = _C.count_reach(xys, radii, conics, op, tb, bands=_C.tile_bands(tb))
                d_order, d_cum = _C.depth_order(depths, radii, counts_b)
                d_ids, d_bins, d_slots = _C.bin_sorted(n, capacity, d_order, d_cum, xys, radii, tb, BLOCK, recs_b,
                                                       device_sized=True, want_slots=True)
                ctx.det = (d_order, d_cum, d_ids, d_bins, d_slots)
        ctx.spec, ctx.stats, ctx.degree = spec, stats, degree
        ctx.sh_collector = sh_collector
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(means, raw_quats, features_dc, features_rest, viewmat, projmat, background, scales, quats,
                              opac, dirs, cov3d, xys, depths, radii, conics, comp, colors, ids, bins, Ts, idx,
                              *(() if opac_aa is None else (opac_aa,)))
        ctx.mark_non_differentiable(radii)
        ctx.accumulators = acc
        ctx.capacity = capacity
        if dep is None:
            return img, alpha, radii
        return img, alpha, radii, dep

    @staticmethod
    def backward(ctx, v_img, v_alpha, _v_radii, v_dep=None):
        (means, raw_quats, features_dc, features_rest, viewmat, projmat, background, scales, quats, opac, dirs, cov3d,
         xys, depths, radii, conics, comp, colors, ids, bins, Ts, idx) = ctx.saved_tensors[:22]
        spec, stats = ctx.spec, ctx.stats
        opac_aa = ctx.saved_tensors[22] if spec.antialiased else None
        n = means.shape[0]
        dev = means.device
        H, W = spec.height, spec.width
        tb = spec.tile_bounds
        with torch.cuda.device(dev):
            if v_img is None:
                v_img = torch.zeros(H, W, 3, device=dev)
            v_img = v_img.contiguous()
            v_a = None if v_alpha is None else v_alpha.contiguous()
            if spec.render_depth:
                v_dep = torch.zeros(H, W, device=dev) if v_dep is None else v_dep.contiguous()
            acc, ctx.accumulators = ctx.accumulators, None
            zeroed = acc is not None
            v_xy_abs = None
            if spec.absgrad:
                v_xy_abs = stats.absgrad
                if tuple(v_xy_abs.shape) != (n, 2) or v_xy_abs.device != dev:
                    raise ValueError("absgrad: DensifyStats.absgrad must be [N,2] on the parameters' device")
            if ctx.det is not None:
                # fixed summation order: the compositing backward from Python, its sums laid out as the accumulators,
                # and gsr_view_backward for everything behind it
                d_order, d_cum, d_ids, d_bins, d_slots = ctx.det
                op = (opac_aa if opac_aa is not None else opac).view(n, 1)
                sums = _C.rasterize_backward_det(
                    H, W, d_ids, d_bins, xys, conics, colors, op, background, Ts, idx, v_img, v_a, d_order, d_cum,
                    d_slots, extra=depths if spec.render_depth else None,
                    v_output_extra=v_dep if spec.render_depth else None, v_xy_abs=v_xy_abs)
                if spec.render_depth:  # (v_xy, v_conic, v_colors, v_extra, v_opacity) -> ... v_opacity | v_extra
                    sums = sums[:3] + (sums[4], sums[3])
                acc = torch.cat([t.reshape(-1) for t in sums])
            elif acc is None:  # a second backward (retain_graph): the kernels clear their own
                acc = _C.backward_accumulators(n, 4 if spec.render_depth else 3, dev)
            e = lambda shape: torch.empty(shape, dtype=_f32, device=dev)
            t_cov2d, t_cov3d, t_vs, t_vq = e((n, 3)), e((n, 6)), e((n, 3)), e((n, 4))
            v_means, g_s, g_q, g_o = e((n, 3)), e((n, 3)), e((n, 4)), torch.empty_like(opac)
            collector = ctx.sh_collector
            if collector is None:
                v_dc, v_rest = torch.empty_like(features_dc), torch.empty_like(features_rest)
            else:  # data parallel: the SH gradient is formed from the ranks' gathered colour cotangents
                v_dc = v_rest = None
            use_stats = stats is not None and stats.enabled
            p = lambda t: None if t is None else t.data_ptr()
            seg = _segments_backward(spec, ctx.capacity, dev)
            desc = _ViewDesc(n, ctx.degree, spec.sh_degree_to_use, int(spec.render_depth), H, W, spec.fx, spec.fy,
                             spec.cx, spec.cy, spec.glob_scale, spec.clip_thresh, ctx.capacity,
                             _C.deep_arg(bins, ctx.capacity, tb[0] * tb[1], backward=True, tile_bounds=tb),
                             p(means), None, p(raw_quats), None, p(features_dc), p(features_rest), p(viewmat),
                             p(projmat), None, p(background), p(scales), p(quats), p(opac), p(dirs), p(cov3d), p(xys),
                             p(depths), p(radii), p(conics), p(comp), None, p(colors), None, None, None, None, p(ids),
                             p(bins), None, None, 0, None, 0, None, None, p(Ts), p(idx), None, None, 0,
                             *_seg_fields(seg), int(spec.antialiased), p(opac_aa))
            grads = _ViewGrads(p(v_img), p(v_a), p(v_dep) if spec.render_depth else None, p(acc), int(zeroed),
                               p(stats.first) if use_stats else None, (1.0 / stats.max_dim) if use_stats else 0.0,
                               p(stats.xys_grad_norm) if use_stats else None, p(stats.vis_counts) if use_stats else None,
                               p(stats.max_2dsize) if use_stats else None, p(t_cov2d), p(t_cov3d), p(t_vs), p(t_vq),
                               p(v_means), p(g_s), p(g_q), p(g_o), p(v_dc), p(v_rest), int(ctx.det is not None),
                               p(v_xy_abs))
            _call("gsr_view_backward", C.byref(desc), C.byref(grads), _stream(dev))
            del seg
            if use_stats:
                stats.first.zero_()
            if collector is not None:
                # the colour cotangents the compositing backward left in the accumulators, cut where the forward's
                # clamp cut the colour (marked -0.0), as gsr_sh_backward_split would have cut them
                v_col = acc[5 * n:8 * n].view(n, 3)
                cut = colors.view(torch.int32) == -2147483648
                collector.offer(torch.where(cut, torch.zeros((), dtype=_f32, device=dev), v_col).contiguous())
        return (v_means, g_s, g_q, g_o, v_dc, v_rest) + (None,) * 10


def render_gaussians(means: Tensor, log_scales: Tensor, raw_quats: Tensor, opacity_logits: Tensor,
                     features_dc: Tensor, features_rest: Tensor, viewmat: Tensor, projmat: Tensor, campos: Tensor,
                     background: Tensor, spec: ViewSpec, capacity: int, count_out: Optional[Tensor] = None,
                     stats: Optional[DensifyStats] = None, sh_collector=None,
                     crop: Optional[Tensor] = None) -> Dict[str, Optional[Tensor]]:
    """The raw parameters of a Gaussian model -> ``{"rgb" [H,W,3] (not clamped at 1), "alpha"
    [H,W], "depth" [H,W] or None (accumulated, not divided by alpha), "radii" [N] i32,
    "count" int32[1]}``.

    viewmat: the top 3x4 (or 4x4) world->camera matrix, projmat 4x4 ``P @ V``, campos [3],
    all on the device.  ``capacity``: entries the tile lists are sized for; ``count`` receives
    the entries the view really needs -- if it exceeds the capacity the lists were cut and
    the result is incomplete: render again with a larger capacity (`ListCapacity`).
    ``spec.absgrad``: the backward overwrites ``stats.absgrad`` [N,2] with the per-pixel |dL/dxy| sums and
    ``stats.xys_grad_norm`` accumulates its norm (``stats`` is then required: ValueError without).
    ``count_out`` may be a caller-owned int32[1] (device, or pinned host memory).    ``sh_collector`` (data parallel, `harness.parallel.GradientExchange.begin_sh_views`): the backward skips its SH
    backward, hands the colour cotangents [N,3] to ``sh_collector.offer`` and returns no gradient for
    ``features_dc`` / ``features_rest`` -- the exchange forms it from all ranks' cotangents.
    ``crop``: float32[16] on the device (`gs_fused.CropBox.tensor`), the oriented crop box of the toolkit's
    ``get_outputs`` (vanilla_gs.py:703-757) without its gathers: a Gaussian whose centre is outside the box is culled
    inside the projection kernel (``radii == 0``; its gradients are zero in all six groups), N stays what it is.  An
    empty box gives the background with alpha 0 (the reference's depth-10 image needs a read-back: `render_view`).
    """
    n = means.shape[0]
    if features_dc.shape != (n, 3) or features_rest.dim() != 3 or features_rest.shape[1] + 1 not in (1, 4, 9, 16):
        raise ValueError("features_dc [N,3] and features_rest [N,K-1,3] with K in (1, 4, 9, 16) expected")
    if log_scales.shape != (n, 3) or raw_quats.shape != (n, 4) or opacity_logits.numel() != n:
        raise ValueError("expected scales [N,3], quats [N,4], opacities [N,1]")
    if capacity < 1:
        raise ValueError("capacity must be positive")
    if spec.absgrad and stats is None:
        raise ValueError("ViewSpec.absgrad needs stats=DensifyStats(...): the absgrad lands in its `absgrad` buffer")
    if count_out is None:
        count_out = torch.empty(1, dtype=_i32, device=means.device)
    if crop is not None:
        _C._check_crop(crop, means.device)
    vm = viewmat[:3, :] if viewmat.shape[0] == 4 else viewmat
    out = _Render.apply(means.contiguous(), log_scales.contiguous(), raw_quats.contiguous(),
                        opacity_logits.contiguous(), features_dc.contiguous(), features_rest.contiguous(),
                        vm.contiguous(), projmat.contiguous(), campos.contiguous(), background.contiguous(), spec,
                        int(capacity), count_out, stats, sh_collector, crop)
    return {"rgb": out[0], "alpha": out[1], "radii": out[2], "depth": out[3] if spec.render_depth else None,
            "count": count_out}


@dataclass
class ListCapacity:
    """Keeps the tile lists large enough without waiting for the GPU: ``capacity`` for the
    next view, and a check of a PREVIOUS view's real count (read from pinned memory
    once its event has fired).  ``grow`` is the head-room over the largest count seen."""
    capacity: int = 1 << 20
    grow: float = 1.5
    _pending: list = field(default_factory=list)

    def slot(self, device) -> Tensor:
        """A pinned int32[1] for `render_gaussians(count_out=...)`; call `submitted()` after
        the render has been enqueued."""
        return torch.zeros(1, dtype=_i32).pin_memory()

    def submitted(self, slot: Tensor, capacity_used: int, device) -> None:
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        self._pending.append((ev, slot, capacity_used))

    def overflowed(self, wait: bool = False) -> bool:
        """Did any finished view need more entries than it was given?  Grows `capacity`."""
        bad = False
        keep = []
        for ev, slot, cap in self._pending:
            if wait:
                ev.synchronize()
            if not ev.query():
                keep.append((ev, slot, cap))
                continue
            need = int(slot[0])
            if need > cap:
                bad = True
            want = int(self.grow * need) + 65536
            if want > self.capacity:
                self.capacity = (want + (1 << 20) - 1) & ~((1 << 20) - 1)
        self._pending = keep
        return bad


class ViewGraph:
    """One HIP graph per view: render -> loss -> backward of a Gaussian model captured once
    (``torch.cuda.CUDAGraph`` = hipGraph on ROCm) and replayed for every view with the same
    `ViewSpec`, number of Gaussians and list capacity.  What varies per view -- the camera
    matrices and position, the target image(s), the crop box of a graph built with one (`set_crop`) -- is copied into
    static buffers before the replay (a target may be a `gs_fused.DeferredTarget`, which writes its buffer itself); the parameter gradients land in static ``.grad`` tensors that the optimizer
    then reads as usual.  The graph holds ~45 kernel nodes that are otherwise ~45 launches
    from Python through ctypes / autograd.

    ``loss_fn(out, targets) -> scalar`` with ``out`` the dict of `render_gaussians` and
    ``targets`` the tuple of static target tensors.  After a replay, ``count_host[0]`` (pinned)
    holds the list entries the view needed: `fits()` tells whether they fitted the capacity
    the graph was captured with -- if not, the result of that view is incomplete and the
    owner re-captures with a larger capacity (`ListCapacity`)."""

    def __init__(self, params: Dict[str, Tensor], spec: ViewSpec, capacity: int, loss_fn, background: Tensor,
                 target_shapes, stats: Optional[DensifyStats] = None, crop: Optional[Tensor] = None):
        if spec.absgrad and stats is None:
            raise ValueError("ViewSpec.absgrad needs stats=DensifyStats(...): the absgrad lands in its `absgrad` buffer")
        self.params, self.spec, self.capacity, self.loss_fn, self.stats = params, spec, int(capacity), loss_fn, stats
        dev = params["means"].device
        self.device = dev
        self.background = background
        self.viewmat = torch.zeros(3, 4, device=dev)
        self.projmat = torch.zeros(4, 4, device=dev)
        self.campos = torch.zeros(3, device=dev)
        self.targets = tuple(torch.zeros(s, device=dev) for s in target_shapes)
        # the crop box the captured view reads (None: the graph has no such node); `set_crop` moves it between replays
        self.crop = None if crop is None else self._crop_values(crop).to(dev).clone()
        self.count_dev = torch.zeros(1, dtype=_i32, device=dev)
        self.count_host = torch.zeros(1, dtype=_i32).pin_memory()
        self.graph = None
        self.out = None
        self.loss = None

    def _set_inputs(self, viewmat, projmat, campos, targets):
        self.viewmat.copy_(viewmat[:3, :])
        self.projmat.copy_(projmat)
        self.campos.copy_(campos)
        for dst, src in zip(self.targets, targets):
            if hasattr(src, "write"):  # a gs_fused.DeferredTarget: its kernel writes the static tensor itself
                src.write(dst)
            else:
                dst.copy_(src)

    @staticmethod
    def _crop_values(box) -> Tensor:
        t = box if isinstance(box, Tensor) else box.tensor("cpu")
        if t.dtype != _f32 or t.numel() != 16:
            raise ValueError("a crop box is a gs_fused.CropBox or its float32[16] tensor")
        return t.reshape(16)

    def set_crop(self, box) -> None:
        """Move the crop box (a `gs_fused.CropBox` or its float32[16]): copied into the static buffer the captured
        view reads, ahead of the next replay -- as `_set_inputs` copies the camera; nothing is captured again.  A
        graph built without a crop has no node that reads one: ValueError."""
        if self.crop is None:
            raise ValueError("this ViewGraph was built without a crop box: build one with crop= to move it later")
        self.crop.copy_(self._crop_values(box))

    def _step(self):
        p = self.params
        out = render_gaussians(p["means"], p["scales"], p["quats"], p["opacities"], p["features_dc"],
                               p["features_rest"], self.viewmat, self.projmat, self.campos, self.background, self.spec,
                               self.capacity, count_out=self.count_dev, stats=self.stats, crop=self.crop)
        loss = self.loss_fn(out, self.targets)
        loss.backward()
        _C.publish_int32(self.count_dev, self.count_host)
        return out, loss

    def capture(self, viewmat, projmat, campos, targets) -> None:
        """Warm up eagerly on a side stream (allocator, lazy initialisation), then capture."""
        self._set_inputs(viewmat, projmat, campos, targets)
        first_flag = None if self.stats is None else self.stats.first.clone()
        saved = None if self.stats is None else [t.clone() for t in self.stats.as_tuple()]
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(2):
                for t in self.params.values():
                    t.grad = None
                self._step()
        torch.cuda.current_stream(self.device).wait_stream(side)
        for t in self.params.values():
            t.grad = None
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out, self.loss = self._step()
        if self.stats is not None:  # the warm-up and the capture must not count as views
            self.stats.first.copy_(first_flag)
            for dst, src in zip(self.stats.as_tuple(), saved):
                dst.copy_(src)

    def replay(self, viewmat, projmat, campos, targets):
        """-> (loss, out): static tensors, overwritten by the next replay."""
        self._set_inputs(viewmat, projmat, campos, targets)
        self.graph.replay()
        return self.loss, self.out

    def fits(self) -> bool:
        """After a synchronisation point: did the last replayed view fit the capacity?"""
        return int(self.count_host[0]) <= self.capacity
