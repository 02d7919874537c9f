"""Child process of tests/test_gpu_lists_tail.py: the job orders the list build's last launch writes against those of
`gsr_tile_jobs_build`, and the compositing calls over them.

A process of its own because the library reads its two switches once: GSR_TILE_SORT=t (the two-level partition at any
list size) and GSR_DEEP_SPLIT_KEY (the key ratio of a split tile's jobs, pinned: the measured one moves from launch to
launch).  Prints one JSON object: {case: {check: value}}; the test asserts on it."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gaussian-splatting-toolkit_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"
BW = 16
ORDERED, SECOND = 1 << 30, 1 << 28
SENTINEL = 0x5A5A5A5A


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def splats(n, W, H, r_lo, r_hi, seed, cluster=0, x_hi=1.0):
    """n splats in screen space (the generator of tests/test_gpu_list_builders_residency.py) over the left `x_hi` of
    the image, and `cluster` more inside a 96 x 96 px square: a few tiles with lists many times the mean."""
    rng = np.random.default_rng(seed)
    m = n + cluster
    radii = rng.integers(r_lo, r_hi + 1, m).astype(np.int32)
    xys = np.stack([rng.uniform(0, W * x_hi, m), rng.uniform(0, H, m)], 1).astype(np.float32)
    if cluster:
        xys[n:] = np.stack([rng.uniform(W * 0.3, W * 0.3 + 96, cluster), rng.uniform(H * 0.4, H * 0.4 + 96, cluster)], 1)
    smax = radii / 3.0
    smin = smax * rng.uniform(0.3, 1.0, m)
    th = rng.uniform(0, np.pi, m)
    c, s = np.cos(th), np.sin(th)
    cxx = c * c * smax**2 + s * s * smin**2
    cyy = s * s * smax**2 + c * c * smin**2
    cxy = c * s * (smax**2 - smin**2)
    det = cxx * cyy - cxy * cxy
    conics = np.stack([cyy / det, -cxy / det, cxx / det], 1).astype(np.float32)
    opac = rng.uniform(0.1, 1.0, (m, 1)).astype(np.float32)
    depths = rng.uniform(0.5, 50.0, m).astype(np.float32)
    return dict(xys=cu(xys), radii=cu(radii), conics=cu(conics), opac=cu(opac), depths=cu(depths)), m


def tail_of(Cm, bins, tb):
    nt = tb[0] * tb[1]
    ints = Cm.tile_jobs_ints(tb)
    return torch.empty(0, dtype=torch.int32, device=DEV).set_(bins.untyped_storage(), bins.storage_offset() + 2 * nt, (ints,))


def stats_pointer(tail):
    return int.from_bytes(tail[-2:].cpu().numpy().tobytes(), "little")


def copy_raw(Cm, src, dst, nbytes):
    Cm._call("gsr_calibrate_copy", C.c_void_p(src), C.c_void_p(dst), C.c_size_t(nbytes), Cm._stream(torch.device(DEV)))
    torch.cuda.synchronize()


def build_lists(Cm, g, n, tb, orders):
    cnt, _ = Cm.count_reach(g["xys"], g["radii"], g["conics"], g["opac"], tb)
    I = int(cnt.sum().item())
    recs, order = Cm.reach_records_depth_order(g["xys"], g["radii"], g["conics"], g["opac"], g["depths"], tb)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    ids, bins = Cm.bin_sorted(n, I + 1000, order, None, g["xys"], g["radii"], tb, BW, recs, device_sized=True,
                              count_out=count, job_orders=orders)
    assert int(count.item()) == I
    return ids, bins, I


def reference_tail(Cm, bins, tb, fwd, bwd):
    """The same tile_bins in a fresh buffer, its orders by gsr_tile_jobs_build."""
    copy = Cm.alloc_tile_bins(tb, torch.device(DEV))
    copy.copy_(bins)
    Cm._call("gsr_tile_jobs_build", C.c_int(tb[0]), C.c_int(tb[1]), Cm._ptr(copy), C.c_int(fwd), C.c_int(bwd),
             Cm._stream(torch.device(DEV)))
    torch.cuda.synchronize()
    return tail_of(Cm, copy, tb), copy


def decode(tail, base, which):
    jobs = tail[which * 4 * base:(which + 1) * 4 * base].cpu().numpy()
    live = jobs[jobs >= 0]
    return live & ((1 << 27) - 1), live >> 27


def order_case(Cm, out, name, W, H, n, r, seed, fwd, bwd, cluster=0, x_hi=1.0, stats=False):
    tb = ((W + BW - 1) // BW, (H + BW - 1) // BW, 1)
    nt = tb[0] * tb[1]
    g, m = splats(n, W, H, r[0], r[1], seed, cluster, x_hi)
    res = out[name] = {}
    stats_buf = torch.full((256,), 16.0, dtype=torch.float32, device=DEV)
    if stats:  # every sum of the library's statistics := 16
        copy_raw(Cm, stats_buf.data_ptr(), stats["ptr"], 1024)
    ids, bins, I = build_lists(Cm, g, m, tb, (fwd, bwd))
    torch.cuda.synchronize()
    if bwd:
        fused = getattr(bins, "_gsr_jobs_fwd", 0) == fwd and getattr(bins, "_gsr_jobs_bwd", 0) == bwd
    else:  # (one order: the package marks pairs only)
        fused = bool((tail_of(Cm, bins, tb)[0] != SENTINEL).item())
    res["fused"] = bool(fused)
    base = (Cm.tile_jobs_ints(tb) - 2) // 8
    res["empty_slots"] = int(base - nt)
    tail = tail_of(Cm, bins, tb)
    if not fused:
        res["tail_untouched"] = bool((tail == SENTINEL).all().item())
        # ... and the forward's own route then builds them with the separate launch, as before
        Cm.forward_orders(bins, ids.numel(), nt, tb, torch.device(DEV))
        torch.cuda.synchronize()
        res["separate_launch_wrote"] = bool((tail_of(Cm, bins, tb) != SENTINEL).any().item())
        return
    if stats:
        got = torch.empty_like(stats_buf)
        copy_raw(Cm, stats["ptr"], got.data_ptr(), 1024)
        sums = got.view(2, 8, 16)[:, :, :4]
        res["stats_after_fused_build"] = sorted(set(sums.flatten().tolist()))
    ref, _ = reference_tail(Cm, bins, tb, fwd, bwd)
    if stats:
        copy_raw(Cm, stats["ptr"], got.data_ptr(), 1024)
        res["stats_after_reference_build"] = sorted(set(got.view(2, 8, 16)[:, :, :4].flatten().tolist()))
        res["stats_padding"] = sorted(set(got.view(2, 8, 16)[:, :, 4:].flatten().tolist()))
    res["equal"] = bool(torch.equal(tail, ref))
    res["differing_ints"] = int((tail != ref).sum().item())
    res["no_sentinel_left"] = bool((tail != SENTINEL).all().item())
    res["stats_pointer"] = stats_pointer(tail)
    lens = (bins[:, 1] - bins[:, 0]).cpu().numpy()
    for which, key in ((0, "fwd"), (1, "bwd")) if bwd else ((0, "fwd"),):
        tile, allowed = decode(tail, base, which)
        seen = np.zeros(nt, np.int64)
        np.add.at(seen, tile, allowed)
        res[key + "_every_tile_once"] = bool(np.all(seen == 15))
        res[key + "_split_jobs"] = int((allowed != 15).sum())
        res[key + "_split_jobs_of_empty_tiles"] = int(((allowed != 15) & (lens[tile] == 0)).sum())
        thr = (bwd if which else fwd) & 0x3FFFFF  # (sub-tile jobs of tiles at or below it: the tail's)
        res[key + "_split_jobs_at_or_below_threshold"] = int(((allowed != 15) & (lens[tile] <= thr)).sum())
    res["empty_tiles"] = int((lens == 0).sum())
    res["longest_over_mean"] = float(lens.max() / max(lens[lens > 0].mean(), 1.0))
    return tail


def end_to_end(Cm, out):
    """The compositing forward and backward over lists that came with their orders against the same lists with the
    orders built by gsr_tile_jobs_build, at a job-ordered grid (43 x 29 = 1 247 tiles) -- the words the package itself
    computes."""
    W, H = 688, 464
    tb = ((W + BW - 1) // BW, (H + BW - 1) // BW, 1)
    nt = tb[0] * tb[1]
    g, m = splats(30000, W, H, 4, 14, seed=31, cluster=3000)
    rng = np.random.default_rng(5)
    colors = cu(rng.uniform(0, 1, (m, 3)).astype(np.float32))
    bg = cu(np.array([0.1, 0.2, 0.3], np.float32))
    v_img = cu(rng.uniform(-1, 1, (H, W, 3)).astype(np.float32))
    v_alpha = cu(rng.uniform(-1, 1, (H, W)).astype(np.float32))
    calls = []
    real_call = Cm._call

    def spy(name, *a):
        calls.append(name)
        return real_call(name, *a)

    Cm._call = spy
    res = out["end_to_end"] = {}
    runs = {}
    for mode, orders in (("prebuilt", None), ("separate", (0, 0))):
        del calls[:]
        ids, bins, I = build_lists(Cm, g, m, tb, orders)
        a = (tb, (BW, BW, 1), (W, H, 1), ids, bins, g["xys"], g["conics"], colors, g["opac"], bg)
        f = Cm.rasterize_forward_ex(*a, want_alpha=True)
        b = Cm.rasterize_backward(H, W, BW, *a[3:], f[1], f[2], v_img, v_alpha)
        torch.cuda.synchronize()
        runs[mode] = (ids, bins, f, b, tail_of(Cm, bins, tb).clone())
        res[mode + "_jobs_build_calls"] = calls.count("gsr_tile_jobs_build")
        res[mode + "_list_build_with_orders"] = calls.count("gsr_bin_sorted_dev_jobs")
    Cm._call = real_call
    p, s = runs["prebuilt"], runs["separate"]
    res["ordered"] = bool(Cm.deep_arg(p[1], p[0].numel(), nt, tile_bounds=tb) & ORDERED)
    res["lists_equal"] = bool(torch.equal(p[0][:I], s[0][:I]) and torch.equal(p[1], s[1]))
    res["orders_equal"] = bool(torch.equal(p[4], s[4]))
    res["images_equal"] = bool(all(torch.equal(x, y) for x, y in zip(p[2], s[2])))
    res["grad_rel_diff"] = [float((x - y).abs().max().item() / x.abs().max().item()) for x, y in zip(p[3], s[3])]
    import rasterizer.rasterize as R

    res["fallbacks"] = int(R.counters["orders_prebuilt_fallbacks"])


def main():
    import rasterizer.cuda as Cm

    real_alloc = Cm.alloc_tile_bins

    def alloc(tile_bounds, dev):  # (so that what a launch did not write shows)
        bins = real_alloc(tile_bounds, dev)
        tail_of(Cm, bins, tile_bounds).fill_(SENTINEL)
        return bins

    Cm.alloc_tile_bins = alloc
    out = {"env": {k: os.environ.get(k) for k in ("GSR_TILE_SORT", "GSR_DEEP_SPLIT_KEY")}}
    word = lambda thr, tail, second: thr | ORDERED | (tail << 22) | (SECOND if second else 0)
    # lists all alike on 43 x 29 tiles (a padded XCD map): the backward splits nothing, both orders the static one
    tail = order_case(Cm, out, "alike", 688, 464, 60000, (6, 10), 21, word(100, 0, False), word(100, 0, True))
    st = {"ptr": stats_pointer(tail)} if tail is not None else False
    # a long-tailed scene on 75 x 43 tiles (448 slots per XCD: two rounds of 256 threads): tiles above the threshold
    # split into four jobs; the statistics' sums halve once per build
    order_case(Cm, out, "longtail", 1200, 688, 30000, (4, 12), 22, word(100, 0, False), word(150, 0, True), cluster=6000,
               stats=st)
    order_case(Cm, out, "tail64", 1200, 688, 30000, (4, 12), 23, word(100, 8, False), word(150, 5, True), cluster=6000)
    # a tenth of the image empty, a quarter of the whole-tile jobs in the tail: empty tiles among them
    order_case(Cm, out, "empty_in_tail", 1200, 688, 30000, (4, 12), 24, word(100, 16, False), word(150, 16, True),
               cluster=3000, x_hi=0.9)
    # 257 x 64 tiles: colscatter_kernel<1024>, tile_bins by gsr_tile_bases
    order_case(Cm, out, "wide", 4112, 1024, 20000, (5, 40), 25, word(200, 4, False), word(400, 0, True), cluster=4000)
    # 256 x 113 tiles: 57 chunks per XCD, more than colscatter_kernel<256>'s LDS holds -- the separate launch stays
    order_case(Cm, out, "no_fit", 4096, 1808, 5000, (5, 40), 26, word(200, 4, False), word(400, 0, True))
    # one order only (8 workgroups in front)
    order_case(Cm, out, "forward_only", 1200, 688, 30000, (4, 12), 27, word(100, 8, False), 0, cluster=6000)
    Cm.alloc_tile_bins = real_alloc
    end_to_end(Cm, out)
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
