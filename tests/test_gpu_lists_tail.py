"""GPU: the two pieces of work taken out of the list build's tail.

1. `emit` (csrc/tile_partition2.hip) keeps a batch's items in SORTED order, three words per item, and an entry reads
   them by its item's sorted index.  The two-level partition against the banded single-pass lists, ids and bins bit for
   bit (the comparison of tests/test_gpu_list_builders_residency.py), on splats given directly in screen space so that
   the number of (Gaussian, row) items of a slab and the number of entries of a batch are what the case says: the
   expectation is derived on the CPU from the box rule alone (gsr_tile_bbox) and asserted before the comparison.
   129 x 129 tiles take the two-level path at any list size.

2. The job orders of the compositing launches, written by the first workgroups of the list build's last launch
   (`colscatter_kernel`) instead of a launch of their own: to the last int what `gsr_tile_jobs_build` -- the
   implementation both share, whose result this change must not move -- writes behind a copy of the same tile_bins.
   Those cases run in ONE child process (tests/list_tail_orders_child.py): the library reads GSR_TILE_SORT and
   GSR_DEEP_SPLIT_KEY once, and the split ratio must be pinned because the measured one moves with every launch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BW = 16
W = H = 2064  # 129 x 129 tiles


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def splats(n, W, H, r_lo, r_hi, seed, cull_every=0):
    """n splats in screen space: radius = ceil(3 sigma_max) like the projection's, anisotropic conics
    (the generator of tests/test_gpu_list_builders_residency.py)."""
    rng = np.random.default_rng(seed)
    radii = rng.integers(r_lo, r_hi + 1, n).astype(np.int32)
    xys = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1).astype(np.float32)
    smax = radii / 3.0
    smin = smax * rng.uniform(0.3, 1.0, n)
    th = rng.uniform(0, np.pi, n)
    c, s = np.cos(th), np.sin(th)
    cxx = c * c * smax**2 + s * s * smin**2
    cyy = s * s * smax**2 + c * c * smin**2
    cxy = c * s * (smax**2 - smin**2)
    det = cxx * cyy - cxy * cxy
    conics = np.stack([cyy / det, -cxy / det, cxx / det], 1).astype(np.float32)
    opac = rng.uniform(0.1, 1.0, (n, 1)).astype(np.float32)
    depths = rng.uniform(0.5, 50.0, n).astype(np.float32)
    if cull_every:
        radii[::cull_every] = 0
    return dict(xys=cu(xys), radii=cu(radii), conics=cu(conics), opac=cu(opac), depths=cu(depths))


def placed(xy, radii, sigma, opac):
    """Splats at given centres with isotropic conics of `sigma` px, in depth order by index."""
    n = len(radii)
    xy = np.asarray(xy, np.float32).reshape(n, 2)
    conics = np.stack([1.0 / np.square(sigma), np.zeros(n), 1.0 / np.square(sigma)], 1).astype(np.float32)
    depths = (1.0 + np.arange(n) * 0.01).astype(np.float32)
    return dict(xys=cu(xy), radii=cu(np.asarray(radii, np.int32)), conics=cu(conics),
                opac=cu(np.asarray(opac, np.float32).reshape(n, 1)), depths=cu(depths))


def box(xy, radii, tiles_x, tiles_y):
    """gsr_tile_bbox in float32 -> (box width, box height) in tiles per splat."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    t = xy / np.float32(BW)
    tr = np.asarray(radii, np.float32) / np.float32(BW)
    lo = lambda c, hi: np.clip((c - tr).astype(np.int32), 0, hi)
    up = lambda c, hi: np.clip((c + tr + np.float32(1)).astype(np.int32), 0, hi)
    return up(t[:, 0], tiles_x) - lo(t[:, 0], tiles_x), up(t[:, 1], tiles_y) - lo(t[:, 1], tiles_y)


def lists_agree(n, W, H, g):
    import rasterizer.cuda as C

    tb = ((W + BW - 1) // BW, (H + BW - 1) // BW, 1)
    nb = C.tile_bands(tb)
    assert nb > 1
    cnt1, recs1 = C.count_reach(g["xys"], g["radii"], g["conics"], g["opac"], tb)
    o1, c1 = C.depth_order(g["depths"], g["radii"], cnt1)
    I1 = int(c1[-1].item())
    assert I1 > 0
    ids_t, bins_t = C.bin_sorted(n, I1, o1, c1, g["xys"], g["radii"], tb, BW, recs1)
    cntb, recs = C.count_reach(g["xys"], g["radii"], g["conics"], g["opac"], tb, bands=nb)
    o2, c2 = C.depth_order(g["depths"], g["radii"], cntb)
    I2 = int(c2[-1].item())
    ids_b, bins_b = C.bin_sorted(n, I2, o2, c2, g["xys"], g["radii"], tb, BW, recs)
    assert I1 == I2 and torch.equal(bins_t, bins_b) and torch.equal(ids_t, ids_b)
    assert int(bins_t[:, 1].max()) == I1
    return I1, cnt1, ids_t, bins_t


def grid_centres(n, dx, dy):
    """n centres at tile centres (16 k + 8), well inside the image."""
    k = np.arange(n)
    return np.stack([16.0 * (20 + (k % 16) * 5) + dx, 16.0 * (20 + (k // 16) * 5) + dy], 1)


@pytest.mark.parametrize("items", [1024, 1025])
def test_a_batch_of_exactly_1024_items_and_one_of_1025(items):
    """One slab of 256 splats whose boxes are 4 rows high (centre at a tile centre, radius 24): 1024 (Gaussian, row)
    items, one batch to the last slot of the sorted table; with one box of 5 rows (radius 32) a second batch of one
    item.  Every box tile is kept (sigma far above the radius), so every item has entries: 4 each, 4096 in the batch
    -- a multiple of 64, the last start-mask word full to its last bit."""
    n = 256
    radii = np.full(n, 24, np.int32)
    if items == 1025:
        radii[100] = 32
    xy = grid_centres(n, 8.0, 8.0)
    bw_, bh_ = box(xy, radii, W // BW, H // BW)
    assert int(bh_.sum()) == items and (bw_[radii == 24] == 4).all()
    g = placed(xy, radii, np.full(n, 1000.0), np.ones(n))
    I, cnt, _, _ = lists_agree(n, W, H, g)
    assert I == int((bw_ * bh_).sum()) and (I % 64 == 0) == (items == 1024)
    assert np.array_equal(cnt.cpu().numpy(), bw_ * bh_)


def test_items_without_entries_between_items_that_have_some():
    """The same slab with sigma = 8 px and opacities from 0.02 to 1: the exact reach test empties the outer rows of the
    faint splats' boxes (alpha >= 1/255 within sqrt(2 ln(255 opacity)) sigma: 15 px at 0.02, 27 px at 1), so sorted
    items with entries alternate with (Gaussian, row) items that have none and are never placed."""
    n = 256
    radii = np.full(n, 24, np.int32)
    xy = grid_centres(n, 8.0, 8.0)
    opac = np.where(np.arange(n) % 3 == 0, 0.02, np.where(np.arange(n) % 3 == 1, 0.2, 1.0))
    g = placed(xy, radii, np.full(n, 8.0), opac)
    bw_, bh_ = box(xy, radii, W // BW, H // BW)
    I, cnt, _, _ = lists_agree(n, W, H, g)
    cnt = cnt.cpu().numpy()
    assert int(bh_.sum()) == 1024
    # a faint splat reaches no further than 15 px from its centre: its box's last row, 24 px away, is empty
    assert (cnt[0::3] <= 3 * 4).all() and (cnt[0::3] > 0).all() and cnt[2::3].min() > cnt[0::3].max()
    assert I < int((bw_ * bh_).sum())


def mask_size_scene():
    """256 splats, one slab of four batches of 64 splats x 16 rows = 1024 items; every box tile kept.  A box is 16 rows
    x 16 columns (radius 124, centre 12.8 px into its tile) = 256 entries; 17 columns (centre 8 px into its tile in x)
    = 272; 15 columns (clipped at the left image edge) = 240.  Batches of 16368, 16400, 16384 and 16400 entries: below,
    above, at and above the 16384 the start masks hold -- both branches, alternating inside one slab."""
    n = 256
    k = np.arange(n)
    xy = np.stack([16.0 * (10 + (k % 8) * 14) + 12.8, 16.0 * (10 + ((k // 8) % 8) * 14) + 12.8], 1)
    xy[5, 0] = 16.0 * 6 + 12.8     # columns [-1, 15) -> 15 inside the image
    xy[64 + 7, 0] = 16.0 * 40 + 8.0
    xy[192 + 9, 0] = 16.0 * 40 + 8.0
    radii = np.full(n, 124, np.int32)
    return n, xy, radii


def test_batches_just_below_at_and_just_above_the_start_mask_size():
    n, xy, radii = mask_size_scene()
    bw_, bh_ = box(xy, radii, W // BW, H // BW)
    assert (bh_ == 16).all()
    per_batch = (bw_ * bh_).reshape(4, 64).sum(1)
    assert per_batch.tolist() == [16368, 16400, 16384, 16400]
    g = placed(xy, radii, np.full(n, 5000.0), np.ones(n))
    I, cnt, _, _ = lists_agree(n, W, H, g)
    assert I == int(per_batch.sum()) and np.array_equal(cnt.cpu().numpy(), bw_ * bh_)


def test_a_capacity_that_cuts_a_batch_in_the_middle():
    """Device-sized lists of the scene above with room for 30 000 of its 65 552 entries.  The row-partitioned stream
    is cut at the capacity: the count that comes back is the uncut one, the tile rows that end below the cut have
    their full lists, the row the cut falls into has a depth-order prefix of every tile's list and the rows behind
    it have none."""
    import rasterizer.cuda as C

    n, xy, radii = mask_size_scene()
    g = placed(xy, radii, np.full(n, 5000.0), np.ones(n))
    I, _, ids_full, bins_full = lists_agree(n, W, H, g)
    tb = (W // BW, H // BW, 1)
    cap = 30000
    recs, order = C.reach_records_depth_order(g["xys"], g["radii"], g["conics"], g["opac"], g["depths"], tb)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    ids, bins = C.bin_sorted(n, cap, order, None, g["xys"], g["radii"], tb, BW, recs, device_sized=True, count_out=count)
    assert int(count.item()) == I and ids.numel() == cap
    ids, bins, ids_full, bins_full = ids.cpu().numpy(), bins.cpu().numpy(), ids_full.cpu().numpy(), bins_full.cpu().numpy()
    lens_full = (bins_full[:, 1] - bins_full[:, 0]).reshape(tb[1], tb[0])
    row_end = np.cumsum(lens_full.sum(1))
    cut_row = int(np.searchsorted(row_end, cap, side="right"))
    assert 0 < cut_row < tb[1] - 1 and row_end[cut_row] > cap > (row_end[cut_row - 1])
    whole = cut_row * tb[0]
    assert np.array_equal(bins[:whole], bins_full[:whole]) and np.array_equal(ids[:row_end[cut_row - 1]],
                                                                               ids_full[:row_end[cut_row - 1]])
    lens = bins[:, 1] - bins[:, 0]
    assert lens[whole + tb[0]:].sum() == 0 and lens[whole:whole + tb[0]].sum() == cap - row_end[cut_row - 1]
    for t in range(whole, whole + tb[0]):
        assert lens[t] <= lens_full[cut_row, t - whole]
        assert np.array_equal(ids[bins[t, 0]:bins[t, 1]], ids_full[bins_full[t, 0]:bins_full[t, 0] + lens[t]])


@pytest.mark.parametrize("W_,H_", [(272, 16368)])
def test_more_tile_rows_than_threads(W_, H_):
    """17 x 1023 tiles: the prologue that scans the rows' totals over more rows than the workgroup has threads."""
    n = 2000
    lists_agree(n, W_, H_, splats(n, W_, H_, 5, 60, seed=43))


def test_a_slab_of_several_batches_and_culled_splats_between():
    n = 700
    lists_agree(n, W, H, splats(n, W, H, 100, 300, seed=41, cull_every=7))


# ---- job orders -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def orders():
    env = dict(os.environ, GSR_TILE_SORT="t", GSR_DEEP_SPLIT_KEY="0.125")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "list_tail_orders_child.py")
    p = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    out = json.loads(line[len("RESULT "):])
    assert out["env"] == {"GSR_TILE_SORT": "t", "GSR_DEEP_SPLIT_KEY": "0.125"}
    return out


def same_as_the_separate_launch(r):
    assert r["fused"], r
    assert r["equal"] and r["differing_ints"] == 0, r
    assert r["stats_pointer"] != 0, "the library's statistics buffer"


def test_lists_all_alike_keep_the_static_order(orders):
    r = orders["alike"]
    same_as_the_separate_launch(r)
    assert r["longest_over_mean"] <= 1.5 and r["empty_slots"] > 0
    assert r["no_sentinel_left"] and r["fwd_every_tile_once"] and r["bwd_every_tile_once"]
    assert r["bwd_split_jobs"] == 0, "all alike: the backward splits nothing, whatever the threshold"
    assert r["fwd_split_jobs"] > 0, "the forward splits as told (threshold 100, mean list above it)"


def test_long_tailed_scene_splits_tiles_above_the_threshold(orders):
    r = orders["longtail"]
    same_as_the_separate_launch(r)
    assert r["longest_over_mean"] > 3 and r["empty_slots"] > 0
    assert r["fwd_every_tile_once"] and r["bwd_every_tile_once"]
    assert r["fwd_split_jobs"] > 0 and r["fwd_split_jobs"] % 4 == 0 and r["bwd_split_jobs"] > 0


def test_job_stats_are_halved_once_per_build(orders):
    """Every sum set to 16 before the list build: 8 behind it (both directions, all eight XCD lines), 4 behind the
    reference's `gsr_tile_jobs_build` on the copy; the padding of the lines is nobody's."""
    r = orders["longtail"]
    assert r["stats_after_fused_build"] == [8.0]
    assert r["stats_after_reference_build"] == [4.0]
    assert r["stats_padding"] == [16.0]


def test_non_zero_tail(orders):
    r = orders["tail64"]
    same_as_the_separate_launch(r)
    assert r["fwd_every_tile_once"] and r["bwd_every_tile_once"]
    # the tail's jobs are sub-tile jobs of tiles at or below the threshold; without a tail there are none
    assert r["fwd_split_jobs_at_or_below_threshold"] > 0 and r["bwd_split_jobs_at_or_below_threshold"] > 0
    assert orders["longtail"]["fwd_split_jobs_at_or_below_threshold"] == 0
    assert orders["longtail"]["bwd_split_jobs_at_or_below_threshold"] == 0
    assert r["no_sentinel_left"]


def test_empty_tiles_inside_the_tail(orders):
    r = orders["empty_in_tail"]
    same_as_the_separate_launch(r)
    assert r["empty_tiles"] > 100 and r["fwd_every_tile_once"] and r["bwd_every_tile_once"]
    assert r["fwd_split_jobs_of_empty_tiles"] == 0 and r["bwd_split_jobs_of_empty_tiles"] == 0


def test_rows_wider_than_256_tiles(orders):
    r = orders["wide"]
    same_as_the_separate_launch(r)
    assert r["fwd_every_tile_once"] and r["bwd_every_tile_once"] and r["no_sentinel_left"]


def test_one_order_only(orders):
    r = orders["forward_only"]
    same_as_the_separate_launch(r)
    assert r["fwd_every_tile_once"] and not r["no_sentinel_left"], "the second array is nobody's"


def test_tables_that_do_not_fit_leave_the_separate_launch(orders):
    r = orders["no_fit"]
    assert not r["fused"] and r["tail_untouched"] and r["separate_launch_wrote"], r


def test_end_to_end_prebuilt_orders_change_nothing(orders):
    """Forward and backward over lists that came with their orders against the same lists with the orders of the
    separate launch.  Gradients: float atomics in the order the waves arrive; two runs of one build differ by up to
    2e-5 of the largest value (the bound of tests/test_gpu_kernels.py for the static against the ordered launch)."""
    r = orders["end_to_end"]
    assert r["ordered"]
    assert r["prebuilt_jobs_build_calls"] == 0 and r["prebuilt_list_build_with_orders"] == 1
    assert r["separate_jobs_build_calls"] == 1 and r["separate_list_build_with_orders"] == 0
    assert r["lists_equal"] and r["orders_equal"] and r["images_equal"]
    print("gradient differences (relative to the largest value):", r["grad_rel_diff"])
    assert max(r["grad_rel_diff"]) <= 2e-5
    assert r["fallbacks"] == 0
