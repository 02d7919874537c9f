"""GPU: the list builders whose LDS and register footprints were cut for residency (csrc/tile_partition2.hip `emit`,
csrc/sort_bucket.hip `scatter`) on the inputs that reach what changed in them.

Lists: the two-level partition against the banded single-pass lists, ids and bins bit for bit -- the comparison of
tests/test_gpu_kernels.py::test_two_level_partition_equals_banded_lists -- on splats given directly in screen space
(centre, integer radius, conic, opacity, depth), so that a few hundred of them fix how many (Gaussian, row) items a
slab holds and how many entries a batch writes.  A grid above 16384 tiles takes the two-level path at any list size.

Depth order: against `torch.sort(stable=True)` on the key the kernels define (the depth's bits with the sign cleared,
0 for a culled splat); the expectation is first derived on the CPU from the generator alone."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BW = 16


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def splats(n, W, H, r_lo, r_hi, seed, cull_every=0, one_row=None):
    """n splats in screen space: radius = ceil(3 sigma_max) like the projection's, anisotropic conics."""
    rng = np.random.default_rng(seed)
    radii = rng.integers(r_lo, r_hi + 1, n).astype(np.int32)
    xys = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1).astype(np.float32)
    if one_row is not None:  # centred in one tile row, box inside it
        xys[:, 1] = BW * one_row + 8.0 + rng.uniform(-1, 1, n).astype(np.float32)
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
    return dict(xys=cu(xys), radii=cu(radii), conics=cu(conics), opac=cu(opac), depths=cu(depths)), radii


def box_rows(g, radii, H):
    """Bounds on the (Gaussian, row) items of all splats together: the tile rows their boxes span, within the image."""
    y = g["xys"][:, 1].cpu().numpy().astype(np.float64)
    span = np.minimum(H, y + radii) - np.maximum(0.0, y - radii)
    return int((np.floor(span / BW) - 1).clip(0).sum()), int((np.ceil(span / BW) + 1).sum())


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
    return I1, cnt1


def test_slab_of_several_batches_reloads_its_records():
    """600 splats of 150-300 px on 129 x 129 tiles: a 256-Gaussian slab holds several thousand (Gaussian, row) items,
    so `emit` loops over batches of 1024 and derives every batch after the first from reloaded records."""
    n, W, H = 600, 2064, 2064
    g, radii = splats(n, W, H, 150, 300, seed=11)
    at_least, _ = box_rows(g, radii, H)
    assert at_least > 3 * 3 * 1024  # three slabs: one of them holds more than three batches
    lists_agree(n, W, H, g)


def test_batches_above_the_start_mask_size():
    """The same image, radii around 600 px: a batch of 1024 items writes far more than 16384 entries (rows of ~60
    tiles), the branch that finds an entry's item by binary search."""
    n, W, H = 600, 2064, 2064
    g, radii = splats(n, W, H, 550, 650, seed=12)
    I, _ = lists_agree(n, W, H, g)
    _, at_most = box_rows(g, radii, H)
    assert I > 2 * 16 * at_most  # an item writes 32 entries on average, a full batch of 1024 twice the mask size


@pytest.mark.parametrize("W,H", [(272, 16368), (16384, 272)])
def test_more_tile_rows_than_threads_and_the_widest_row_tables(W, H):
    """17 x 1023 tiles (the row scans run over more rows than the workgroup has threads; the per-row tables of `emit`
    at their widest) and 1024 x 17 (the widest rows)."""
    n = 2000
    g, _ = splats(n, W, H, 5, 60, seed=13)
    lists_agree(n, W, H, g)


def test_second_slab_of_one_gaussian():
    n, W, H = 257, 2064, 2064
    g, _ = splats(n, W, H, 20, 120, seed=14)
    lists_agree(n, W, H, g)


def test_a_third_of_the_gaussians_culled():
    n, W, H = 3000, 2064, 2064
    g, radii = splats(n, W, H, 4, 90, seed=15, cull_every=3)
    assert (radii == 0).sum() == 1000
    lists_agree(n, W, H, g)


def test_every_visible_gaussian_in_one_tile_row():
    n, W, H = 3000, 2064, 2064
    g, _ = splats(n, W, H, 1, 6, seed=16, cull_every=5, one_row=77)
    I, cnt = lists_agree(n, W, H, g)
    import rasterizer.cuda as C

    tb = ((W + BW - 1) // BW, (H + BW - 1) // BW, 1)
    cntb, _ = C.count_reach(g["xys"], g["radii"], g["conics"], g["opac"], tb, bands=C.tile_bands(tb))
    per_band = cntb.view(C.tile_bands(tb), n).sum(1)
    assert int((per_band > 0).sum()) == 1 and int(per_band.sum()) == I


# ---- depth order ------------------------------------------------------------------------------------------------
# Whole chunks of 4096, one item more, one less than two, three chunks and one -- and the same remainders above 65536
# items, from where the public entry sorts with the bucket pass (csrc/binning_fast.hip); below, it takes the
# small-size sorter, which must agree all the same.
SIZES = [4_096, 4_097, 8_191, 12_289, 65_536 + 4_096, 65_536 + 4_097, 65_536 + 8_191, 65_536 + 12_289]


def key_set(name, n, rng):
    """-> depths f32[n], radii i32[n], and the expected order derived from the generator alone."""
    radii = np.ones(n, np.int32)
    idx = np.arange(n)
    if name == "equal":
        d = np.full(n, 3.25, np.float32)
        expect = idx
    elif name == "two_depths":
        pick = rng.integers(0, 2, n)
        d = np.where(pick == 0, np.float32(2.0), np.float32(7.5)).astype(np.float32)
        expect = np.concatenate([idx[pick == 0], idx[pick == 1]])
    elif name == "twelve_octaves":
        # a random permutation of n distinct, increasing depths over [2^-4, 2^8): the order is the inverse permutation
        grid = np.exp2(np.linspace(-4.0, 8.0, n, endpoint=False)).astype(np.float32)
        assert (np.diff(grid) > 0).all()
        perm = rng.permutation(n)
        d = np.empty(n, np.float32)
        d[perm] = grid
        expect = perm
    elif name == "half_culled":
        grid = np.linspace(1.0, 40.0, n).astype(np.float32)
        assert (np.diff(grid) > 0).all()
        perm = rng.permutation(n)
        d = np.empty(n, np.float32)
        d[perm] = grid
        culled = rng.permutation(n)[: n // 2]
        radii[culled] = 0
        vis = radii[perm] > 0  # culled first (key 0) by index, then the visible ones by depth
        expect = np.concatenate([np.sort(culled), perm[vis]])
    else:
        raise AssertionError(name)
    return d, radii, expect.astype(np.int64)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["equal", "two_depths", "twelve_octaves", "half_culled"])
def test_depth_order_is_the_stable_sort_of_the_keys(n, name, monkeypatch):
    import rasterizer.cuda as C

    monkeypatch.setenv("GSR_DEPTH_SORT", "bucket")  # (a view of equal depths would send later calls to the LSD passes)
    rng = np.random.default_rng(n * 7 + len(name))
    d, radii, expect = key_set(name, n, rng)
    key = torch.from_numpy((d.view(np.uint32) & 0x7FFFFFFF).astype(np.int64) * (radii > 0))
    ref = torch.sort(key, stable=True).indices
    assert torch.equal(ref, torch.from_numpy(expect)), "the test's own expectation"
    order, cum = C.depth_order(cu(d), cu(radii), None)
    assert cum is None and torch.equal(order.cpu().long(), ref)
    tiles = rng.integers(0, 5, n).astype(np.int32) * (radii > 0)
    order2, cum2 = C.depth_order(cu(d), cu(radii), cu(tiles))
    assert torch.equal(order2.cpu().long(), ref)
    assert np.array_equal(cum2.cpu().numpy(), np.cumsum(tiles[expect]).astype(np.int32))
