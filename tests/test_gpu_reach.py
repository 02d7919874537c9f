"""GPU: both reach culls -- the 16-px tile lists (csrc/tile_rows.h) and the 8 x 8 sub-tile mask of the staging
(csrc/raster_common.h) -- against the float64 truth of tests/reach_reference.py, on splats built to graze them.

Lists: a (splat, tile) pair with a pixel at alpha >= (1 + 1e-5) / 255 must be listed.  Images: every compositing route
in front of which the sub-tile mask sits, within the project's 1e-4 on the pixels whose decisions are stable (header
of tests/test_gpu_kernels.py); a grazing pair that a cull drops changes its target pixel by >= 5e-4
(tests/test_reach_host.py).  Gradients: 1e-3 relative with a floor of 1e-3 x the largest, against the float64
backward."""
import numpy as np
import pytest
import torch

import reach_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def cu(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the families are read-only)


def npy(t):
    return t.detach().cpu().numpy()


def on_device(sc):
    return dict(xys=cu(sc["xys"]), depths=cu(sc["depths"]), radii=cu(sc["radii"]), conics=cu(sc["conics"]),
                tiles=cu(sc["num_tiles_hit"]), opac=cu(sc["opacities"]), colors=cu(sc["colors"]),
                bg=cu(sc["background"]))


def box_lists(C, g, n, tb):
    order, cum = C.depth_order(g["depths"], g["radii"], g["tiles"])
    ids, bins = C.bin_sorted(n, int(cum[-1].item()), order, cum, g["xys"], g["radii"], tb, 16)
    return ids, bins, order


def exact_lists(C, g, n, tb, bands):
    cnt, recs = C.count_reach(g["xys"], g["radii"], g["conics"], g["opac"], tb, bands=bands)
    order, cum = C.depth_order(g["depths"], g["radii"], cnt)
    ids, bins = C.bin_sorted(n, int(cum[-1].item()), order, cum, g["xys"], g["radii"], tb, 16, recs)
    return ids, bins, cnt.view(bands, n).sum(0), order


def one_call_lists(C, g, sc, capacity):
    count = torch.zeros(1, dtype=torch.int32).pin_memory()
    ids, bins = C.rasterize_gaussians_forward(g["xys"], g["depths"], g["radii"], g["conics"], None, g["opac"], None,
                                              sc["H"], sc["W"], capacity, count, composite=False)
    torch.cuda.synchronize()
    assert 0 < int(count[0]) <= capacity
    return ids[:int(count[0])], bins


def check_lists(sc, live, order, exact, counts, label, box=None):
    """`exact` lists against the bounding-box lists `box` (both (ids, bins) as NumPy; None: against the tile boxes
    themselves, which is what those lists hold) and the float64 must-keep set."""
    n = sc["xys"].shape[0]
    tiles_x, tiles_y = R.grid(sc)
    nt = tiles_x * tiles_y

    def keys(ids, bins):
        lens = bins[:, 1] - bins[:, 0]
        assert (lens >= 0).all() and lens.sum() == ids.size
        tile = np.repeat(np.arange(nt, dtype=np.int64), lens)
        pos = np.concatenate([np.arange(a, b) for a, b in bins]) if ids.size else np.zeros(0, np.int64)
        return tile, tile * n + ids[pos].astype(np.int64), ids[pos]

    te, ke, ge = keys(*exact)
    assert np.unique(ke).size == ke.size
    # a subsequence of the bounding-box list, tile by tile: the same pairs or fewer, in the same (depth) order
    if box is not None:
        _, kb, _ = keys(*box)
        assert np.unique(kb).size == kb.size == int(sc["num_tiles_hit"].sum())
        assert np.isin(ke, kb).all(), f"{label}: an entry that the bounding-box lists do not have"
    tbox = R.tile_box(sc["xys"], sc["radii"], tiles_x, tiles_y)[ge]
    ex, ey = te % tiles_x, te // tiles_x
    assert ((ex >= tbox[:, 0]) & (ex < tbox[:, 2]) & (ey >= tbox[:, 1]) & (ey < tbox[:, 3])).all(), \
        f"{label}: an entry outside its splat's tile box"
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    same_tile = te[1:] == te[:-1]
    assert (np.diff(rank[ge])[same_tile] > 0).all(), f"{label}: a tile's list is out of depth order"
    assert np.array_equal(np.bincount(ge, minlength=n), counts), f"{label}: counts differ from the occurrences"
    must = live["cls"] == R.MUST_KEEP
    want = (live["ry"][must] * tiles_x + live["rx"][must]) * n + live["g"][must]
    missing = ~np.isin(want, ke)
    worst = [(int(live["g"][must][i]), int(live["rx"][must][i]), int(live["ry"][must][i]),
              float(live["amax"][must][i] * 255)) for i in np.nonzero(missing)[0][:8]]
    print(f"{label}: {int(sc['num_tiles_hit'].sum())} box entries, {ke.size} exact, {int(must.sum())} must-keep, "
          f"{int(missing.sum())} missing")
    assert not missing.any(), f"{label}: live pairs dropped (splat, tile x, tile y, 255 amax): {worst}"
    return ke.size


@pytest.mark.parametrize("name", R.FAMILIES)
def test_lists_keep_every_live_pair(name):
    import rasterizer.cuda as C

    sc, tr = R.family(name), R.truth(name)
    n, tb = sc["xys"].shape[0], R.grid(sc) + (1,)
    g = on_device(sc)
    ids_b, bins_b, order = box_lists(C, g, n, tb)
    assert np.array_equal(npy(ids_b), tr["ids"]) and np.array_equal(npy(bins_b), tr["bins"])  # the truth's lists
    ids_e, bins_e, cnt, order_e = exact_lists(C, g, n, tb, C.tile_bands(tb))
    assert torch.equal(order, order_e)
    ids_o, bins_o = one_call_lists(C, g, sc, ids_b.numel())
    assert torch.equal(ids_e, ids_o) and torch.equal(bins_e, bins_o)
    kept = check_lists(sc, tr["live16"], npy(order), (npy(ids_e), npy(bins_e)), npy(cnt), name,
                       box=(tr["ids"], tr["bins"]))
    if name == "norule":  # no culling for what is not positive definite, nor for a NaN opacity
        whole = sc["whole_box"]
        assert whole.sum() >= 28
        assert np.array_equal(npy(cnt)[whole], sc["num_tiles_hit"][whole])
    else:
        assert kept < tr["ids"].size  # the cull is at work


def test_lists_on_a_large_grid():
    """3840 x 2160: tile-row bands and the two-level partition, lists only.  (The bounding-box lists of these needles
    would hold ten million entries; the exact lists are held to the tile boxes themselves.)"""
    import rasterizer.cuda as C

    sc = R.large_grid_scene()
    n, tb = sc["xys"].shape[0], R.grid(sc) + (1,)
    live = R.live_pairs(sc, 16)
    g = on_device(sc)
    nb = C.tile_bands(tb)
    assert nb > 1
    ids_e, bins_e, cnt, order = exact_lists(C, g, n, tb, nb)   # tile-row bands
    ids_t, bins_t, cnt_t, _ = exact_lists(C, g, n, tb, 1)      # one count per Gaussian: the two-level partition
    assert torch.equal(ids_e, ids_t) and torch.equal(bins_e, bins_t) and torch.equal(cnt, cnt_t)
    ids_o, bins_o = one_call_lists(C, g, sc, ids_e.numel() + 4096)
    assert torch.equal(ids_e, ids_o) and torch.equal(bins_e, bins_o)
    check_lists(sc, live, npy(order), (npy(ids_e), npy(bins_e)), npy(cnt), "4K")


ROUTES = ("exact", "box", "generic", "four waves", "four waves box", "default")


def composite(C, monkeypatch, route, sc, g, lists):
    """One compositing route -> (img, T, idx, ids) as NumPy; `ids`: the list that idx points into."""
    tb = R.grid(sc) + (1,)
    ids, bins = lists["box" if route in ("box", "generic", "four waves box") else "exact"]
    a = (tb, (16, 16, 1), (sc["W"], sc["H"], 1), ids, bins, g["xys"], g["conics"], g["colors"], g["opac"], g["bg"])
    with monkeypatch.context() as m:
        if route != "default":  # (the default policy of a small grid splits the tiles above 96 entries)
            m.setattr(C, "depth_segments", lambda *a, **k: (1, 0))
            m.setattr(C, "deep_tile_threshold", lambda *a, **k: 1 if route.startswith("four waves") else 0)
        out = (C.nd_rasterize_forward if route == "generic" else C.rasterize_forward)(*a)
    return tuple(npy(t) for t in out) + (npy(ids),)


@pytest.mark.parametrize("name", R.FAMILIES)
def test_images_equal_the_float64_forward(name, monkeypatch):
    import rasterizer.cuda as C

    sc, tr = R.family(name), R.truth(name)
    n, tb = sc["xys"].shape[0], R.grid(sc) + (1,)
    g = on_device(sc)
    ids_b, bins_b, _ = box_lists(C, g, n, tb)
    ids_e, bins_e, _, _ = exact_lists(C, g, n, tb, 1)
    lists = {"box": (ids_b, bins_b), "exact": (ids_e, bins_e)}
    ok = ~tr["unstable"]
    assert ok.mean() >= 0.98
    drawn = ok & (tr["T"] < 1.0)
    last = tr["ids"][tr["idx"]]  # the Gaussian drawn last, whatever the list
    graze = name.startswith("graze")
    if graze:
        ty, tx = sc["target"][:, 1], sc["target"][:, 0]
        assert ok[ty, tx].all()
        mirror = sc["delta"] < 0
    failures = []
    for route in ROUTES:
        img, T, idx, ids = composite(C, monkeypatch, route, sc, g, lists)
        err = np.maximum(np.abs(img - tr["img"]).max(axis=2), np.abs(T - tr["T"]))
        err = np.where(ok, np.nan_to_num(err, nan=np.inf), 0.0)
        line = f"{name} / {route}: largest error on stable pixels {err.max():.2e}"
        if graze:
            line += f", on target pixels {err[ty, tx].max():.2e}, on the mirrors' {err[ty, tx][mirror].max():.2e}"
        print(line)
        wrong_idx = int((ids[idx][drawn] != last[drawn]).sum()) + int((T[ok & ~drawn] != 1.0).sum())
        if err.max() > 1e-4 or wrong_idx:
            at = np.unravel_index(err.argmax(), err.shape)
            failures.append(f"{route}: error {err.max():.3e} at pixel (x {at[1]}, y {at[0]}), {wrong_idx} pixels with "
                            f"another last splat")
    assert not failures, failures


def grad_close(mine, ref, name, tol=1e-3):
    floor = 1e-3 * max(1e-6, float(np.abs(ref).max()))
    e = np.abs(mine - ref) / np.maximum(np.abs(ref), floor)
    print(f"{name}: largest relative error {e.max():.2e}")
    return None if e.max() < tol else f"{name}: {e.max():.3e} at {np.unravel_index(e.argmax(), e.shape)}"


@pytest.mark.parametrize("name", ["graze16", "graze8"])
def test_gradients_equal_the_float64_backward(name, monkeypatch):
    import rasterizer.cuda as C

    sc, tr = R.family(name), R.truth(name)
    n, tb = sc["xys"].shape[0], R.grid(sc) + (1,)
    H, W = sc["H"], sc["W"]
    ref = R.backward64(name)
    solo = R.solo_splats(sc, tr)
    vo_ref = ref[3].reshape(-1)
    floor = 1e-3 * np.abs(vo_ref).max()
    assert solo.size >= 20 and (np.abs(vo_ref[solo]) > floor).all()  # no solo gradient hides under the floor
    g = on_device(sc)
    ids_e, bins_e, _, _ = exact_lists(C, g, n, tb, 1)
    v_img, v_alpha = (cu(v) for v in R.cotangents(name))
    monkeypatch.setattr(C, "depth_segments", lambda *a, **k: (1, 0))
    failures = []
    for route, threshold in (("single walk", 0), ("four waves", 1)):
        monkeypatch.setattr(C, "deep_tile_threshold", lambda *a, **k: threshold)
        _, Ts, idx = C.rasterize_forward(tb, (16, 16, 1), (W, H, 1), ids_e, bins_e, g["xys"], g["conics"], g["colors"],
                                         g["opac"], g["bg"])
        got = C.rasterize_backward(H, W, 16, ids_e, bins_e, g["xys"], g["conics"], g["colors"], g["opac"], g["bg"], Ts,
                                   idx, v_img, v_alpha)
        for t, r, nm in zip(got, ref, ("v_xy", "v_conic", "v_colors", "v_opacity")):
            failures.append(grad_close(npy(t).astype(np.float64), r.reshape(npy(t).shape), f"{name} / {route} / {nm}"))
        vo = npy(got[3]).reshape(-1).astype(np.float64)
        e = np.abs(vo[solo] - vo_ref[solo]) / np.maximum(np.abs(vo_ref[solo]), floor)
        print(f"{name} / {route}: v_opacity of the {solo.size} one-pixel splats, largest relative error {e.max():.2e}, "
              f"{int((vo[solo] == 0).sum())} zero")
        if (vo[solo] == 0).any() or e.max() >= 1e-3:
            failures.append(f"{route}: one-pixel splats {solo[(vo[solo] == 0) | (e >= 1e-3)][:8]} lost their gradient")
    failures = [f for f in failures if f]
    assert not failures, failures
