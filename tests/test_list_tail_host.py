"""Host: argument handling of `gsr_bin_sorted_dev_jobs` (every case is refused before anything is launched) and the
package's bookkeeping around it -- which words the list build is given, when the forward takes the orders as prebuilt
and when it falls back to `gsr_tile_jobs_build` (counted).

(The refused calls leave their message in the library's last-error buffer, which nothing clears: this module runs behind
tests/test_capi_and_host.py, which asserts that a fresh library has none.)"""
import ctypes as C

import pytest
import torch

ORDERED, PREBUILT, SECOND = 1 << 30, 1 << 29, 1 << 28


def call(lib, built, num_points=10, capacity=100, tiles_x=8, tiles_y=8, block_width=16, first=0, second=0):
    null = C.c_void_p(None)
    return lib.gsr_bin_sorted_dev_jobs(C.c_int(num_points), C.c_int(capacity), null, null, null, null, null,
                                       C.c_int(tiles_x), C.c_int(tiles_y), C.c_uint(block_width), C.c_int(1), null, null,
                                       null, null, null, C.c_size_t(0), C.c_int(first), C.c_int(second), built, null)


def test_bad_arguments_are_refused_and_nothing_is_reported_built():
    from rasterizer.cuda._backend import lib as load

    lib = load()
    err = lambda: lib.gsr_last_error().decode()
    assert call(lib, None) != 0 and "jobs_built" in err()
    cases = [
        (dict(capacity=0), "positive"),
        (dict(num_points=0), "positive"),
        (dict(first=100 | ORDERED, second=200), "GSR_DEEP_ORDERED"),            # a second word that is no order
        (dict(first=100 | ORDERED, second=200 | ORDERED), "same array"),         # both name the first array
        (dict(first=100 | ORDERED | SECOND, second=200 | ORDERED | SECOND), "same array"),
        (dict(first=100 | ORDERED, second=200 | ORDERED | SECOND, block_width=1), "block_width"),
        (dict(first=100 | ORDERED, second=200 | ORDERED | SECOND, tiles_x=0), "empty tile grid"),
        (dict(first=100 | ORDERED, second=200 | ORDERED | SECOND), "null pointer"),  # (tile_bins)
        (dict(first=100, second=200 | ORDERED | SECOND), "null pointer"),         # no order asked for: the plain build's checks
    ]
    for kw, what in cases:
        built = C.c_int(7)
        assert call(lib, C.byref(built), **kw) != 0, kw
        assert what in err(), (kw, err())
        assert built.value == 0, kw


def test_the_forward_takes_the_list_builds_orders_or_falls_back_counted(monkeypatch):
    import rasterizer.cuda as R
    import rasterizer.rasterize as rast

    t = (120, 68, 1)  # 1920 x 1080
    nt = t[0] * t[1]
    bins = R.alloc_tile_bins(t, "cpu")
    fwd, bwd = R._list_build_orders(bins, 8_000_000, nt, t)
    assert fwd & ORDERED and bwd & ORDERED and bwd & SECOND and not fwd & SECOND and not (fwd | bwd) & PREBUILT
    assert fwd == R.deep_arg(bins, 8_000_000, nt, tile_bounds=t)
    assert bwd == R.deep_arg(bins, 8_000_000, nt, backward=True, tile_bounds=t)
    # as bin_sorted marks the lists it built with these words
    bins._gsr_jobs_bwd, bins._gsr_jobs_fwd, bins._gsr_jobs_by_list_build = bwd, fwd, True
    calls = []
    monkeypatch.setattr(R, "_call", lambda name, *a: calls.append(name))
    monkeypatch.setattr(R, "_stream", lambda dev: None)
    before = rast.counters["orders_prebuilt_fallbacks"]
    assert R.forward_orders(bins, 8_000_000, nt, t, "cpu") == fwd | PREBUILT and calls == []
    assert R.backward_order(bins, 8_000_000, nt, t) == bwd | PREBUILT
    assert rast.counters["orders_prebuilt_fallbacks"] == before
    # another list count -> another threshold: the separate launch, once, and the lists are marked with the new words
    got = R.forward_orders(bins, 16_000_000, nt, t, "cpu")
    assert calls == ["gsr_tile_jobs_build"] and got & PREBUILT and got != fwd | PREBUILT
    assert rast.counters["orders_prebuilt_fallbacks"] == before + 1
    assert R.forward_orders(bins, 16_000_000, nt, t, "cpu") == got and calls == ["gsr_tile_jobs_build"]
    assert rast.counters["orders_prebuilt_fallbacks"] == before + 1
    # a small grid has no orders: the list build is given none
    small = (30, 17, 1)
    assert R._list_build_orders(R.alloc_tile_bins(small, "cpu"), 300_000, small[0] * small[1], small) == (0, 0)
