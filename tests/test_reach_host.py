"""Pins the inputs of tests/test_gpu_reach.py without a GPU: the float64 truth of tests/reach_reference.py classifies
the families as designed, the float32 emulation of the 16-px list rule keeps every pair it must, and the grazing
family has teeth against a margin that is short by 0.2 % in alpha or by half a pixel."""
import numpy as np
import pytest

import reach_reference as R
from oracle import oracle as O


@pytest.mark.parametrize("name", R.FAMILIES)
def test_row_rule_keeps_every_must_keep_pair(name):
    sc, tr = R.family(name), R.truth(name)
    live = tr["live16"]
    g, tx, ty = R.box_pairs(sc)
    assert np.array_equal(g, live["g"]) and np.array_equal(tx, live["rx"]) and np.array_equal(ty, live["ry"])
    assert g.size == int(sc["num_tiles_hit"].sum()) == tr["ids"].size  # the pairs ARE the bounding-box lists' entries
    keep = R.row_rule32(sc)
    must = live["cls"] == R.MUST_KEEP
    dropped = np.nonzero(must & ~keep)[0]
    print(f"{name}: {g.size} pairs, {int(must.sum())} must-keep, the rule keeps {int(keep.sum())}")
    assert dropped.size == 0, [(int(g[i]), int(tx[i]), int(ty[i]), float(live["amax"][i] * 255)) for i in dropped[:5]]
    assert 0 < must.sum() and keep.sum() < g.size or name == "norule"  # the rule culls something, and not everything


@pytest.mark.parametrize("name", R.FAMILIES)
def test_family_counts_are_as_designed(name):
    sc, tr = R.family(name), R.truth(name)
    assert sc["H"] <= 128 and sc["W"] <= 128 and sc["xys"].shape[0] <= 600
    assert np.unique(sc["depths"]).size == sc["depths"].size
    for unit in (16, 8):
        cls = tr[f"live{unit}"]["cls"]
        counts = [int((cls == c).sum()) for c in (R.MUST_KEEP, R.DEAD, R.UNDECIDED)]
        print(f"{name} unit {unit}: must-keep {counts[0]}, dead {counts[1]}, undecided {counts[2]}")
        if name.startswith("graze"):
            assert counts[2] == 0
        else:
            assert counts[2] <= 0.02 * cls.size
        assert counts[0] > 0 and (counts[1] > 0 or name == "norule" or unit == 16)
    share = float(tr["unstable"].mean())
    print(f"{name}: unstable share of the image {share:.4f}")
    assert share <= 0.02  # the cap `check_image` uses (tests/test_gpu_kernels.py)


@pytest.mark.parametrize("name", ["graze16", "graze8"])
def test_graze_targets(name):
    sc, tr = R.family(name), R.truth(name)
    unit = sc["unit"]
    live = tr[f"live{unit}"]
    tp = R.target_pairs(sc, live, unit)
    tx, ty = sc["target"][:, 0], sc["target"][:, 1]
    assert (sc["colors"] >= 0.5).all()
    assert (sc["smin"] > 0.05).all() and (sc["smin"] < 5.4).all()
    for delta in R.DELTAS:
        m = sc["delta"] == delta
        assert m.sum() >= 150
        assert np.bincount(sc["case"][m], minlength=len(R.GRAZE_CASES)).min() >= m.sum() // len(R.GRAZE_CASES)
        want = R.MUST_KEEP if delta > 0 else R.DEAD
        assert (live["cls"][tp][m] == want).all()
        # the target's alpha is (1 + delta) / 255 up to the rounding of the float32 opacity
        np.testing.assert_allclose(live["amax"][tp][m] * 255.0, 1.0 + delta, rtol=0, atol=2e-7)
    assert not tr["unstable"][ty, tx].any()          # every target pixel is stable ...
    assert sc["T_front"].min() >= 0.5 and sc["others_live"].max() <= 1  # ... at most two overlap there, T in front >= 0.5
    # the centre is outside the target rectangle
    x0, y0 = sc["rect"][:, 0] * unit, sc["rect"][:, 1] * unit
    inside = ((sc["xys"][:, 0] >= x0) & (sc["xys"][:, 0] <= x0 + unit - 1)
              & (sc["xys"][:, 1] >= y0) & (sc["xys"][:, 1] <= y0 + unit - 1))
    assert not inside.any()
    if unit == 8:  # the target sub-tile is its tile's only live one
        l8 = tr["live8"]
        for i in np.nonzero(sc["delta"] > 0)[0][::7]:
            m = (l8["g"] == i) & (l8["rx"] // 2 == tx[i] // 16) & (l8["ry"] // 2 == ty[i] // 16)
            assert (l8["cls"][m] == R.MUST_KEEP).sum() == 1
    # a dropped target pair would be seen: its contribution is at least (1/255) x colour x T
    bg = sc["background"].astype(np.float64)
    pos = sc["delta"] > 0
    contrib = np.abs(sc["colors"][pos].astype(np.float64) - bg[None, :]).max(axis=1) * sc["T_front"][pos] / 255.0
    print(f"{name}: smallest image change of a dropped target pair {contrib.min():.2e}")
    assert contrib.min() > 5e-4  # five times the 1e-4 image tolerance
    solo = R.solo_splats(sc, tr)
    print(f"{name}: {solo.size} splats whose target is their only live pixel")
    assert solo.size >= 20


def test_graze16_has_teeth():
    """A bound on sigma that is tighter by 0.002 (0.2 % in alpha), or a row interval that is shorter by half a pixel,
    drops must-keep pairs of graze16; rounding alone (all three margins at zero) is counted for the record."""
    sc, tr = R.family("graze16"), R.truth("graze16")
    must = tr["live16"]["cls"] == R.MUST_KEEP
    dropped = {}
    for label, kw in (("log margin -0.002", dict(log_margin=-0.002)), ("pixel margin -0.5", dict(px_margin=-0.5)),
                      ("all margins 0", dict(log_margin=0.0, rel_margin=0.0, px_margin=0.0))):
        dropped[label] = int((must & ~R.row_rule32(sc, **kw)).sum())
        print(f"graze16, {label}: {dropped[label]} of {int(must.sum())} must-keep pairs dropped")
    assert dropped["log margin -0.002"] >= 1
    assert dropped["pixel margin -0.5"] >= 1


def test_banded_truth_equals_the_dense_one():
    """`live_pairs` on a large grid evaluates only the pixels near each ellipse: the same classes as every pixel."""
    for name in ("needles", "graze16", "tiny"):
        sc, tr = R.family(name), R.truth(name)
        for unit in (16, 8):
            band = R.live_pairs(sc, unit, banded=True)
            assert np.array_equal(band["cls"], tr[f"live{unit}"]["cls"])
            big = tr[f"live{unit}"]["amax"] * 255.0 > 0.95
            assert np.array_equal(band["amax"][big], tr[f"live{unit}"]["amax"][big])


def test_large_grid_scene_row_rule():
    """The 3840 x 2160 list scene of the GPU test (needles and graze16 moved into it): the emulated rule keeps every
    must-keep pair there too -- with the compensated determinant.  With the plain float32 a c - b^2 it drops live pairs
    of needles whose determinant cancels (the device dropped the same ones before `conic_det`)."""
    sc = R.large_grid_scene()
    live = R.live_pairs(sc, 16)
    keep = R.row_rule32(sc)
    must = live["cls"] == R.MUST_KEEP
    print(f"4K: {live['g'].size} pairs, {int(must.sum())} must-keep, undecided {int((live['cls'] == R.UNDECIDED).sum())}, "
          f"the rule keeps {int(keep.sum())}")
    bad = np.nonzero(must & ~keep)[0]
    assert bad.size == 0, [(int(live["g"][i]), int(live["rx"][i]), int(live["ry"][i]), float(live["amax"][i] * 255))
                           for i in bad[:5]]
    plain = int((must & ~R.row_rule32(sc, plain_det=True)).sum())
    print(f"4K: with the plain float32 determinant {plain} must-keep pairs dropped")
    assert plain >= 1


@pytest.mark.parametrize("name", R.FAMILIES)
def test_float32_oracle_decides_like_float64_on_stable_pixels(name):
    """`composite64` against the project's float32 oracle on the same lists: the image within 1e-4 and the same
    final_idx wherever neither flags the pixel."""
    sc, tr = R.family(name), R.truth(name)
    tb = R.grid(sc) + (1,)
    img, Ts, idx, amb = O.rasterize_forward(tb, (16, 16, 1), (sc["W"], sc["H"], 1), tr["ids"], tr["bins"], sc["xys"],
                                            sc["conics"], sc["colors"], sc["opacities"], sc["background"], ambig_eps=1e-5)
    ok = ~tr["unstable"]
    assert np.abs(img - tr["img"])[ok].max() < 1e-4 and np.abs(Ts - tr["T"])[ok].max() < 1e-4
    assert np.array_equal(idx[ok], tr["idx"][ok])


@pytest.mark.parametrize("name", ["graze16", "graze8"])
def test_solo_gradients_stand_above_the_floor(name):
    """The float64 backward: every solo splat's v_opacity is non-zero and above the floor of the 1e-3 gradient rule."""
    sc, tr = R.family(name), R.truth(name)
    ref = R.backward64(name)
    solo = R.solo_splats(sc, tr)
    vo = np.abs(ref[3].reshape(-1))
    floor = 1e-3 * vo.max()
    print(f"{name}: |v_opacity| of solo splats {vo[solo].min():.3e} .. {vo[solo].max():.3e}, floor {floor:.3e}")
    assert (vo[solo] > floor).all()
