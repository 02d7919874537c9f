"""CPU: the float64 restatement of the absgrad rule (tests/absgrad_reference.py) against the golden vectors and the
oracle, the properties the absgrad has by construction, and the public surface of the switch."""
import inspect
import os

import numpy as np
import pytest

import absgrad_reference as A
from oracle import oracle as O
from test_oracle_golden import SCENES, fix_bins, rel_err


def _golden(golden_dir, name):
    g = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    W, H = (int(v) for v in g["img_size"])
    bw = int(g["block_width"])
    assert bw == 16
    tb = ((W + bw - 1) // bw, (H + bw - 1) // bw, 1)
    bins = fix_bins(g)
    _, Ts, idx = O.rasterize_forward(tb, (bw, bw, 1), (W, H, 1), g["gaussian_ids_sorted"], bins, g["xys"], g["conics"],
                                     g["colors"], g["opacities"], g["background"])
    args = (g["gaussian_ids_sorted"], bins, g["xys"], g["conics"], g["colors"], g["opacities"], g["background"], Ts, idx,
            g["v_out_img"], g["v_out_alpha"])
    return g, H, W, args


def _scene(sc):
    ids, bins, Ts, idx = A.oracle_lists(sc)
    return sc["H"], sc["W"], (ids, bins, sc["xys"], sc["conics"], sc["colors"], sc["opacities"], sc["background"], Ts,
                              idx, sc["v_img"], sc["v_alpha"])


@pytest.fixture(scope="module")
def scenes():
    return {"small": A.small_scene(0), "deep": A.deep_scene(0), "single": A.single_splat_scene()}


@pytest.mark.parametrize("name", SCENES)
def test_signed_sum_equals_the_golden_gradient(golden_dir, name):
    """The restated rule's signed v_xy is the reference implementation's autograd gradient, under the rule and the
    numbers of test_oracle_golden.py::test_rasterize_backward."""
    g, H, W, args = _golden(golden_dir, name)
    v_xy, v_abs, _ = A.absgrad_reference(H, W, *args)
    ref = g["g_xys"]
    floor = 1e-3 * max(1.0, float(np.abs(ref).max()))
    assert rel_err(v_xy, ref, floor).max() < 1e-3
    assert (v_abs >= np.abs(v_xy)).all()


def _oracle_distance(H, W, args):
    v_xy = A.absgrad_reference(H, W, *args)[0]
    o64 = O.rasterize_backward_fp64(H, W, 16, *args)[0]
    return float(np.abs(v_xy - o64).max() / np.abs(o64).max())


def test_signed_sum_equals_the_float64_oracle(golden_dir, scenes):
    """... and oracle.rasterize_backward_fp64 on the same lists and decisions.  Measured here (max |ref - oracle| /
    max |oracle| over the five golden scenes and the three scenes of the GPU tests): 5.6e-16 -- two float64
    accumulations in different orders; the assertion is ten times that."""
    cases = [_golden(golden_dir, name)[1:] for name in SCENES] + [_scene(sc) for sc in scenes.values()]
    worst = max(_oracle_distance(*c) for c in cases)
    print(f"reference against the float64 oracle: {worst:.3e}")
    assert worst <= 5.6e-15


@pytest.mark.parametrize("name", ["small", "deep"])
def test_abs_dominates_signed_and_the_scenes_meet_the_slack_cap(scenes, name):
    """abs >= |signed| elementwise; the scenes of the GPU tests cancel (the absgrad is several times the signed
    norm: what the switch is for) and at most 5 % of their Gaussians carry decision slack."""
    H, W, args = _scene(scenes[name])
    v_xy, v_abs, U = A.absgrad_reference(H, W, *args)
    assert (v_abs >= np.abs(v_xy)).all()
    assert v_abs.sum() > 3 * np.abs(v_xy).sum()
    assert (v_abs > 0).any(axis=1).mean() > 0.9
    print(f"{name}: slack on {A.slack_fraction(U):.4f} of the Gaussians")
    assert A.slack_fraction(U) <= 0.05


def test_small_scene_spans_the_list_lengths_it_is_for(scenes):
    """Who reaches which tile of the 40 x 24 scene, by the exact criterion (some pixel centre of the tile gets
    alpha >= 1/255): 130, 101, 70, 23, 1, 1."""
    sc = scenes["small"]
    H, W = sc["H"], sc["W"]
    py, px = np.mgrid[0:H, 0:W]
    lens = np.zeros(6, int)
    for g in range(sc["xys"].shape[0]):
        a, b, c = sc["conics"][g].astype(np.float64)
        dx, dy = sc["xys"][g, 0] - px, sc["xys"][g, 1] - py
        alpha = sc["opacities"][g, 0] * np.exp(-(0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy))
        for t in np.unique(((py // 16) * 3 + px // 16)[alpha >= A.ALPHA_MIN]):
            lens[t] += 1
    assert lens.tolist() == A.SMALL_LIST_LENGTHS


def test_sign_coherent_single_splat(scenes):
    """A Gaussian wholly to one side of the image with b = 0 under cotangents of one sign: no cancellation in x, so
    abs_x == |v_xy_x| to the rounding of 256 same-sign additions; y does cancel."""
    H, W, args = _scene(scenes["single"])
    v_xy, v_abs, U = A.absgrad_reference(H, W, *args)
    assert not U.any()
    assert abs(v_abs[0, 0] - abs(v_xy[0, 0])) <= 256 * 2.0 ** -24 * v_abs[0, 0]
    assert v_abs[0, 0] > 1.0 and v_abs[0, 1] > 10 * abs(v_xy[0, 1])


def test_two_segment_lists_are_one_walk(scenes):
    """A tile's list cut in two (`bins2`, `idx_base2`: the two-round layout) gives the single walk's sums."""
    sc = scenes["small"]
    H, W, args = _scene(sc)
    ids, bins = args[0], args[1]
    cut = bins[:, 0] + (bins[:, 1] - bins[:, 0]) // 3
    first, second = [], []
    bins1, bins2 = np.zeros_like(bins), np.zeros_like(bins)
    for t in range(bins.shape[0]):
        bins1[t] = (len(first), len(first) + cut[t] - bins[t, 0])
        first.extend(ids[bins[t, 0]:cut[t]])
        bins2[t] = (len(second), len(second) + bins[t, 1] - cut[t])
        second.extend(ids[cut[t]:bins[t, 1]])
    ids2 = np.array(first + second, np.int32)
    # final_idx of the single walk, moved to the two-segment array
    where = np.zeros(ids.shape[0], np.int64)
    for t in range(bins.shape[0]):
        for e in range(bins[t, 0], bins[t, 1]):
            where[e] = bins1[t, 0] + e - bins[t, 0] if e < cut[t] else len(first) + bins2[t, 0] + e - cut[t]
    idx2 = where[np.clip(args[8], 0, ids.shape[0] - 1)]
    one = A.absgrad_reference(H, W, *args)
    two = A.absgrad_reference(H, W, ids2, bins1, *args[2:8], idx2, *args[9:], bins2=bins2, idx_base2=len(first))
    for a, b in zip(one, two):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-300)


# ---- the surface of the switch (each of these fails without it) ------------------------------------------------------

def test_view_spec_takes_absgrad():
    from gs_fused import DensifyStats, ViewSpec

    assert ViewSpec(24, 40, 30.0, 30.0, 20.0, 12.0, 0).absgrad is False
    spec = ViewSpec(24, 40, 30.0, 30.0, 20.0, 12.0, 0, absgrad=True)
    assert spec.absgrad and spec != ViewSpec(24, 40, 30.0, 30.0, 20.0, 12.0, 0)  # (a graph's key tells them apart)
    stats = DensifyStats(7, "cpu", 40)
    assert tuple(stats.absgrad.shape) == (7, 2) and not stats.absgrad.any()


def test_train_config_refuses_absgrad_on_the_cpu():
    import torch

    from harness.train import TrainConfig, train

    assert TrainConfig().absgrad is False
    with pytest.raises(ValueError, match=r"absgrad.*CUDA"):
        train(TrainConfig(absgrad=True), torch.device("cpu"))


def test_rasterize_functions_take_absgrad():
    from gs_fused import rasterize_gaussians_rgbd
    from rasterizer import rasterize_gaussians

    for fn in (rasterize_gaussians, rasterize_gaussians_rgbd):
        p = inspect.signature(fn).parameters["absgrad"]
        assert p.default is False


def test_absgrad_needs_the_16_px_three_channel_kernel():
    import torch

    from rasterizer import rasterize_gaussians

    z = torch.zeros
    for bw, ch in ((8, 3), (16, 4)):
        with pytest.raises(ValueError, match="absgrad"):
            rasterize_gaussians(z(1, 2), z(1), z(1, dtype=torch.int32), z(1, 3), z(1, dtype=torch.int32), z(1, ch),
                                z(1, 1), 16, 16, bw, absgrad=True)


def test_header_declares_what_the_bindings_load():
    from rasterizer.cuda import _backend

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "gsraster.h")).read()
    for s in ("gsr_rasterize_backward_abs", "gsr_rasterize_backward_two_abs", "gsr_rasterize_backward_det_abs"):
        assert s + "(" in src and s in _backend.SYMBOLS and hasattr(_backend.lib(), s)
    grads = src[src.index("typedef struct gsr_view_grads"):src.index("} gsr_view_grads;")]
    assert grads.rstrip().endswith("float *v_xy_abs;")  # appended: every earlier field keeps its offset
    from gs_fused.render import _ViewGrads

    assert _ViewGrads._fields_[-1][0] == "v_xy_abs"
