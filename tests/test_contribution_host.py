"""CPU: the float64 restatement of the contribution walk (tests/contribution_reference.py) on hand-computed rays, the
cap on the near share of every case the GPU test runs (tests/test_gpu_contribution.py: the seeds are chosen so that the
reference alone meets it), and the host side of gs_fused/contribution.py and of the trainer's `prune_at`."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import contribution_reference as R


def ray(opac):
    """A 1 x 1 image whose pixel sits exactly on the centres of Gaussians in list order: sigma = 0, alpha = opacity."""
    n = len(opac)
    return (np.arange(n, dtype=np.int32), np.array([[0, n]], np.int32), np.zeros((n, 2), np.float32),
            np.tile(np.array([[0.25, 0.0, 0.25]], np.float32), (n, 1)), np.asarray(opac, np.float32))


def test_one_pixel_two_splats_by_hand():
    # alpha = 0.5 and 0.25 (exact in float32): w_1 = 0.5 * 1, T = 0.5, w_2 = 0.25 * 0.5 = 0.125
    ref = R.contribution_reference(1, 1, *ray([0.5, 0.25]))
    assert ref["max_w"].tolist() == [0.5, 0.125] and ref["sum_w"].tolist() == [0.5, 0.125]
    assert ref["sum_q"].tolist() == [1 << 23, 1 << 21]
    assert ref["hits"].tolist() == [1, 1] and ref["dominant"].tolist() == [1, 0]
    assert float(ref["alpha_img"][0, 0]) == 0.625 and int(ref["best"][0, 0]) == 0
    assert ref["near"].tolist() == [True, True]  # (sigma = 0 is within 1e-6 of the `sigma < 0` decision)
    assert not bool(ref["tie_pixels"].any()) and not bool(ref["near_tie"].any())
    # the second weight is the larger: 0.25, then 0.5 * 0.75 = 0.375
    ref = R.contribution_reference(1, 1, *ray([0.25, 0.5]))
    assert ref["max_w"].tolist() == [0.25, 0.375] and ref["dominant"].tolist() == [0, 1]
    # the float32 run on the same decisions: these weights are exact in float32 as well
    ref32 = R.contribution_reference(1, 1, *ray([0.25, 0.5]), dtype=torch.float32, decisions=ref["decisions"])
    assert R.e32_of(ref, ref32) == 0.0


def test_skip_stop_tie_and_clamp_on_hand_built_rays():
    # below 1/255: skipped, no statistics, and the entry behind it sees T = 1
    ref = R.contribution_reference(1, 1, *ray([0.003, 0.5]))
    assert ref["hits"].tolist() == [0, 1] and ref["max_w"].tolist() == [0.0, 0.5] and ref["dominant"].tolist() == [0, 1]
    # the clamp: alpha = 0.999, T = 0.001; the next opaque entry would make T 1e-6 <= 1e-4: the walk stops BEFORE it
    ref = R.contribution_reference(1, 1, *ray([1.0, 1.0, 0.5]))
    assert ref["hits"].tolist() == [1, 0, 0] and abs(float(ref["max_w"][0]) - 0.999) < 1e-7
    assert ref["sum_q"].tolist() == [math.floor(0.999 * 2 ** 24), 0, 0]  # (the float64 clamp)
    # equal weights to 1e-8: 0.2, then 0.25 * 0.8 -- a near-tie pixel; the front-most keeps it
    ref = R.contribution_reference(1, 1, *ray([0.2, 0.25]))
    assert bool(ref["tie_pixels"][0, 0]) and ref["near_tie"].tolist() == [True, True]
    assert ref["dominant"].tolist() == [1, 0]
    # three of opacity 0.5: weights 0.5, 0.25, 0.125
    ref = R.contribution_reference(1, 1, *ray([0.5, 0.5, 0.5]))
    assert ref["max_w"].tolist() == [0.5, 0.25, 0.125] and ref["dominant"].tolist() == [1, 0, 0]
    # nothing in the list
    ids, bins, xy, co, op = ray([0.5])
    ref = R.contribution_reference(1, 1, ids[:0], np.array([[0, 0]], np.int32), xy, co, op)
    assert ref["hits"].tolist() == [0] and int(ref["best"][0, 0]) == -1


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_every_gpu_case_meets_the_cap_on_the_near_share(name):
    """At most 2 % of the Gaussians with hits > 0 are near a decision or a tie, on the reference alone; and each scene
    is the scene its docstring describes."""
    sc = R.build_case(name)
    ids, bins = R.oracle_lists(sc)
    H, W = sc["H"], sc["W"]
    ref = R.contribution_reference(H, W, ids, bins, sc["xys"], sc["conics"], sc["opacities"])
    lengths = (np.asarray(bins)[:, 1] - np.asarray(bins)[:, 0]).tolist()
    share = R.near_share(ref)
    print(f"{name}: seed {R.CASES[name][1]}, lists {lengths}, Gaussians with hits {int((ref['hits'] > 0).sum())}, near "
          f"share {share:.4f}, near-tie pixels {int(ref['tie_pixels'].sum())}")
    assert share <= 0.02
    assert int(ref["dominant"].sum()) == int((ref["best"] >= 0).sum())
    assert bool((ref["hits"] >= ref["dominant"]).all()) and bool(((ref["hits"] > 0) == (ref["max_w"] > 0)).all())
    if name == "edges":
        assert (H, W) == (24, 40) and len(lengths) == 6 and min(lengths) > 0
    if name == "deep":
        assert lengths == [600]
        last = torch.stack([torch.where(d.any(dim=1), d.shape[1] - 1 - d.flip(1).to(torch.int8).argmax(dim=1), -1)
                            for d in [ref["decisions"][0]]])[0].reshape(16, 16)
        final_T = 1.0 - ref["alpha_img"]
        stopped = final_T < 2e-4  # (the stop rule fired: T (1 - alpha) <= 1e-4 with alpha <= 0.05)
        print(f"deep: {int(stopped.sum())} pixels stopped, last contributing entry there {int(last[stopped].min())} .. "
              f"{int(last[stopped].max())}; elsewhere up to {int(last[~stopped].max())}")
        assert bool(stopped[7:9, 7:9].all()) and 256 <= int(last[8, 8]) < 512  # inside the second batch
        assert not bool(stopped[0, 0]) and int(last[~stopped].max()) >= 512    # the third batch is walked and counts
    if name == "hidden":
        rows = R.hidden_rows()
        for k in ("stopper", "hidden", "faint"):
            for s in R.STATS:
                assert bool((ref[s][rows[k]] == 0).all()), (k, s)
        for k in ("front", "wall"):
            assert bool((ref["max_w"][rows[k]] >= 0.05).all()), k  # far from the pruning threshold 0.01
        assert not bool(ref["near"].any())


def _stats(max_weight, weight_sum=None, dominant=None):
    n = len(max_weight)
    return SimpleNamespace(max_weight=torch.tensor(max_weight, dtype=torch.float32),
                           weight_sum=torch.tensor(weight_sum if weight_sum is not None else [0.0] * n, dtype=torch.float64),
                           hits=torch.zeros(n, dtype=torch.int64),
                           dominant=torch.tensor(dominant if dominant is not None else [0] * n, dtype=torch.int64))


def test_prune_mask_rules_on_cpu_tensors():
    from gs_fused import prune_mask

    st = _stats([0.5, 0.009, 0.01, 0.0, 0.2], weight_sum=[4.0, 1.0, 2.0, 0.0, 3.0], dominant=[3, 0, 1, 0, 0])
    assert prune_mask(st, "max_weight").tolist() == [True, False, True, False, True]  # default 0.01: `<` removes
    assert prune_mask(st, "max_weight", threshold=0.1).tolist() == [True, False, False, False, True]
    assert prune_mask(st, "dominant").tolist() == [True, False, True, False, False]    # default 1
    assert prune_mask(st, "dominant", threshold=2).tolist() == [True, False, False, False, False]
    # weight_sum: volumes 1, 1, 1, 1, 1e-10 -> q90 = 1, v = 1 except the last: 3 * (1e-10)^0.1 = 0.3
    scales = torch.ones(5, 3)
    scales[4] = torch.tensor([1e-4, 1e-3, 1e-3])
    assert prune_mask(st, "weight_sum", threshold=0.5, scales=scales).tolist() == [True, True, True, False, False]
    assert prune_mask(st, "weight_sum", threshold=0.25, scales=scales).tolist() == [True, True, True, False, True]
    assert prune_mask(st, "weight_sum", threshold=0.5, scales=scales, power=0.0).tolist() == [True, True, True, False, True]
    # a volume above the 90 % quantile is clamped to v = 1
    big = torch.ones(20, 3)
    big[19] = 100.0
    st20 = _stats([0.0] * 20, weight_sum=[1.0] * 20)
    assert bool(prune_mask(st20, "weight_sum", threshold=1.0, scales=big).all())
    with pytest.raises(ValueError, match="prune_mask.*weight_sum.*scales"):
        prune_mask(st, "weight_sum", threshold=0.5)
    with pytest.raises(ValueError, match="prune_mask.*threshold.*keep"):
        prune_mask(st, "max_weight", threshold=0.1, keep=0.5)
    with pytest.raises(ValueError, match="prune_mask.*no default threshold"):
        prune_mask(st, "weight_sum", scales=scales)
    with pytest.raises(ValueError, match="prune_mask.*unknown rule"):
        prune_mask(st, "bogus")
    with pytest.raises(ValueError, match="prune_mask.*keep"):
        prune_mask(st, "max_weight", keep=0.0)


def test_prune_mask_keep_counts_and_ties():
    from gs_fused import prune_mask

    st = _stats([0.3, 0.1, 0.3, 0.1, 0.1, 0.05, 0.3])
    for keep in (1.0, 0.9, 0.5, 0.43, 0.3, 0.1, 0.01):
        mask = prune_mask(st, "max_weight", keep=keep)
        assert int(mask.sum()) == math.ceil(keep * 7), keep
    # ceil(0.3 * 7) = 3: the three of 0.3; ceil(0.5 * 7) = 4: and the FIRST of the three 0.1
    assert prune_mask(st, "max_weight", keep=0.3).tolist() == [True, False, True, False, False, False, True]
    assert prune_mask(st, "max_weight", keep=0.5).tolist() == [True, True, True, False, False, False, True]
    assert prune_mask(st, "max_weight", keep=0.7).tolist() == [True, True, True, True, False, False, True]
    # ceil(0.1 * 7) = 1: of equal scores the lower index
    assert prune_mask(st, "max_weight", keep=0.1).tolist() == [True] + [False] * 6
    assert prune_mask(_stats([0.0] * 4), "dominant", keep=0.5).tolist() == [True, True, False, False]


def test_prune_gaussians_keeps_rows_bit_for_bit():
    from gs_fused import prune_gaussians
    from gs_fused.refine import PARAM_NAMES

    g = torch.Generator().manual_seed(0)
    n = 11
    shapes = {"means": (n, 3), "scales": (n, 3), "quats": (n, 4), "features_dc": (n, 3), "features_rest": (n, 15, 3),
              "opacities": (n, 1)}
    params = {k: torch.randn(shapes[k], generator=g) for k in PARAM_NAMES}
    moments = {k: (torch.randn(shapes[k], generator=g), torch.rand(shapes[k], generator=g)) for k in PARAM_NAMES}
    del moments["quats"]  # (a parameter without Adam state yet)
    keep = torch.tensor([1, 0, 1, 1, 0, 0, 1, 0, 0, 0, 1], dtype=torch.bool)
    new, new_m = prune_gaussians(params, moments, keep)
    assert sorted(new) == sorted(PARAM_NAMES) and sorted(new_m) == sorted(moments)
    for k in PARAM_NAMES:
        assert new[k].shape == (5,) + shapes[k][1:] and new[k].is_contiguous()
        assert torch.equal(new[k], params[k][keep])
        if k in moments:
            for a, b in zip(new_m[k], moments[k]):
                assert torch.equal(a, b[keep]) and a.data_ptr() != b.data_ptr()
    new, new_m = prune_gaussians(params, None, keep)
    assert new_m == {} and torch.equal(new["means"], params["means"][keep])
    with pytest.raises(ValueError, match="prune_gaussians.*keep"):
        prune_gaussians(params, moments, keep[:5])


def test_accumulate_refuses_by_name():
    from gs_fused import ContributionStats, view_contributions

    n = 4
    args = (torch.zeros(n, 2), torch.ones(n), torch.ones(n, dtype=torch.int32), torch.ones(n, 3),
            torch.ones(n, dtype=torch.int32), torch.full((n, 1), 0.5), 16, 16)
    st = ContributionStats(n, "cpu")
    assert st.views == 0 and st.max_weight.dtype == torch.float32 and st.weight_sum.dtype == torch.float64
    assert st.hits.dtype == torch.int64 and st.dominant.dtype == torch.int64
    assert all(t.shape == (n,) and not bool(t.any()) for t in (st.max_weight, st.weight_sum, st.hits, st.dominant))
    with pytest.raises(ValueError, match="ContributionStats.accumulate.*CPU"):
        st.accumulate(*args)
    with pytest.raises(ValueError, match="ContributionStats.accumulate.*block_width"):
        st.accumulate(*args, block_width=8)
    with pytest.raises(ValueError, match="ContributionStats.accumulate.*CPU"):
        view_contributions(*args)
    assert st.views == 0


def test_check_prune_refusals_and_the_default_config():
    import harness.train as HT

    cfg = HT.TrainConfig()
    assert cfg.prune_at == () and cfg.prune_rule == "max_weight" and cfg.prune_threshold is None
    assert cfg.prune_keep is None
    cuda, cpu = torch.device("cuda"), torch.device("cpu")
    HT._check_prune(cfg, cpu, 2)  # off: nothing to refuse
    HT._check_prune(HT.TrainConfig(prune_at=(10,)), cuda, 1)
    HT._check_prune(HT.TrainConfig(prune_at=(10,), fused_render=True, use_graph=True, prune_keep=0.5), cuda, 1)
    for match, kw, dev, world in (
            ("prune_at.*world size", dict(), cuda, 2),
            ("prune_at.*mcmc", dict(strategy="mcmc"), cuda, 1),
            ("prune_at.*sharded_adam", dict(sharded_adam=True), cuda, 1),
            ("prune_at.*CUDA", dict(), cpu, 1),
            ("prune_at.*prune_keep.*prune_threshold", dict(prune_keep=0.5, prune_threshold=0.01), cuda, 1),
            ("prune_at.*prune_rule", dict(prune_rule="bogus"), cuda, 1),
            ("prune_at.*no default threshold", dict(prune_rule="weight_sum"), cuda, 1),
            ("prune_at.*prune_keep", dict(prune_keep=1.5), cuda, 1)):
        with pytest.raises(ValueError, match=match):
            HT._check_prune(HT.TrainConfig(prune_at=(10,), **kw), dev, world)
