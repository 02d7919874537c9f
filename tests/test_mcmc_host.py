"""CPU: the restatement of the MCMC densification kernels (tests/mcmc_reference.py) against written-out answers and
50-digit `decimal`, the host arithmetic of gs_fused.mcmc, and what the trainer refuses."""
import decimal
import math

import numpy as np
import pytest

import mcmc_reference as MR

# computed against 80-digit decimal: (o, n, o', o / D)
TABLE = ((0.8, 2, 0.5527864045000421, 0.8993814692265614),
         (0.8, 3, 0.4151964523574268, 0.8684109968198377),
         (0.8, 8, 0.1822345660420575, 0.8315444240387823),
         (0.8, 51, 0.03106486175379377, 0.8136777337313845))


def _decimal_relocation(o: float, n: int):
    D = decimal.Decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        od = D(o)  # the binary value, exactly
        o_new = 1 - ((1 - od).ln() / n).exp()
        total = D(0)
        for i in range(1, n + 1):
            for k in range(i):
                total += math.comb(i - 1, k) * (-1) ** k * o_new ** (k + 1) / D(k + 1).sqrt()
        return o_new, od / total


def test_relocation_check_values():
    for o, n, want_o, want_r in TABLE:
        got_o, got_r = MR.relocation_values(o, n)
        assert abs(got_o - want_o) <= 1e-11 * want_o, (o, n, got_o)
        assert abs(got_r - want_r) <= 1e-11 * want_r, (o, n, got_r)


@pytest.mark.parametrize("n", (1, 2, 3, 5, 8, 20, 51))
def test_relocation_against_decimal(n):
    for o in (0.005, 0.05, 0.2, 0.5, 0.8, 0.999, 1 - 1e-6):
        got_o, got_r = MR.relocation_values(o, n)
        want_o, want_r = _decimal_relocation(o, n)
        assert abs(decimal.Decimal(got_o) - want_o) <= decimal.Decimal(1e-11) * want_o, (o, n)
        assert abs(decimal.Decimal(got_r) - want_r) <= decimal.Decimal(1e-11) * want_r, (o, n)


def test_ratio_one_is_the_identity_and_ratios_clamp():
    o = np.array([0.005, 0.3, 0.999], np.float32)
    s = np.array([[0.1, 0.2, 0.3], [1e-3, 1.0, 5.0], [0.02, 0.02, 0.02]], np.float32)
    out_o, out_s = MR.relocation(o, s, [1, 1, 0])
    assert np.array_equal(out_o.astype(np.float32), o) and np.array_equal(out_s.astype(np.float32), s)
    for v in (0.2, 0.8):  # o' = o and D = o to rounding
        o_new, ratio = MR.relocation_values(v, 1)
        assert abs(o_new - v) <= 1e-15 and abs(ratio - 1) <= 1e-15
    assert MR.relocation_values(0.8, 60) == MR.relocation_values(0.8, 51)


def test_branch_and_growth_arithmetic():
    from gs_fused import MCMCConfig, mcmc_branch, mcmc_num_new

    cfg = MCMCConfig()
    assert (cfg.cap_max, cfg.noise_lr, cfg.refine_start_iter, cfg.refine_stop_iter, cfg.refine_every, cfg.min_opacity,
            cfg.opacity_reg, cfg.scale_reg, cfg.grow_factor) == (1_000_000, 5e5, 500, 25_000, 100, 0.005, 0.01, 0.01, 1.05)
    assert not mcmc_branch(cfg, 500) and mcmc_branch(cfg, 600) and not mcmc_branch(cfg, 650)
    assert mcmc_branch(cfg, 24_900) and not mcmc_branch(cfg, 25_000) and not mcmc_branch(cfg, 0)
    small = MCMCConfig(cap_max=3000)
    for n, want in ((3000, 0), (2999, 1), (3500, 0), (1, 0), (19, 0), (20, 1), (2000, 100), (2900, 100)):
        assert mcmc_num_new(small, n) == want == MR.num_new(3000, 1.05, n), n
    # 2000 -> 3000 at 5 % per refinement takes nine of them
    n, k = 2000, 0
    while n < 3000:
        n, k = n + mcmc_num_new(small, n), k + 1
    assert (n, k) == (3000, 9)


def test_sampler_frequencies_follow_the_weights():
    w = [5_000_000, 1, 16_777_215, 250_000, 8_000_000, 123_456, 3_000_000, 12_000_000]
    prefix = list(np.cumsum(np.array(w, dtype=object)))
    total, draws = int(prefix[-1]), 200_000
    src = np.array(MR.sample(prefix, MR.draw_targets(draws, MR.ADD, 700, 12345, total)))
    assert src.min() >= 0 and src.max() < len(w)
    for i, wi in enumerate(w):
        p = wi / total
        got = int((src == i).sum())
        assert abs(got - draws * p) <= 4.0 * math.sqrt(draws * p * (1 - p)) + 1e-9, (i, got, draws * p)


def test_zero_weight_rows_are_never_drawn():
    opac = np.array([0.001, 0.5, 0.0, 0.004, 0.9, 0.005, 0.2, 0.0049999], np.float32)
    pl = MR.plan(opac, 0.005, MR.RELOCATE, 0, 3, 99)
    w, dead = MR.weights(opac, 0.005, MR.RELOCATE)
    assert [bool(d) for d in dead] == [True, False, True, True, False, True, False, True]
    assert [x == 0 for x in w] == [bool(d) for d in dead]
    assert pl["dead_index"] == [0, 2, 3, 5, 7] and set(pl["draw_source"]) <= {1, 4, 6}
    many = MR.sample(pl["prefix"], MR.draw_targets(50_000, MR.RELOCATE, 3, 99, pl["total"]))
    assert set(many) == {1, 4, 6}
    # targets at the edges of the table: 0 and total - 1
    assert MR.sample(pl["prefix"], [0, pl["total"] - 1]) == [1, 6]
    # add phase: every row with a non-zero opacity has weight, dead or not
    w_add, _ = MR.weights(opac, 0.005, MR.ADD)
    assert [x > 0 for x in w_add] == [True, True, False, True, True, True, True, True]
    # nothing alive: the phase does nothing
    none = MR.plan(np.full(5, 0.001, np.float32), 0.005, MR.RELOCATE, 0, 3, 99)
    assert none["total"] == 0 and none["counts"] == [0] * 5 and none["row_source"] == [-1] * 5


def test_train_config_refusals():
    import torch

    from gs_fused import RefineConfig
    from harness.train import TrainConfig, _check_config, _check_mcmc

    _check_config(TrainConfig(strategy="mcmc"))
    _check_config(TrainConfig(strategy="mcmc", use_graph=True))
    with pytest.raises(ValueError, match="strategy"):
        _check_config(TrainConfig(strategy="gradient"))
    with pytest.raises(ValueError, match="refine"):
        _check_config(TrainConfig(strategy="mcmc", refine=RefineConfig()))
    with pytest.raises(ValueError, match="sharded_adam"):
        _check_config(TrainConfig(strategy="mcmc", sharded_adam=True))
    with pytest.raises(ValueError, match="world size"):
        _check_mcmc(TrainConfig(strategy="mcmc"), torch.device("cuda"), 2)
    with pytest.raises(ValueError, match="CUDA"):
        _check_mcmc(TrainConfig(strategy="mcmc"), torch.device("cpu"), 1)
    _check_mcmc(TrainConfig(), torch.device("cpu"), 4)  # the default strategy is not concerned
    assert TrainConfig().strategy == "default" and TrainConfig().mcmc is None


def test_cpu_tensors_raise():
    import torch

    from gs_fused import MCMCConfig, mcmc_inject_noise_, mcmc_refine, mcmc_regularizer, relocation

    n = 4
    p = {"means": torch.zeros(n, 3), "scales": torch.zeros(n, 3), "quats": torch.ones(n, 4),
         "features_dc": torch.zeros(n, 3), "features_rest": torch.zeros(n, 15, 3), "opacities": torch.zeros(n, 1)}
    with pytest.raises(RuntimeError, match="CUDA"):
        mcmc_refine(p, None, MCMCConfig(), 600, 1)
    with pytest.raises(RuntimeError, match="CUDA"):
        mcmc_inject_noise_(p["means"], p["scales"], p["quats"], p["opacities"], 1.0, 1, 1)
    with pytest.raises(RuntimeError, match="CUDA"):
        mcmc_regularizer(p["opacities"], p["scales"])
    with pytest.raises(RuntimeError, match="CUDA"):
        relocation(torch.full((n,), 0.5), torch.ones(n, 3), torch.ones(n, dtype=torch.int32))
