"""GPU: contribution-based pruning in the trainer (TrainConfig.prune_at) on the separate ops, the
one-node view and its HIP graph: 2 000 Gaussians, 96 x 64, 6 views, 60 iterations, pruned once after step 40 to 0.7."""
import json
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = dict(num_gaussians=2000, width=96, height=64, num_views=6, iters=60, sh_degree=1, sh_degree_interval=20,
             log_every=5, densify=False)
ROUTES = {"separate": dict(), "fused_render": dict(fused_render=True), "use_graph": dict(use_graph=True)}
# what differs from run to run whatever the options: times, and a peak that depends on what ran before in the process
TIMING = ("seconds", "iters_per_s", "views_per_s", "peak_memory_bytes")


def _train(**kw):
    from harness.train import TrainConfig, train

    return train(TrainConfig(**SMALL, **kw), torch.device("cuda", 0))


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_one_prune_to_a_fraction_and_training_goes_on(route):
    res = _train(prune_at=(40,), prune_keep=0.7, **ROUTES[route])
    assert res["render"] == {"separate": "separate ops", "fused_render": "one fused op",
                             "use_graph": "hip graph per view"}[route]
    n0 = res["num_gaussians_start"]
    want = math.ceil(0.7 * n0)
    print(f"{route}: {n0} -> {res['num_gaussians_end']} Gaussians, prune {res['prune']}, PSNR {res['psnr_start']:.2f} -> "
          f"{res['psnr_end']:.2f}, losses {res['losses']}")
    assert n0 == 2000 and res["num_gaussians_end"] == want
    assert len(res["prune"]) == 1
    rec = res["prune"][0]
    assert (rec["step"], rec["n_in"], rec["n_out"]) == (40, n0, want) and rec["ms"] > 0.0
    assert [tuple(h) for h in res["refinements"]] == [(40, want)]
    assert len(res["losses"]) == 12 and all(math.isfinite(v) for v in res["losses"])  # steps 0, 5, ..., 55
    assert math.isfinite(res["param_checksum"]) and math.isfinite(res["psnr_end"])


def test_a_threshold_prunes_by_the_rules_default_and_twice():
    res = _train(prune_at=(20, 40), prune_rule="dominant")
    a, b = res["prune"]
    print(f"dominant, default threshold: {a} then {b}")
    assert (a["step"], b["step"]) == (20, 40) and a["n_in"] == 2000 and b["n_in"] == a["n_out"]
    assert 0 < a["n_out"] < 2000 and b["n_out"] <= a["n_out"] and res["num_gaussians_end"] == b["n_out"]
    assert all(math.isfinite(v) for v in res["losses"])


def test_without_prune_at_the_record_is_what_it_was():
    from rasterizer import rasterize as R

    was = R.is_deterministic()
    R.set_deterministic(True)  # (fixed summation order: two runs are comparable bit for bit)
    try:
        plain = _train()
        named = _train(prune_at=(), prune_rule="dominant", prune_keep=0.5)
    finally:
        R.set_deterministic(was)
    assert "prune" not in plain and "prune" not in named
    strip = lambda r: {k: v for k, v in r.items() if k not in TIMING and not k.startswith("phase_")}  # noqa: E731
    assert json.dumps(strip(named), sort_keys=True, default=str) == json.dumps(strip(plain), sort_keys=True, default=str)
    assert plain["num_gaussians_end"] == 2000
