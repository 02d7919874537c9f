"""GPU: the trainer with the depth-normal consistency term (TrainConfig.normal_consistency):
twenty iterations of the size the trainer tests use, on both model kinds, with the term on from the first step.  The
losses are finite, the record carries the term, two runs agree bit for bit in deterministic mode, and a run with the
option off equals a run of a config that never mentions it."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# the size the trainer tests use (tests/test_gpu_pose_opt.py), twenty iterations
SMALL = dict(num_gaussians=20_000, width=320, height=180, num_views=8, iters=20, sh_degree=3, sh_degree_interval=100,
             log_every=1, depth_loss_start_iteration=5)
ON = dict(normal_consistency=True, normal_start_iteration=0)


@pytest.fixture(scope="module", params=["gaussian-splatting", "co-gs"])
def runs(request):
    from harness.train import TrainConfig, train
    from rasterizer.rasterize import is_deterministic, set_deterministic

    was = is_deterministic()
    set_deterministic(True)
    try:
        dev = torch.device("cuda", 0)
        kw = dict(SMALL, model=request.param)
        yield {"model": request.param,
               "on": train(TrainConfig(**ON, **kw), dev), "again": train(TrainConfig(**ON, **kw), dev),
               "off": train(TrainConfig(normal_consistency=False, normal_lambda=0.3, normal_start_iteration=0, **kw), dev),
               "plain": train(TrainConfig(**kw), dev)}
    finally:
        set_deterministic(was)


def test_the_term_joins_the_loss_and_the_record(runs):
    on, plain = runs["on"], runs["plain"]
    assert on["render"] == "separate ops" and len(on["losses"]) == SMALL["iters"]
    assert all(math.isfinite(v) for v in on["losses"]) and math.isfinite(on["param_checksum"])
    rec = on["normal_consistency"]
    print(f"{runs['model']}: term {rec['term_first']:.5f} -> {rec['term_last']:.5f}; loss {on['losses'][0]:.5f} -> "
          f"{on['losses'][-1]:.5f} (without: {plain['losses'][0]:.5f} -> {plain['losses'][-1]:.5f})")
    assert rec["lambda"] == 0.05 and rec["start_iteration"] == 0
    assert math.isfinite(rec["term_first"]) and math.isfinite(rec["term_last"])
    assert 0.0 < rec["term_first"] <= 2.0 and 0.0 < rec["term_last"] <= 2.0  # (a mean of 1 - alpha <N, n_d>)
    # step 0 has no term (`step > normal_start_iteration`: the same loss up to the other compositing kernel's
    # rounding); from step 1 it is part of the loss
    assert abs(on["losses"][0] - plain["losses"][0]) < 1e-5 * abs(plain["losses"][0])
    assert on["losses"][1] > plain["losses"][1]
    assert on["psnr_start"] == plain["psnr_start"]


def test_a_second_run_is_bit_equal(runs):
    on, again = runs["on"], runs["again"]
    assert again["losses"] == on["losses"]
    assert again["param_checksum"] == on["param_checksum"]
    assert again["normal_consistency"] == on["normal_consistency"]


def test_the_option_off_is_a_run_that_never_mentions_it(runs):
    off, plain = runs["off"], runs["plain"]
    assert "normal_consistency" not in off and "normal_consistency" not in plain
    assert off["losses"] == plain["losses"] and off["param_checksum"] == plain["param_checksum"]
    assert off["psnr_end"] == plain["psnr_end"]
    assert set(off) == set(plain)
