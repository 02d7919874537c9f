"""GPU: the trainer with per-view bilateral grids (TrainConfig.bilateral_grid) on a synthetic
run whose training targets carry a per-view exposure error (`view_exposure`): the grids absorb it (a lower training
loss on the disturbed targets, grids away from the identity), the run is reproducible bit for bit in deterministic
mode, a checkpoint carries the grids and their Adam state and a resumed run continues as the uninterrupted one did, and
the settings the grids cannot serve are refused.  The PSNR on the TRUE images is printed, not asserted: the grids leave
a global colour gauge free, and nobody has measured which way a few hundred steps fall."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# the size the trainer tests use (tests/test_gpu_pose_opt.py)
SMALL = dict(num_gaussians=20_000, width=320, height=180, num_views=8, iters=300, sh_degree=3, sh_degree_interval=100,
             view_exposure=(0.15, 0.03), log_every=1)
SAVE_AT = 200


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Deterministic mode; the run with grids (saving at step 200), the run without, same seeds."""
    from harness.train import TrainConfig, train
    from rasterizer.rasterize import is_deterministic, set_deterministic

    was = is_deterministic()
    set_deterministic(True)
    try:
        dev = torch.device("cuda", 0)
        ckpt = str(tmp_path_factory.mktemp("bilagrid_ckpt"))
        on = train(TrainConfig(bilateral_grid=True, checkpoint_dir=ckpt, save_every=SAVE_AT, **SMALL), dev)
        off = train(TrainConfig(**SMALL), dev)
        yield {"on": on, "off": off, "ckpt": ckpt, "dev": dev}
    finally:
        set_deterministic(was)


def _final_loss(res):
    """The mean training loss of the last pass over the views (one step each)."""
    return float(np.mean(res["losses"][-SMALL["num_views"]:]))


def test_the_grids_absorb_the_exposure_error(runs):
    on, off = runs["on"], runs["off"]
    assert on["render"] == "separate ops" and np.isfinite(on["param_checksum"])
    print(f"final training loss on the disturbed targets: grids {_final_loss(on):.5f}, none {_final_loss(off):.5f}; "
          f"PSNR on the true images: grids {on['psnr_start']:.2f} -> {on['psnr_end']:.2f} dB, "
          f"none {off['psnr_start']:.2f} -> {off['psnr_end']:.2f} dB")
    assert len(on["losses"]) == len(off["losses"]) == SMALL["iters"]
    assert _final_loss(on) < _final_loss(off)  # (the grids' own TV term is part of theirs)
    rec = on["bilateral_grid"]
    assert rec["shape"] == [16, 16, 8] and np.isfinite(rec["tv_end"]) and rec["tv_end"] > 0
    away = rec["max_abs_from_identity"]
    assert len(away) == SMALL["num_views"] and all(np.isfinite(a) and a > 1e-3 for a in away), away
    gain = np.array(on["view_exposure"]["gain"])
    assert gain.shape == (8, 3) and np.abs(np.log(gain)).max() > 0.05  # every view was disturbed
    assert "bilateral_grid" not in off and off["view_exposure"] == on["view_exposure"]
    assert on["psnr_start"] == off["psnr_start"]  # evaluation keeps the true images, and renders without grids


def test_a_second_run_is_bit_equal(runs):
    from harness.train import TrainConfig, train

    again = train(TrainConfig(bilateral_grid=True, **SMALL), runs["dev"])
    on = runs["on"]
    assert again["losses"] == on["losses"]
    assert again["param_checksum"] == on["param_checksum"]
    assert again["bilateral_grid"]["checksum"] == on["bilateral_grid"]["checksum"]
    assert again["bilateral_grid"]["max_abs_from_identity"] == on["bilateral_grid"]["max_abs_from_identity"]


def test_checkpoint_carries_the_grids_and_a_resumed_run_continues_equal(runs):
    from harness import checkpoint as CK
    from harness.train import TrainConfig, train

    on = runs["on"]
    path = CK.checkpoint_path(runs["ckpt"], SAVE_AT)
    saved = torch.load(path, map_location="cpu", weights_only=True)
    grids = saved["pipeline"]["_model.bilateral_grids.grids"]
    assert tuple(grids.shape) == (8, 8, 16, 16, 12) and grids.dtype == torch.float32
    st = saved["optimizers"]["bilateral_grid"]["state"][0]
    assert int(st["step"]) == SAVE_AT + 1 and bool(st["exp_avg"].any()) and bool(st["exp_avg_sq"].any())
    more = train(TrainConfig(bilateral_grid=True, resume_from=path, **SMALL), runs["dev"])
    assert more["start_step"] == SAVE_AT + 1 and more["iters"] == SMALL["iters"] - SAVE_AT - 1
    assert more["losses"] == on["losses"][SAVE_AT + 1:]
    assert more["param_checksum"] == on["param_checksum"]
    assert more["bilateral_grid"]["checksum"] == on["bilateral_grid"]["checksum"]


def test_the_one_node_view_takes_the_grids_too():
    from harness.train import TrainConfig, train

    kw = {**SMALL, "iters": 24, "log_every": 0}
    res = train(TrainConfig(bilateral_grid=True, fused_render=True, **kw), torch.device("cuda", 0))
    assert res["render"] == "one fused op" and np.isfinite(res["param_checksum"])
    assert all(a > 0 for a in res["bilateral_grid"]["max_abs_from_identity"])


def test_settings_the_grids_cannot_serve_are_refused():
    from harness.train import TrainConfig, train

    dev = torch.device("cuda", 0)
    kw = {**SMALL, "iters": 2}
    with pytest.raises(ValueError, match="use_graph"):
        train(TrainConfig(bilateral_grid=True, use_graph=True, **kw), dev)
    with pytest.raises(ValueError, match="world size"):
        train(TrainConfig(bilateral_grid=True, **kw), dev, rank=0, world=2)
    with pytest.raises(ValueError, match="CUDA"):
        train(TrainConfig(bilateral_grid=True, **kw), torch.device("cpu"))
    with pytest.raises(ValueError, match="grid_w"):
        train(TrainConfig(bilateral_grid=True, bilagrid_shape=(1, 16, 8), **kw), dev)
