"""CPU: the host side of the per-view bilateral grids (gs_fused/bilagrid.py) -- argument checks,
the float64 restatement the GPU tests are held to (tests/_bilagrid_ref.py) against autograd's own finite differences
and against an explicit loop, the gsplat layout round trip, the learning-rate schedule and the trainer's refusals."""
import math

import numpy as np
import pytest
import torch

import _bilagrid_ref as B
from gs_fused import BilateralGrids, bilagrid_slice, bilagrid_tv_loss
from gs_fused.bilagrid import check_grid_shape, identity_grids, lr_schedule, strips, workspace_doubles


def test_slice_argument_checks_name_the_argument():
    grids, rgb = identity_grids(3, 4, 3, 2), torch.zeros(5, 7, 3)
    for view in (-1, 3, 10):
        with pytest.raises(ValueError, match="view"):
            bilagrid_slice(grids, rgb, view)
    with pytest.raises(ValueError, match="view"):
        bilagrid_slice(grids, rgb, 1.0)
    for bad in (torch.zeros(5, 7), torch.zeros(5, 7, 4), torch.zeros(3, 5, 7), torch.zeros(1, 5, 7, 3), torch.zeros(0, 7, 3)):
        with pytest.raises(ValueError, match="rgb"):
            bilagrid_slice(grids, bad, 0)
    with pytest.raises(ValueError, match="grids"):
        bilagrid_slice(torch.zeros(3, 2, 3, 4, 11), rgb, 0)
    with pytest.raises(ValueError, match="grids"):
        bilagrid_slice(torch.zeros(2, 3, 4, 12), rgb, 0)


@pytest.mark.parametrize("shape,name", [((1, 4, 4), "grid_w"), ((65, 4, 4), "grid_w"), ((4, 1, 4), "grid_h"),
                                        ((4, 65, 4), "grid_h"), ((4, 4, 1), "grid_l"), ((4, 4, 17), "grid_l"),
                                        ((4, 4, 0), "grid_l"), ((4.0, 4, 4), "grid_w")])
def test_grid_dimensions_outside_their_range_raise(shape, name):
    gw, gh, gl = shape
    with pytest.raises(ValueError, match=name):
        check_grid_shape(gw, gh, gl)
    with pytest.raises(ValueError, match=name):
        BilateralGrids(2, gw, gh, gl)
    if all(isinstance(s, int) and s >= 1 for s in shape):
        with pytest.raises(ValueError, match=name):  # (the ops check the tensor's own shape: [V,L,Gh,Gw,12])
            bilagrid_tv_loss(torch.zeros(2, gl, gh, gw, 12))
        with pytest.raises(ValueError, match=name):
            bilagrid_slice(torch.zeros(2, gl, gh, gw, 12), torch.zeros(4, 4, 3), 0)
    for ok in ((2, 2, 2), (64, 64, 16)):
        check_grid_shape(*ok)
    with pytest.raises(ValueError, match="num_views"):
        BilateralGrids(0)


def test_cpu_tensors_and_wrong_dtypes_raise_runtime_errors():
    grids, rgb = identity_grids(3, 4, 3, 2), torch.zeros(5, 7, 3)
    with pytest.raises(RuntimeError, match="CUDA"):
        bilagrid_slice(grids, rgb, 0)
    with pytest.raises(RuntimeError, match="CUDA"):
        bilagrid_tv_loss(grids)
    with pytest.raises(RuntimeError, match="tensor"):
        bilagrid_slice(grids, [[0.0, 0.0, 0.0]], 0)
    with pytest.raises(RuntimeError, match="tensor"):
        bilagrid_tv_loss(None)
    # (dtype is checked after the device: what a GPU run reports is asserted in tests/test_gpu_bilagrid.py)


def test_workspace_size_follows_the_header_macro():
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "gsraster.h")).read()
    assert re.search(r"#define GSR_BILAGRID_TV_WORKSPACE_DOUBLES 3072\b", src)
    assert "((gw) * (gh) >= 2048 ? 1 : ((gw) * (gh) <= 32 ? 64 : 2048 / ((gw) * (gh))))" in src
    assert [strips(*s) for s in ((2, 2), (3, 2), (4, 8), (3, 11), (16, 16), (32, 63), (32, 64), (64, 64))] == \
        [64, 64, 64, 62, 8, 1, 1, 1]
    assert workspace_doubles(16, 16, 8) == 8 * 16 * 16 * 8 * 12
    assert workspace_doubles(64, 64, 16) == 64 * 64 * 16 * 12


def test_restatement_identity_grids_return_the_image():
    gen = torch.Generator().manual_seed(3)
    rgb = B.draw_rgb(9, 11, 8, gen).double()
    out = B.slice_ref(B.identity_grids(2, 16, 16, 8, torch.float64), rgb, 1)
    assert float((out - rgb).abs().max()) <= 4e-16


def test_restatement_passes_gradcheck():
    """5x7 image, (3, 2, 3)-vertex grid, float64: autograd's gradient of the restatement (the path through the guide
    and the border clamp included) against finite differences."""
    gen = torch.Generator().manual_seed(5)
    gw, gh, gl = 3, 2, 3
    grids = (B.identity_grids(2, gw, gh, gl, torch.float64) + 0.25 * torch.randn((2, gl, gh, gw, 12), generator=gen,
                                                                                 dtype=torch.float64)).requires_grad_(True)
    rgb = B.draw_rgb(5, 7, gl, gen).double().requires_grad_(True)
    g = B.guide64(rgb.detach())
    assert bool((g < 0).any()) and bool((g > 1).any()) and bool(((g > 0) & (g < 1)).any())
    assert torch.autograd.gradcheck(lambda a, x: B.slice_ref(a, x, 1), (grids, rgb), eps=1e-6, atol=1e-7, rtol=1e-5)
    # the guide's path is zero where the guide is clamped: there v_rgb = M[:, :3]^T v_out alone
    out = B.slice_ref(grids, rgb, 1)
    v = torch.randn(out.shape, generator=gen, dtype=torch.float64)
    (v_rgb,) = torch.autograd.grad(out, rgb, v)
    m = _matrices(grids.detach()[1], rgb.detach())
    direct = torch.einsum("hwkc,hwk->hwc", m[..., :3], v)
    clamped = (g < 0) | (g > 1)
    assert float((v_rgb - direct)[clamped].abs().max()) <= 1e-14
    assert float((v_rgb - direct)[~clamped].abs().max()) > 1e-3


def _matrices(grid, rgb):
    """The [H,W,3,4] maps by an explicit trilinear loop over the 8 corners (float64): a second statement of the rule."""
    L, Gh, Gw, _ = grid.shape
    H, W, _ = rgb.shape
    out = torch.zeros(H, W, 3, 4, dtype=torch.float64)
    for py in range(H):
        for px in range(W):
            ix, iy = (px + 0.5) / W * (Gw - 1), (py + 0.5) / H * (Gh - 1)
            g = 0.299 * float(rgb[py, px, 0]) + 0.587 * float(rgb[py, px, 1]) + 0.114 * float(rgb[py, px, 2])
            iz = min(max(g, 0.0), 1.0) * (L - 1)
            x0, y0, z0 = min(int(ix), Gw - 2), min(int(iy), Gh - 2), min(int(iz), L - 2)
            fx, fy, fz = ix - x0, iy - y0, iz - z0
            m = torch.zeros(12, dtype=torch.float64)
            for dz, wz in ((0, 1 - fz), (1, fz)):
                for dy, wy in ((0, 1 - fy), (1, fy)):
                    for dx, wx in ((0, 1 - fx), (1, fx)):
                        m += wz * wy * wx * grid[z0 + dz, y0 + dy, x0 + dx]
            out[py, px] = m.reshape(3, 4)
    return out


def test_restatement_equals_the_explicit_trilinear_loop():
    gen = torch.Generator().manual_seed(7)
    grids = torch.randn((3, 5, 2, 3, 12), generator=gen, dtype=torch.float64)
    rgb = B.draw_rgb(5, 7, 5, gen).double()
    m = _matrices(grids[2], rgb)
    want = torch.einsum("hwkc,hwc->hwk", m[..., :3], rgb) + m[..., 3]
    assert float((B.slice_ref(grids, rgb, 2) - want).abs().max()) <= 1e-13


def test_tv_restatement_equals_the_triple_loop():
    gen = torch.Generator().manual_seed(11)
    a = torch.randn((2, 2, 3, 4, 12), generator=gen, dtype=torch.float64)
    V, L, Gh, Gw, C = a.shape
    sums, counts = [0.0, 0.0, 0.0], [0, 0, 0]
    for v in range(V):
        for z in range(L):
            for y in range(Gh):
                for x in range(Gw):
                    for c in range(C):
                        here = float(a[v, z, y, x, c])
                        for axis, (ok, there) in enumerate(((z + 1 < L, (v, min(z + 1, L - 1), y, x, c)),
                                                            (y + 1 < Gh, (v, z, min(y + 1, Gh - 1), x, c)),
                                                            (x + 1 < Gw, (v, z, y, min(x + 1, Gw - 1), c)))):
                            if ok:
                                sums[axis] += (float(a[there]) - here) ** 2
                                counts[axis] += 1
    assert counts == [V * C * (L - 1) * Gh * Gw, V * C * L * (Gh - 1) * Gw, V * C * L * Gh * (Gw - 1)]
    want = sum(s / n for s, n in zip(sums, counts))
    assert abs(float(B.tv_ref(a)) - want) <= 1e-13 * want
    assert float(B.tv_ref(B.identity_grids(2, 4, 3, 2, torch.float64))) == 0.0


def test_gsplat_layout_round_trip_is_exact():
    gen = torch.Generator().manual_seed(13)
    m = BilateralGrids(3, 5, 4, 2)
    assert tuple(m.grids.shape) == (3, 2, 4, 5, 12) and m.shape == (5, 4, 2) and m.num_views == 3
    assert torch.equal(m.grids.detach(), B.identity_grids(3, 5, 4, 2))
    with torch.no_grad():
        m.grids.copy_(torch.randn(m.grids.shape, generator=gen))
    theirs = m.to_gsplat()
    assert tuple(theirs.shape) == (3, 12, 2, 4, 5) and theirs.is_contiguous()
    # channel c of vertex (z, y, x) sits at [v, c, z, y, x] there
    assert float(theirs[1, 7, 1, 3, 2]) == float(m.grids.detach()[1, 1, 3, 2, 7])
    other = BilateralGrids(3, 5, 4, 2).from_gsplat(theirs)
    assert torch.equal(other.grids.detach(), m.grids.detach())
    assert torch.equal(other.to_gsplat(), theirs)
    with pytest.raises(ValueError, match="grids"):
        other.from_gsplat(theirs[:2])
    with pytest.raises(ValueError, match="grids"):
        other.from_gsplat(m.grids.detach())  # (our own layout is not theirs)


def test_lr_schedule_hand_computed():
    lr0, n = 2e-3, 7000
    assert lr_schedule(0, lr0, n) == pytest.approx(2e-5, rel=1e-12)                       # 1 % of lr0
    assert lr_schedule(500, lr0, n) == pytest.approx(2e-3 * 0.505 * 0.01 ** (500 / 7000), rel=1e-12)
    assert lr_schedule(500, lr0, n) == pytest.approx(7.26883e-4, rel=1e-5)                # 1.01e-3 * 0.719686
    assert lr_schedule(1000, lr0, n) == pytest.approx(2e-3 * 0.01 ** (1 / 7), rel=1e-12)  # warm-up over
    assert lr_schedule(1000, lr0, n) == pytest.approx(1.035895e-3, rel=1e-5)
    assert lr_schedule(n, lr0, n) == pytest.approx(2e-5, rel=1e-12)                       # decayed to 1 %
    assert lr_schedule(3500, lr0, n) == pytest.approx(2e-4, rel=1e-12)                    # 0.01 ** 0.5
    short = 300                                                                          # max_steps inside the warm-up
    assert lr_schedule(short, lr0, short) == pytest.approx(2e-3 * (0.01 + 0.99 * 0.3) * 0.01, rel=1e-12)
    assert math.isfinite(lr_schedule(5, lr0, 0))


def test_trainer_refusals_name_the_option():
    from harness.train import TrainConfig, _check_bilateral_grid

    cpu, cuda = torch.device("cpu"), torch.device("cuda:0")
    _check_bilateral_grid(TrainConfig(), cpu, 1)  # off: nothing to refuse
    _check_bilateral_grid(TrainConfig(bilateral_grid=True), cuda, 1)
    _check_bilateral_grid(TrainConfig(bilateral_grid=True, model="co-gs"), cuda, 1)
    with pytest.raises(ValueError, match="use_graph"):
        _check_bilateral_grid(TrainConfig(bilateral_grid=True, use_graph=True), cuda, 1)
    with pytest.raises(ValueError, match="world size"):
        _check_bilateral_grid(TrainConfig(bilateral_grid=True), cuda, 2)
    with pytest.raises(ValueError, match="CUDA"):
        _check_bilateral_grid(TrainConfig(bilateral_grid=True), cpu, 1)
    with pytest.raises(ValueError, match="grid_l"):
        _check_bilateral_grid(TrainConfig(bilateral_grid=True, bilagrid_shape=(16, 16, 32)), cuda, 1)
    with pytest.raises(ValueError, match="bilagrid_shape"):
        _check_bilateral_grid(TrainConfig(bilateral_grid=True, bilagrid_shape=(16, 16)), cuda, 1)
    _check_bilateral_grid(TrainConfig(view_exposure=(0.1, 0.0), background_color="random"), cpu, 1)
    with pytest.raises(ValueError, match="view_exposure"):
        _check_bilateral_grid(TrainConfig(view_exposure=(0.1, 0.0), dataset="somewhere"), cpu, 1)
    with pytest.raises(ValueError, match="view_exposure"):
        _check_bilateral_grid(TrainConfig(view_exposure=(-0.1, 0.0)), cpu, 1)
    cfg = TrainConfig()
    assert (cfg.bilateral_grid, tuple(cfg.bilagrid_shape), cfg.bilagrid_lr, cfg.bilagrid_tv_weight,
            tuple(cfg.view_exposure)) == (False, (16, 16, 8), 2e-3, 10.0, (0.0, 0.0))


@pytest.fixture()
def standins(monkeypatch):
    """The CPU stand-ins of the native ops, as every CPU run of the trainer uses them (tests/test_cogs_host.py)."""
    import cpu_standins as SI
    import harness.pipeline as HP
    import harness.train as HT
    from oracle import oracle as O

    O.set_threads(4)
    monkeypatch.setattr(HP, "project_gaussians", SI.project_gaussians)
    monkeypatch.setattr(HP, "spherical_harmonics", SI.spherical_harmonics)
    monkeypatch.setattr(HP, "rasterize_gaussians", SI.rasterize_gaussians)
    return HT


@pytest.mark.parametrize("background", ["fixed", "random"])
def test_trainer_fits_the_disturbed_targets_and_evaluates_on_the_true_ones(standins, background):
    HT = standins
    kw = dict(num_gaussians=300, width=48, height=32, num_views=3, iters=6, sh_degree=1, sh_degree_interval=3,
              eval_views=3, scene_scale=(0.03, 0.15), log_every=1, background_color=background)
    cpu = torch.device("cpu")
    plain = HT.train(HT.TrainConfig(**kw), cpu)
    bent = HT.train(HT.TrainConfig(view_exposure=(0.15, 0.03), **kw), cpu)
    assert "view_exposure" not in plain and "bilateral_grid" not in plain and "bilateral_grid" not in bent
    assert np.array(bent["view_exposure"]["gain"]).shape == (3, 3)
    assert bent["psnr_start"] == plain["psnr_start"]       # the same model against the same true images
    assert bent["losses"][0] != plain["losses"][0]         # ... but the first step fits another target
    data = HT.make_data(HT.TrainConfig(view_exposure=(0.15, 0.03), **kw), cpu)
    gain, bias = torch.tensor(data.exposure["gain"]), torch.tensor(data.exposure["bias"])
    for v in range(3):
        assert torch.allclose(data.gt_train[v], data.gt[v] * gain[v] + bias[v], atol=1e-7)
        if background == "random":
            assert torch.equal(data.gt_rgba_train[v][..., 3], data.gt_rgba[v][..., 3])
            assert torch.allclose(data.gt_rgba_train[v][..., :3], data.gt_rgba[v][..., :3] * gain[v] + bias[v], atol=1e-7)
    clean = HT.make_data(HT.TrainConfig(**kw), cpu)
    assert clean.gt_train is None and clean.gt_rgba_train is None and clean.exposure is None
    inputs = HT.StepInputs(HT.TrainConfig(view_exposure=(0.15, 0.03), **kw), data, cpu)
    _, target, _ = inputs(1, 1)
    if background == "fixed":
        assert torch.equal(target, data.gt_train[1])


def test_view_exposure_disturbs_every_view_once_and_reproducibly():
    from harness.train import disturb_exposure

    gt = [torch.full((4, 5, 3), 0.5), torch.full((4, 5, 3), 0.25)]
    a, rec = disturb_exposure(gt, 0.15, 0.03, 7)
    b, rec2 = disturb_exposure(gt, 0.15, 0.03, 7)
    assert rec == rec2 and all(torch.equal(x, y) for x, y in zip(a, b))
    gain, bias = torch.tensor(rec["gain"]), torch.tensor(rec["bias"])
    assert gain.shape == (2, 3) and bias.shape == (2, 3) and bool((gain > 0).all())
    for v in range(2):
        assert torch.allclose(a[v], gt[v] * gain[v] + bias[v], rtol=0, atol=1e-7)
        assert a[v].is_contiguous() and a[v].dtype == torch.float32
    assert not torch.equal(a[0][0, 0] / 0.5, a[1][0, 0] / 0.25)  # per view
    assert len({float(x) for x in gain[0]}) == 3                 # per channel
    c, _ = disturb_exposure(gt, 0.0, 0.0, 7)
    assert all(torch.equal(x, y) for x, y in zip(c, gt))
