"""CPU: the pieces `harness.train.train` is a driver over, each on its own -- the per-step inputs, the densification
statistics, the choice of loss heads and the tile lists' capacity rounding.  No render runs here."""
import pytest
import torch

import harness.train as HT


def _data(h=8, w=12, views=2, masks=False, seed=0):
    """Hand-made ground truth (no hidden scene): RGBA images and, composited over the fixed background, RGB ones."""
    g = torch.Generator().manual_seed(seed)
    bg = torch.tensor(HT.S.BACKGROUND)
    rgba = [torch.rand(h, w, 4, generator=g) for _ in range(views)]
    gt = [HT.composite_with_background(im, bg) for im in rgba]
    m = HT.view_masks("box", h, w, [None] * views, "cpu") if masks else None
    return HT.TrainData(factors=[1, 2], cams_by_d={}, bg=bg, gt=gt, gt_rgba=rgba, gt_depth=None, masks=m)


VISITS = [(0, 2), (1, 2), (0, 2), (0, 1), (1, 1), (0, 1)]  # (view, downscale factor): every pair comes round again


def test_step_inputs_random_background_fused_and_per_step_targets_agree():
    data, cpu = _data(masks=True), torch.device("cpu")
    kw = dict(background_color="random", width=12, height=8, seed=5, mask="box")
    fused = HT.StepInputs(HT.TrainConfig(fused_target=True, **kw), data, cpu, rank=1)
    plain = HT.StepInputs(HT.TrainConfig(fused_target=False, **kw), data, cpu, rank=1)
    gen = torch.Generator().manual_seed(5 + 977 * 2)  # the trainer's seed for rank 1
    worst = 0.0
    for v, d in VISITS:
        (bg_f, t_f, m_f), (bg_p, t_p, m_p) = fused(v, d), plain(v, d)
        bg = torch.rand(3, generator=gen)
        assert torch.equal(bg_f, bg) and torch.equal(bg_p, bg)  # one background sequence for one seed
        want = HT.composite_with_background(HT.downscale_image(data.gt_rgba[v], d), bg)
        assert t_f.shape == t_p.shape == (8 // d, 12 // d, 3)
        assert torch.equal(t_p, want)
        worst = max(worst, float((t_f - want).abs().max()))
        assert torch.equal(m_f, HT.downscale_mask(data.masks[v], d)) and m_f.shape == (8 // d, 12 // d, 1)
    print(f"addcmul target against a * rgb + (1 - a) * bg: largest difference {worst:.3g}")  # seen: 5.96e-08
    assert worst <= 1e-6  # one fp32 fused multiply-add against a multiply and an add of values in [0, 1]


def test_step_inputs_cache_what_does_not_depend_on_the_step():
    data = _data(masks=True)
    cfg = HT.TrainConfig(background_color="random", width=12, height=8, mask="box")
    inputs = HT.StepInputs(cfg, data, torch.device("cpu"))
    first = {}
    for i, (v, d) in enumerate(VISITS):
        _, _, mask = inputs(v, d)
        planes = inputs.target_cache[(v, d)]
        if (v, d) in first:  # the second visit: the same storage
            assert planes is first[(v, d)][0] and mask is first[(v, d)][1]
            assert planes[0].data_ptr() == first[(v, d)][2]
        else:
            first[(v, d)] = (planes, mask, planes[0].data_ptr())
    assert set(inputs.target_cache) == set(inputs.mask_cache) == set(VISITS)


def test_step_inputs_static_background_for_graph_replay_and_fixed_background():
    data, cpu = _data(), torch.device("cpu")
    cfg = HT.TrainConfig(background_color="random", use_graph=True, seed=3)
    inputs = HT.StepInputs(cfg, data, cpu)
    gen = torch.Generator().manual_seed(3 + 977)
    for v, d in VISITS:
        bg, target, mask = inputs(v, d)
        want = torch.rand(3, generator=gen)
        assert bg is inputs.bg_static and torch.equal(bg, want)  # the one tensor, the step's value in it
        assert float((target - HT.composite_with_background(HT.downscale_image(data.gt_rgba[v], d), want))
                     .abs().max()) <= 1e-6
        assert mask is None
    fixed = HT.StepInputs(HT.TrainConfig(), data, cpu)
    assert fixed.bg_gen is None and fixed.bg_static is None
    bg, target, _ = fixed(1, 2)
    assert bg is data.bg and torch.equal(target, HT.downscale_image(data.gt[1], 2))


def _view(radii, grads):
    xys = torch.zeros(len(radii), 2, requires_grad=True)
    xys.grad = torch.tensor(grads, dtype=torch.float32)
    return {"radii": torch.tensor(radii, dtype=torch.int32), "xys": xys}


def test_densify_state_assigns_after_a_restart_and_accumulates_after_that():
    st = HT.DensifyState(5, torch.device("cpu"), 10)
    assert [t.shape[0] for t in st.as_tuple()] == [5, 5, 5] and st.first
    # Gaussians 1 and 3 are not visible; gradient norms 5, 0, 10, 1, 2; radii / max_dim with max_dim = 10
    st.update(_view([3, 0, 2, 0, 7], [[3, 4], [0, 0], [6, 8], [1, 0], [0, 2]]), 10, step=0)
    assert st.xys_grad_norm.tolist() == [5.0, 0.0, 10.0, 1.0, 2.0]  # the first view's norms as they are (:355)
    assert st.vis_counts.tolist() == [1, 1, 1, 1, 1] and st.vis_counts.dtype == torch.int32
    assert torch.allclose(st.max_2dsize, torch.tensor([0.3, 0.0, 0.2, 0.0, 0.7]), rtol=0, atol=1e-7)
    assert not st.first
    # second view: Gaussians 0 and 3 not visible; norms 1, 3, 5, 13, 10
    st.update(_view([0, 4, 1, 0, 9], [[1, 0], [0, 3], [3, 4], [5, 12], [8, 6]]), 10, step=1)
    assert st.xys_grad_norm.tolist() == [5.0, 3.0, 15.0, 1.0, 12.0]
    assert st.vis_counts.tolist() == [1, 2, 2, 1, 2]
    assert torch.allclose(st.max_2dsize, torch.tensor([0.3, 0.4, 0.2, 0.0, 0.9]), rtol=0, atol=1e-7)
    st.restart()
    st.update(_view([0, 0, 0, 0, 1], [[0, 0]] * 4 + [[0, 1]]), 20, step=2)  # assigns again
    assert st.xys_grad_norm.tolist() == [0.0, 0.0, 0.0, 0.0, 1.0] and st.vis_counts.tolist() == [1] * 5
    assert torch.allclose(st.max_2dsize, torch.tensor([0.0, 0.0, 0.0, 0.0, 0.05]), rtol=0, atol=1e-7)
    st.reset(7)
    assert [t.shape[0] for t in st.as_tuple()] == [7, 7, 7] and st.first and st.first_vis is None
    assert st.vis_counts.dtype == torch.int32


def test_densify_state_stops_updating_at_stop_split_at():
    st = HT.DensifyState(2, torch.device("cpu"), 10, densify_until=4)
    st.update(_view([1, 1], [[3, 4], [0, 1]]), 10, step=3)
    st.update(_view([1, 1], [[3, 4], [0, 1]]), 10, step=4)  # step >= stop_split_at: nothing (vanilla_gs.py:347)
    assert st.xys_grad_norm.tolist() == [5.0, 1.0] and st.vis_counts.tolist() == [1, 1]


@pytest.mark.parametrize("world,rank,densify_until,step", [(2, 1, 55, 0), (8, 7, 55, 54), (2, 1, 55, 55), (2, 0, 55, 0),
                                                           (1, 0, 55, 0), (2, 1, None, 0)])
def test_first_view_visibility_is_recorded_for_the_ranks_that_must_report_it(world, rank, densify_until, step):
    st = HT.DensifyState(3, torch.device("cpu"), 10, densify_until=densify_until, rank=rank, world=world)
    view = _view([2, 0, 1], [[1, 0]] * 3)
    st.update(view, 10, step)
    densify, stop_split_at = densify_until is not None, densify_until
    if world > 1 and rank > 0 and densify and step < stop_split_at:  # the condition of the loop this class came from
        assert st.first_vis.tolist() == [1, 0, 1] and st.first_vis.dtype == torch.int32
    else:
        assert st.first_vis is None
    st.first_vis = None
    st.update(_view([1, 1, 1], [[1, 0]] * 3), 10, step)  # not the first view after a restart: never recorded
    assert st.first_vis is None
    st.restart()
    assert st.first and st.first_vis is None


def _ssim_2d(a, b):
    """SSIM as the models' `self.ssim` computes it (pytorch_msssim defaults: 11x11 Gaussian window, sigma 1.5, no
    padding, K = 0.01 / 0.03, data range 1), written with ONE two-dimensional window."""
    x = torch.arange(11, dtype=torch.float32) - 5
    g = torch.exp(-x * x / (2 * 1.5 ** 2))
    g = g / g.sum()
    w = (g[:, None] * g[None, :])[None, None].repeat(3, 1, 1, 1)
    blur = lambda t: torch.nn.functional.conv2d(t.permute(2, 0, 1)[None], w, groups=3)
    mu_a, mu_b = blur(a), blur(b)
    va, vb, cov = blur(a * a) - mu_a ** 2, blur(b * b) - mu_b ** 2, blur(a * b) - mu_a * mu_b
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu_a * mu_b + c1) * (2 * cov + c2)) / ((mu_a ** 2 + mu_b ** 2 + c1) * (va + vb + c2))).mean()


def _images(seed=1, h=12, w=16):
    g = torch.Generator().manual_seed(seed)
    pred, gt = torch.rand(h, w, 3, generator=g), torch.rand(h, w, 3, generator=g)
    mask = (torch.rand(h, w, 1, generator=g) > 0.3).float()
    pred_depth, gt_depth = 4 * torch.rand(h, w, 1, generator=g), 4 * torch.rand(h, w, generator=g)
    gt_depth[gt_depth < 1.0] = 0.0  # no measurement
    return pred, gt, mask, pred_depth, gt_depth


@pytest.mark.parametrize("masked", [False, True])
def test_vanilla_heads_on_the_cpu_are_the_models_formula(masked):
    photo, depth, fused_clamp = HT.loss_heads(HT.TrainConfig(), torch.device("cpu"))
    assert depth is None and fused_clamp is False
    pred, gt, mask, _, _ = _images()
    got = photo(pred, gt, mask) if masked else photo(pred, gt)
    if masked:  # vanilla_gs.py:915-924
        gt, pred = gt * mask.repeat(1, 1, 3), pred * mask.repeat(1, 1, 3)
    want = (1 - 0.2) * torch.abs(gt - pred).mean() + 0.2 * (1 - _ssim_2d(gt, pred))  # :926-944
    print(f"vanilla head, masked={masked}: {float(got):.8f}, {abs(float(got) - float(want)):.3g} from the formula")
    # the L1 is the same ops; the separable window against the 2-D one rounds differently in fp32: a few ulp of values
    # near 1, on the SSIM map's mean, times lambda
    assert abs(float(got) - float(want)) <= 1e-6


@pytest.mark.parametrize("masked", [False, True])
def test_cogs_heads_on_the_cpu_are_the_models_formulas(masked):
    cfg = HT.TrainConfig(model="co-gs", ssim_lambda=0.25)
    photo, depth, fused_clamp = HT.loss_heads(cfg, torch.device("cpu"))
    assert fused_clamp is False
    pred, gt, mask, pred_depth, gt_depth = _images(seed=2)
    got = photo(pred, gt, mask if masked else None)
    got_depth = depth({"depth": pred_depth}, gt_depth, mask if masked else None)
    if masked:  # depth_gs.py:424-437
        gt, pred = gt * mask.repeat(1, 1, 3), pred * mask.repeat(1, 1, 3)
        gt_depth, pred_depth = gt_depth * mask[..., 0], pred_depth * mask
    want = (1 - 0.25) * torch.abs(gt - pred).mean()  # :445-448: the SSIM line is an expression statement
    nonzero = gt_depth > 0
    want_depth = torch.abs(gt_depth * nonzero - pred_depth.squeeze(-1) * nonzero).mean()  # :531-538
    assert abs(float(got) - float(want)) <= 1e-7 and abs(float(got_depth) - float(want_depth)) <= 1e-7  # the same ops
    assert float(want_depth) > 0.1 and float(want) > 0.1


def test_heads_look_their_loss_functions_up_when_they_are_called(monkeypatch):
    """The tests of the loop substitute `ssim`, `cogs_main_loss` and `cogs_depth_l1` in harness.train: a head that
    bound them when it was built would make those tests pass without testing anything."""
    pred, gt, mask, pred_depth, gt_depth = _images(seed=3)
    photo, _, _ = HT.loss_heads(HT.TrainConfig(), torch.device("cpu"))
    cogs_photo, cogs_depth, _ = HT.loss_heads(HT.TrainConfig(model="co-gs"), torch.device("cpu"))
    calls = []
    real_ssim = HT.ssim
    monkeypatch.setattr(HT, "ssim", lambda a, b: calls.append("ssim") or real_ssim(a, b))
    monkeypatch.setattr(HT, "cogs_main_loss", lambda p, t, lam: calls.append(("main", lam)) or (p - t).sum())
    monkeypatch.setattr(HT, "cogs_depth_l1", lambda p, t: calls.append("depth") or p.sum())
    photo(pred, gt)
    assert calls == ["ssim"]
    assert float(cogs_photo(pred, gt, mask)) == float((pred * mask - gt * mask).sum())
    assert float(cogs_depth({"depth": pred_depth}, gt_depth)) == float(pred_depth.sum())
    assert calls == ["ssim", ("main", 0.2), "depth"]


@pytest.mark.parametrize("need", [1, 2 ** 20 - 65536, 2 ** 20, 3_000_000])
def test_round_capacity_is_the_three_expressions_it_replaced(need):
    fits = ((int(1.5 * need) + 65536 + (1 << 20) - 1) >> 20) << 20      # the probe render, lists large enough
    grow_probe = ((int(1.5 * need) + (1 << 20)) >> 20) << 20            # the probe render, lists too small
    grow_graph = ((int(1.5 * int(need)) + (1 << 20)) >> 20) << 20       # a replayed graph whose view did not fit
    assert HT._round_capacity(need, fits=True) == fits
    assert HT._round_capacity(need, fits=False) == grow_probe == grow_graph
    assert fits % (1 << 20) == 0 and fits >= 1.5 * need + 65536 and grow_probe > 1.5 * need
