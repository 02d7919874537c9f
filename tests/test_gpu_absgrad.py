"""GPU: the absgrad of the compositing backward (`raster_bwd_tile16_kernel<.., ABS = true>`) on every route that
`launch_tile16_backward` serves, against the float64 restatement of tests/absgrad_reference.py fed the forward's own
lists, final_Ts and final_idx; then the one-call view, its graph and the trainer.

The bound, everywhere a reference exists:  |hip - ref| <= 1e-3 max(ref_g, 1e-3 max ref) + U_g,  U_g the decision
slack of DESIGN.md section 2, which at most 5 % of a scene's Gaussians may carry (seeds checked on the CPU in
tests/test_absgrad_host.py)."""
import numpy as np
import pytest
import torch

import absgrad_reference as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def cu(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.requires_grad_(True) if grad else t


def npy(t):
    return t.detach().cpu().numpy()


@pytest.fixture(autouse=True)
def recipe_detection_stays_on():
    """The views of this file hand `rasterize_gaussians` opacities that rasterizer/ahead.py cannot trace to a leaf (the
    activation op's output): enough of them in a row switch its recipe detection off for the device, for the rest of
    the process.  Put back, as the tests that provoke it on purpose do (tests/test_gpu_api.py)."""
    yield
    from rasterizer import ahead

    st = ahead._spec.get(torch.device(DEV))
    if st is not None:
        st["recipes_off"], st["unknown_run"] = False, 0


@pytest.fixture(scope="module")
def scenes():
    return {"small": A.small_scene(0), "deep": A.deep_scene(0), "single": A.single_splat_scene()}


def run(sc, absgrad=True, rgbd=False, fresh_lists=True):
    """One forward + backward through the public op on a scene's projection outputs -> everything the checks need,
    with the lists, final_Ts and final_idx the kernels really used (the autograd node's saved tensors)."""
    from gs_fused import rasterize_gaussians_rgbd
    from rasterizer import rasterize as R
    from rasterizer import rasterize_gaussians

    if fresh_lists:
        R._bin_cache["key"] = None
    H, W = sc["H"], sc["W"]
    xys, conics, colors, opac = (cu(sc[k], True) for k in ("xys", "conics", "colors", "opacities"))
    depths, radii, tiles, bg = (cu(sc[k]) for k in ("depths", "radii", "num_tiles_hit", "background"))
    extra = None
    if rgbd:
        extra = cu(sc["depths"], True)
        img, alpha, ext = rasterize_gaussians_rgbd(xys, depths, radii, conics, tiles, colors, extra, opac, H, W,
                                                   background=bg, absgrad=absgrad)
        node = img.grad_fn
        ids, bins, Ts, idx = (node.saved_tensors[i] for i in (0, 1, 8, 9))
    else:
        img, alpha = rasterize_gaussians(xys, depths, radii, conics, tiles, colors, opac, H, W, 16, background=bg,
                                         return_alpha=True, absgrad=absgrad)
        node = img.grad_fn
        ids, bins, Ts, idx = (node.saved_tensors[i] for i in (0, 1, 7, 8))
    res = {"img": img.detach().clone(), "alpha": alpha.detach().clone(), "two": node.two, "det": node.det,
           "ids": npy(ids).reshape(-1), "bins": npy(bins).reshape(-1, 2), "Ts": npy(Ts), "idx": npy(idx),
           "t": (ids, bins, Ts, idx)}
    outs, cots = [img, alpha], [cu(sc["v_img"]), cu(sc["v_alpha"])]
    if rgbd:
        res["ext"] = ext.detach().clone()
        outs.append(ext)
        cots.append(cu(sc["v_extra"])[..., None])
    torch.autograd.backward(outs, cots)
    torch.cuda.synchronize()
    res["grads"] = tuple(t.grad.clone() for t in (xys, conics, colors, opac) + ((extra,) if rgbd else ()))
    res["absgrad"] = getattr(xys, "absgrad", None)
    res["inputs"] = (xys, conics, colors, opac, bg)
    return res


def reference(sc, res, rgbd=False):
    H, W = sc["H"], sc["W"]
    colors, v_out, bg = sc["colors"], sc["v_img"], sc["background"]
    if rgbd:  # the extra channel (the depths, over background 0) is one more colour of the same walk
        colors = np.concatenate([colors, sc["depths"][:, None]], axis=1)
        v_out = np.concatenate([v_out, sc["v_extra"][..., None]], axis=2)
        bg = np.concatenate([bg, [0.0]])
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    bins2, base2 = (None, 0) if res["two"] is None else (npy(res["two"][0]).reshape(-1, 2)[:tiles], int(res["two"][1]))
    return A.absgrad_reference(H, W, res["ids"], res["bins"][:tiles], sc["xys"], sc["conics"], colors, sc["opacities"],
                               bg, res["Ts"], res["idx"], v_out, sc["v_alpha"], bins2=bins2, idx_base2=base2)


def hold(got, ref, U, what):
    ok, worst = A.within_bound(npy(got) if isinstance(got, torch.Tensor) else got, ref, U)
    print(f"{what}: worst error / bound = {worst:.3e}, slack on {A.slack_fraction(U):.4f} of the Gaussians")
    assert A.slack_fraction(U) <= 0.05, what
    assert ok, f"{what}: error / bound = {worst:.3e}"


def check(sc, res, what, rgbd=False):
    v_xy, v_abs, U = reference(sc, res, rgbd)
    assert res["absgrad"] is not None and tuple(res["absgrad"].shape) == (sc["xys"].shape[0], 2)
    assert res["absgrad"].dtype == torch.float32
    hold(res["absgrad"], v_abs, U, what + " absgrad")
    hold(res["grads"][0], v_xy, U, what + " v_xy")  # (the reference itself, on the kernel's signed sums)
    return v_abs, U


@pytest.mark.parametrize("one_wave", [False, True])
def test_small_scene_lists_of_1_to_130_entries(scenes, tune, one_wave):
    """3 x 2 tiles with partial edge tiles; lists of 130, 101, 70, 23, 1, 1 entries.  As is, the two lists above the
    small-grid threshold (96) take four waves; with `small_grid_bwd` = 0 every list takes one wave."""
    tune(**({"two_round": "0", "small_grid_bwd": 0} if one_wave else {"two_round": "0"}))
    sc = scenes["small"]
    res = run(sc)
    assert (res["bins"][:6, 1] - res["bins"][:6, 0]).tolist() == A.SMALL_LIST_LENGTHS
    check(sc, res, "small" + (" one wave" if one_wave else ""))
    off = run(sc, absgrad=False)
    assert off["absgrad"] is None
    assert torch.equal(off["img"], res["img"]) and torch.equal(off["alpha"], res["alpha"])


@pytest.mark.parametrize("segments", [True, False])
def test_deep_scene_lists_beyond_1024_entries(scenes, tune, segments):
    """Four tiles of 1 500 entries: with depth segments (5 runs of 320 entries, the absgrad sums add over the runs)
    and as single walks.  Both are held to the reference."""
    tune(**({"two_round": "0", "depth_segments": 5, "depth_segments_min": 64} if segments
            else {"two_round": "0", "depth_segments": 1}))
    sc = scenes["deep"]
    res = run(sc)
    assert (res["bins"][:4, 1] - res["bins"][:4, 0]).min() > 1024
    check(sc, res, "deep" + (" segments" if segments else ""))
    off = run(sc, absgrad=False)
    assert torch.equal(off["img"], res["img"]) and torch.equal(off["alpha"], res["alpha"])


@pytest.mark.parametrize("name,segments", [("deep", True), ("small", False)])
def test_rgbd_pass(scenes, tune, name, segments):
    """The same scenes through `rasterize_gaussians_rgbd` (the fourth channel joins v_alpha, so it joins the absgrad)."""
    tune(**({"two_round": "0", "depth_segments": 5, "depth_segments_min": 64} if segments else {"two_round": "0"}))
    sc = scenes[name]
    res = run(sc, rgbd=True)
    check(sc, res, name + " rgbd", rgbd=True)
    off = run(sc, absgrad=False, rgbd=True)
    assert off["absgrad"] is None
    assert torch.equal(off["img"], res["img"]) and torch.equal(off["ext"], res["ext"])


@pytest.mark.parametrize("rgbd", [False, True])
def test_two_round_lists(scenes, tune, monkeypatch, rgbd):
    """Two-round lists forced as tests/test_gpu_api.py forces them (`two_round` = "1": every view behind the one that
    asks for the number of culled Gaussians builds a prefix list, composites, filters, builds the rest)."""
    import rasterizer.cuda as C_
    from rasterizer import rasterize as R

    monkeypatch.setattr(C_, "depth_segments", lambda entries, num_tiles: (1, 0))  # (two rounds resume ONE chain)
    sc = scenes["deep"]
    tune(two_round="0")
    run(sc, rgbd=rgbd)  # exact sizing: leaves the count hint
    tune(two_round="1")
    R._two_hint.clear()
    res = None
    for _ in range(4):
        res = run(sc, rgbd=rgbd)
        if res["two"] is not None:
            break
    assert res["two"] is not None, "no view took two rounds"
    check(sc, res, "two-round" + (" rgbd" if rgbd else ""), rgbd=rgbd)
    tune(two_round="0")


@pytest.mark.parametrize("name", ["small", "deep"])
def test_deterministic_mode(scenes, tune, name):
    """Slots 10 and 11 of the partial rows, summed in reduce_partials_kernel's fixed order: bit-identical over two
    calls; the atomic mode stays within the bound of it; and with the switch on, the image and all four gradients of
    the deterministic backward keep their bits."""
    from rasterizer import rasterize as R

    tune(two_round="0")
    sc = scenes[name]
    atomic = run(sc)
    R.set_deterministic(True)
    try:
        a, b = run(sc), run(sc)
        off = run(sc, absgrad=False)
    finally:
        R.set_deterministic(False)
    assert a["det"] is not None
    assert torch.equal(a["absgrad"], b["absgrad"])
    v_abs, U = check(sc, a, name + " deterministic")
    hold(atomic["absgrad"], npy(a["absgrad"]).astype(np.float64), U, name + " atomic against deterministic")
    assert torch.equal(off["img"], a["img"]) and torch.equal(off["alpha"], a["alpha"])
    for g_off, g_on in zip(off["grads"], a["grads"]):
        assert torch.equal(g_off, g_on)


def test_sign_coherent_single_splat(scenes, tune):
    """n = 1, wholly to one side of the image, b = 0, cotangents of one sign: abs_x == |v_xy_x| to the rounding of
    256 same-sign additions."""
    tune(two_round="0")
    sc = scenes["single"]
    res = run(sc)
    check(sc, res, "single splat")
    ax, vx = float(res["absgrad"][0, 0]), float(res["grads"][0][0, 0])
    print(f"single splat: abs_x {ax!r}, v_xy_x {vx!r}")
    assert ax > 1.0 and abs(ax - abs(vx)) <= 256 * 2.0 ** -24 * ax
    assert float(res["absgrad"][0, 1]) > 10 * abs(float(res["grads"][0][0, 1]))


def test_empty_view_and_culled_rows(scenes, tune):
    """A view with no intersections gives exact zeros; the rows of culled Gaussians (radius 0) are exactly 0."""
    tune(two_round="0")
    sc = dict(scenes["small"])
    n = sc["xys"].shape[0]
    culled = np.zeros(n, bool)
    culled[::7] = True
    sc["radii"] = np.where(culled, 0, sc["radii"]).astype(np.int32)
    sc["num_tiles_hit"] = np.where(culled, 0, sc["num_tiles_hit"]).astype(np.int32)
    res = run(sc)
    ab = npy(res["absgrad"])
    assert not ab[culled].any() and ab[~culled].any(axis=1).mean() > 0.9
    check(sc, res, "with culled rows")
    sc["radii"] = np.zeros(n, np.int32)
    sc["num_tiles_hit"] = np.zeros(n, np.int32)
    res = run(sc)
    assert tuple(res["absgrad"].shape) == (n, 2) and not res["absgrad"].any()
    # overwritten by each backward: the same tensor after a view that does draw
    xys = cu(scenes["small"]["xys"], True)
    for tiles_key, expect in (("small", True), (None, False)):
        from rasterizer import rasterize_gaussians

        s2 = scenes["small"] if tiles_key else sc
        img = rasterize_gaussians(xys, cu(s2["depths"]), cu(s2["radii"]), cu(s2["conics"]), cu(s2["num_tiles_hit"]),
                                  cu(s2["colors"]), cu(s2["opacities"]), s2["H"], s2["W"], 16, absgrad=True)
        img.sum().backward()
        assert bool(xys.absgrad.any()) is expect


def test_output_is_a_view_of_a_larger_allocation(scenes, tune):
    """Exactly [N,2] is written: the output as a slice of a sentinel-filled allocation, through the three bindings."""
    import rasterizer.cuda as C_

    tune(two_round="0")
    sc = scenes["small"]
    res = run(sc)
    v_abs, U = reference(sc, res)[1:]
    n = sc["xys"].shape[0]
    ids, bins, Ts, idx = res["t"]
    xys, conics, colors, opac, bg = (t.detach() for t in res["inputs"])
    v_img, v_alpha = cu(sc["v_img"]), cu(sc["v_alpha"])
    big = torch.full((n + 64, 2), -7.5, device=DEV)
    out = big[32:32 + n]
    C_.rasterize_backward(sc["H"], sc["W"], 16, ids, bins, xys, conics, colors, opac, bg, Ts, idx, v_img, v_alpha,
                          v_xy_abs=out)
    torch.cuda.synchronize()
    assert bool((big[:32] == -7.5).all()) and bool((big[32 + n:] == -7.5).all())
    hold(out, v_abs, U, "rasterize_backward(v_xy_abs=view)")
    # NULL behaves as the entry it extends
    plain = C_.rasterize_backward(sc["H"], sc["W"], 16, ids, bins, xys, conics, colors, opac, bg, Ts, idx, v_img, v_alpha)
    assert len(plain) == 4
    with pytest.raises(RuntimeError, match="v_xy_abs"):
        C_.rasterize_backward(sc["H"], sc["W"], 16, ids, bins, xys, conics, colors, opac, bg, Ts, idx, v_img, v_alpha,
                              v_xy_abs=big[:n, :1])


# ---- the one-call view and its graph ---------------------------------------------------------------------------------

def _model(n, K, seed):
    from harness.train import blob_scene

    raw = blob_scene(n, seed=seed, sh_degree={1: 0, 4: 1, 9: 2, 16: 3}[K])
    return {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in raw.items()}


def _camera(W, H, i=3):
    from harness.pipeline import CameraTensors
    from harness.train import orbit_cameras

    return CameraTensors.from_numpy(orbit_cameras(8, W, H)[i], DEV)


def _loose(got, ref, what):
    """The bound without a reference's slack (two routes to the same kernel: the order of the float atomics)."""
    hold(got, npy(ref).astype(np.float64), np.zeros((ref.shape[0], 2)), what)


VIEW = dict(W=160, H=96, n=2000, K=4, deg=1)


def _separate_absgrad(p, cam, bg, deg, v_img, v_alpha, render_depth=False):
    from gs_fused import activate_gaussians
    from harness.pipeline import render_view

    scales, quats, opac, dirs = activate_gaussians(p["means"], p["scales"], p["quats"], p["opacities"], cam.campos)
    out = render_view(p["means"], scales, quats, opac, (p["features_dc"], p["features_rest"]), cam, bg, deg,
                      render_depth=render_depth, retain_xys_grad=True, viewdirs=dirs, clamp_rgb=False, fused_depth=True,
                      absgrad=True)
    torch.autograd.backward([out["rgb"], out["alpha"][..., 0]], [v_img, v_alpha])
    return out


@pytest.mark.parametrize("deterministic", [False, True])
def test_render_gaussians_absgrad_equals_the_separate_ops(tune, deterministic):
    from gs_fused import DensifyStats, ViewSpec, render_gaussians
    from rasterizer import rasterize as R

    tune(two_round="0")
    W, H, n, K, deg = (VIEW[k] for k in ("W", "H", "n", "K", "deg"))
    cam, bg = _camera(W, H), torch.tensor([0.1, 0.2, 0.3], device=DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    v_img = torch.rand(H, W, 3, device=DEV, generator=g) * 2 - 1
    v_alpha = torch.rand(H, W, device=DEV, generator=g) * 2 - 1
    ref = _separate_absgrad(_model(n, K, 4), cam, bg, deg, v_img, v_alpha)
    spec = ViewSpec(H, W, cam.fx, cam.fy, cam.cx, cam.cy, deg, absgrad=True)
    R.set_deterministic(deterministic)
    try:
        got = []
        for _ in range(2):
            p = _model(n, K, 4)
            stats = DensifyStats(n, DEV, max(W, H))
            out = render_gaussians(p["means"], p["scales"], p["quats"], p["opacities"], p["features_dc"],
                                   p["features_rest"], cam.viewmat, cam.projmat, cam.campos, bg, spec, 1 << 20, stats=stats)
            torch.autograd.backward([out["rgb"], out["alpha"]], [v_img, v_alpha])
            torch.cuda.synchronize()
            got.append(stats)
    finally:
        R.set_deterministic(False)
    stats = got[0]
    assert torch.equal(out["rgb"], ref["rgb"])
    assert bool(stats.absgrad.any())
    _loose(stats.absgrad, ref["xys"].absgrad, "render_gaussians absgrad")
    # after one backward (the first update: every Gaussian's norm is written) xys_grad_norm is the absgrad's norm
    assert torch.allclose(stats.xys_grad_norm, stats.absgrad.norm(dim=-1), rtol=1e-6, atol=0)
    assert bool((stats.absgrad.norm(dim=-1) >= ref["xys"].grad.norm(dim=-1) * (1 - 1e-3)).all())
    if deterministic:
        assert torch.equal(got[0].absgrad, got[1].absgrad) and torch.equal(got[0].xys_grad_norm, got[1].xys_grad_norm)
    with pytest.raises(ValueError, match="absgrad"):
        render_gaussians(p["means"], p["scales"], p["quats"], p["opacities"], p["features_dc"], p["features_rest"],
                         cam.viewmat, cam.projmat, cam.campos, bg, spec, 1 << 20)


def test_view_graph_absgrad_replays_equal_eager_and_do_not_accumulate(tune):
    from gs_fused import DensifyStats, ViewSpec, l1_ssim_loss, render_gaussians
    from gs_fused.render import ViewGraph

    tune(two_round="0")
    W, H, n, K, deg = (VIEW[k] for k in ("W", "H", "n", "K", "deg"))
    cam, bg = _camera(W, H), torch.tensor([0.1, 0.2, 0.3], device=DEV)
    gt = torch.rand(H, W, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    spec = ViewSpec(H, W, cam.fx, cam.fy, cam.cx, cam.cy, deg, absgrad=True)
    loss_fn = lambda out, targets: l1_ssim_loss(out["rgb"], targets[0], 0.2, clamp_pred=True)  # noqa: E731
    q = _model(n, K, 6)
    stats_e = DensifyStats(n, DEV, max(W, H))
    oe = render_gaussians(q["means"], q["scales"], q["quats"], q["opacities"], q["features_dc"], q["features_rest"],
                          cam.viewmat, cam.projmat, cam.campos, bg, spec, 1 << 20, stats=stats_e)
    loss_fn(oe, (gt,)).backward()
    p = _model(n, K, 6)
    with pytest.raises(ValueError, match="absgrad"):
        ViewGraph(p, spec, 1 << 20, loss_fn, bg, [(H, W, 3)])
    stats = DensifyStats(n, DEV, max(W, H))
    vg = ViewGraph(p, spec, 1 << 20, loss_fn, bg, [(H, W, 3)], stats=stats)
    vg.capture(cam.viewmat, cam.projmat, cam.campos, (gt,))
    seen = []
    for _ in range(2):
        vg.replay(cam.viewmat, cam.projmat, cam.campos, (gt,))
        torch.cuda.synchronize()
        assert vg.fits()
        seen.append((stats.absgrad.clone(), stats.xys_grad_norm.clone()))
    assert bool(seen[0][0].any())
    _loose(seen[0][0], stats_e.absgrad, "graph replay 1 against eager")
    _loose(seen[1][0], seen[0][0], "graph replay 2 against replay 1")  # overwritten, not accumulated
    assert torch.allclose(seen[0][1], stats_e.xys_grad_norm, rtol=1e-3, atol=1e-3 * float(stats_e.xys_grad_norm.max()))
    assert float(seen[1][1].sum()) > 1.5 * float(seen[0][1].sum())  # ... while the statistic does accumulate


# ---- the trainer ------------------------------------------------------------------------------------------------------

def _train_stats(monkeypatch, **kw):
    """A short run without refinement -> the accumulated xys_grad_norm its statistics object ends with."""
    import harness.train as T

    made = []

    class Spy(T.DensifyState):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(T, "DensifyState", Spy)
    cfg = T.TrainConfig(num_gaussians=2000, width=160, height=96, num_views=4, iters=24, sh_degree=1,
                        sh_degree_interval=12, **kw)
    res = T.train(cfg, torch.device("cuda", 0))
    torch.cuda.synchronize()
    assert np.isfinite(res["param_checksum"])
    return made[-1].xys_grad_norm.detach().clone(), res


def test_trainer_statistics_agree_between_the_step_bodies(monkeypatch, tune):
    """`TrainConfig.absgrad` through FusedStep (ViewSpec) and SeparateStep (the rasterize functions): the accumulated
    statistics agree, and are at least the signed run's on every Gaussian."""
    tune(two_round="0")
    sep, res_sep = _train_stats(monkeypatch, absgrad=True)
    fus, res_fus = _train_stats(monkeypatch, absgrad=True, fused_render=True)
    off, _ = _train_stats(monkeypatch)
    assert res_sep["render"] == "separate ops" and res_fus["render"] == "one fused op" and res_sep["absgrad"] is True
    s, f, o = (npy(t).astype(np.float64) for t in (sep, fus, off))
    bound = 1e-3 * np.maximum(s, 1e-3 * s.max())
    print(f"trainer: fused against separate, worst error / bound = {(np.abs(f - s) / bound).max():.3e}; "
          f"absgrad / signed statistics = {s.sum() / o.sum():.3f}")
    assert (np.abs(f - s) <= bound).all()
    assert (s >= o - bound).all() and (s > o + bound).mean() > 0.25


def test_trainer_densifies_and_checkpoints_with_absgrad(tmp_path, tune):
    from gs_fused import RefineConfig
    from harness import checkpoint as CK
    from harness.train import TrainConfig, train

    rcfg = RefineConfig(warmup_length=10, refine_every=10, reset_alpha_every=6, stop_screen_size_at=200,
                        stop_split_at=60, densify_grad_thresh=0.0004)
    for fused in (False, True):
        d = tmp_path / ("fused" if fused else "separate")
        cfg = TrainConfig(num_gaussians=2000, width=160, height=96, num_views=4, iters=41, sh_degree=1,
                          sh_degree_interval=12, densify=True, refine=rcfg, absgrad=True, fused_render=fused,
                          checkpoint_dir=str(d), save_every=40)
        res = train(cfg, torch.device("cuda", 0))
        assert np.isfinite(res["param_checksum"]) and len(res["refinements"]) >= 2, res
        assert res["num_gaussians_end"] != res["num_gaussians_start"], res
        saved = torch.load(CK.latest_checkpoint(str(d)), map_location="cpu", weights_only=False)
        assert saved["step"] == 40
