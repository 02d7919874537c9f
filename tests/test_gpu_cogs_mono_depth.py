"""GPU: the fused monocular-depth heads through the harness -- `optional_depth_terms(fused=True)` returns the three terms
of the float64 restatement (tests/mono_depth_reference.py) under the keys of the torch path, with and without a per-view
mask, and the co-gs loop of `harness.train` runs with `fused_mono_depth=True`."""
import numpy as np
import pytest
import torch

import mono_depth_reference as M
from test_gpu_mono_depth import TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = {"depth_local_pearson": "local_pearson", "log_depth": "log_depth", "tv_loss": "tv"}


class _Cfg:
    use_pearson_depth = True
    local_patch_size = 16
    depth_loss_stop_iteration = 100
    use_scaled_est_depth = True
    use_depth_regularization = True
    using_tv_loss = True


@pytest.mark.parametrize("masked", [False, True])
def test_optional_depth_terms_fused_returns_the_terms_of_the_restatement(masked):
    from harness import cogs_losses as CL

    H, W, box = 48, 64, _Cfg.local_patch_size
    pred, gt, img = M.smooth_noise(H, W, 21)
    mask = (np.random.default_rng(22).uniform(size=(H, W, 1)) < 0.8).astype(np.float32) if masked else None
    tg, ti = torch.from_numpy(gt).to(DEV), torch.from_numpy(img).to(DEV)
    tm = None if mask is None else torch.from_numpy(mask).to(DEV)
    rows, cols = CL.local_pearson_patches(H, W, box, 0.5, torch.Generator(device=DEV).manual_seed(5), DEV)
    assert rows.numel() == 6 and rows.dtype == torch.int64 and rows.is_cuda
    p = torch.from_numpy(pred[..., None]).to(DEV).requires_grad_(True)
    terms = CL.optional_depth_terms(_Cfg, 50, p, tg, ti, torch.Generator(device=DEV).manual_seed(5), (0.875, 0.125),
                                    fused=True, mask=tm)
    # the torch path takes the products; the same keys in the same order (depth_gs.py:477-531)
    q = torch.from_numpy(pred).to(DEV)
    plain = CL.optional_depth_terms(_Cfg, 50, q if tm is None else q * tm[..., 0], tg if tm is None else tg * tm[..., 0],
                                    ti, torch.Generator(device=DEV).manual_seed(5), (0.875, 0.125))
    assert list(terms) == list(plain) == ["depth_local_pearson", "log_depth", "depth_reg_loss", "tv_loss"]
    assert float(terms["depth_reg_loss"]) == float(plain["depth_reg_loss"])      # that term is the same head either way
    m2 = None if mask is None else mask[..., 0]
    s, t = (pred.astype(np.float64), gt.astype(np.float64)) if m2 is None else M.products(pred, gt, m2)
    want = {"depth_local_pearson": M.local_pearson(s, t, box, rows.cpu().numpy(), cols.cpu().numpy(), m2),
            "log_depth": M.log_depth(s, t, img, 0.875, 0.125, m2), "tv_loss": M.tv(s, m2)}
    for key, name in KEYS.items():
        p.grad = None
        terms[key].backward()
        loss64, grad64 = want[key]
        assert abs(float(terms[key]) - loss64) <= TOL[name][0] * abs(loss64), key
        assert abs(float(plain[key]) - loss64) <= 1e-5 * abs(loss64), key
        grad = p.grad.cpu().numpy().reshape(H, W).astype(np.float64)
        assert np.abs(grad - grad64).max() <= TOL[name][1] * np.abs(grad64).max(), key
    late = CL.optional_depth_terms(_Cfg, 20_000, p, tg, ti, None, None, fused=True, mask=tm)
    assert list(late) == ["depth_reg_loss"]                                      # the step limits and the missing scale


def _train(fused, **over):
    """-> (result, [(step, {term: value}, {term: float64 value})]) of a 20-step co-gs run whose scene fills the frame (a
    patch of constant depth -- empty background -- is 0 / 0 in the source's local Pearson).  Every call of
    `optional_depth_terms` is repeated on the same tensors through the torch path in float64, from the same state of the
    device's random generator (the same patch corners); with `fused` the heads' terms are held to it."""
    import harness.train as HT

    seen = []
    real = HT.cogs_losses.optional_depth_terms

    def terms(cfg, step, pred, gt, img, *a, fused=False, mask=None, **k):
        state = torch.cuda.get_rng_state(DEV)
        out = real(cfg, step, pred, gt, img, *a, fused=fused, mask=mask, **k)
        torch.cuda.set_rng_state(state, DEV)
        with torch.no_grad():
            d64 = (pred if mask is None else pred * mask).double()
            g64 = (gt if mask is None else gt * mask[..., 0]).double()
            ref = {n: float(v) for n, v in real(cfg, step, d64, g64, img.double(), *a, **k).items()}
        assert list(ref) == list(out)
        seen.append((step, {n: float(v.detach()) for n, v in out.items()}, ref))
        if fused:
            for key, v in ref.items():
                assert abs(seen[-1][1][key] - v) <= TOL[KEYS[key]][0] * abs(v), (step, key)
        return out

    HT.cogs_losses.optional_depth_terms = terms
    try:
        torch.manual_seed(11)
        kw = dict(model="co-gs", num_gaussians=2000, width=96, height=64, num_views=4, iters=20, sh_degree=1,
                  sh_degree_interval=10, eval_views=2, scene_scale=(0.15, 0.5), cam_radius=2.0,
                  depth_loss_start_iteration=4, background_color="random", densify=False, use_est_depth=True,
                  use_pearson_depth=True, local_patch_size=16, use_scaled_est_depth=True, using_tv_loss=True,
                  log_every=1, fused_mono_depth=fused)
        kw.update(over)
        res = HT.train(HT.TrainConfig(**kw), torch.device("cuda", 0))
    finally:
        HT.cogs_losses.optional_depth_terms = real
    return res, seen


def test_cogs_loop_trains_on_the_fused_heads_as_on_the_torch_path():
    from rasterizer import rasterize as RZ

    RZ.set_deterministic(True)   # fixed summation order in the compositing backward: two runs are comparable
    try:
        plain, seen_plain = _train(False)
        fused, seen_fused = _train(True)
    finally:
        RZ.set_deterministic(False)
    for res, seen in ((plain, seen_plain), (fused, seen_fused)):
        assert [s for s, _, _ in seen] == list(range(5, 20))
        for _, t, _ in seen:
            assert set(t) == set(KEYS) and all(np.isfinite(v) for v in t.values())
        assert len(res["losses"]) == 20 and all(np.isfinite(v) for v in res["losses"])
        assert np.isfinite(res["param_checksum"])
    # the same seed: steps 0-4 (no depth terms yet) are the same run bit for bit, so step 5 sees the same parameters, the
    # same view and the same patch corners -- the float64 values of its terms are the same in both runs, and the two
    # runs' terms differ by the two paths' errors against them: the torch path's own float32 error AT THIS STEP (measured
    # here against its float64 run: on a rendered depth of 2 +- 0.1 per patch it is far above the r of the golden
    # cases, whose depths spread over 0.5 .. 4) plus the heads' tolerance; the loss adds the float32 sum of its terms
    assert plain["losses"][:5] == fused["losses"][:5]
    (_, a, ref), (_, b, ref_b) = seen_plain[0], seen_fused[0]
    bound = 4 * 2.0 ** -24 * abs(plain["losses"][5])
    for key, name in KEYS.items():
        own = abs(a[key] - ref[key]) + abs(ref[key] - ref_b[key])   # (the second: 0 when both runs saw the same bits)
        print(f"step 5 {key}: float64 {ref[key]:.12g} torch {a[key]:.9g} (rel {own / abs(ref[key]):.2e}) "
              f"fused {b[key]:.9g} (rel {abs(b[key] - ref[key]) / abs(ref[key]):.2e})")
        assert abs(a[key] - b[key]) <= own + TOL[name][0] * abs(ref[key]), key
        bound += own + TOL[name][0] * abs(ref[key])
    print(f"step 5 loss: torch {plain['losses'][5]:.9g} fused {fused['losses'][5]:.9g} bound {bound:.3g}")
    assert abs(plain["losses"][5] - fused["losses"][5]) <= bound
    print(f"step 19 loss: torch {plain['losses'][-1]:.9g} fused {fused['losses'][-1]:.9g}")


def test_masked_cogs_loop_passes_the_mask_into_the_heads():
    """Under a per-view mask the local-Pearson term is off (a patch inside the masked-out region is two constant images:
    0 / 0 in the source); the log-depth and TV terms get the mask inside their kernels."""
    res, seen = _train(True, mask="box", use_pearson_depth=False, iters=12)
    assert [s for s, _, _ in seen] == list(range(5, 12))
    for _, t, _ in seen:
        assert set(t) == {"log_depth", "tv_loss"} and all(np.isfinite(v) and v > 0 for v in t.values())
    assert all(np.isfinite(v) for v in res["losses"])
