"""GPU: the depth-distortion walk (csrc/distortion.hip) on lists built by the existing binning entries, against the
float64 autograd restatement of tests/distortion_reference.py fed the same lists; then the high-level op.

Bounds.  Forward maps (distortion, vsum, final_T) on stable pixels: e(X) = max|X - X64| / max|X64| <= 4 e32 + 2^-23,
e32 the same restatement run in float32 on the float64 run's decisions.  Where X64 itself is zero the kernel's map is
held to exact zero; where it is rounding noise around a mathematical zero (two Gaussians of equal depth: the term
between them vanishes, |X64| ~ 1e-16) the scale is max|values| -- the size of the quantities whose difference the
term is, with weights <= 1 -- instead of the noise.  The median on stable pixels equals the float32 value the
reference picks.  Gradients: `absgrad_reference.within_bound` (1e-3 relative per Gaussian, floor 1e-3 of the largest,
plus the decision slack U[g]).  The stability cap of every case is asserted on the CPU (tests/test_distortion_host.py)."""
import numpy as np
import pytest
import torch

import absgrad_reference as A
import distortion_reference as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -23


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_lists(sc):
    """ids, bins of a scene from the package's binning entries (the bounding-box pipeline of rasterizer.utils)."""
    from rasterizer.utils import bin_and_sort_gaussians, compute_cumulative_intersects

    H, W = sc["H"], sc["W"]
    tb = ((W + 15) // 16, (H + 15) // 16, 1)
    I, cum = compute_cumulative_intersects(cu(sc["num_tiles_hit"]))
    _, _, _, ids, bins = bin_and_sort_gaussians(sc["xys"].shape[0], I, cu(sc["xys"]), cu(sc["depths"]), cu(sc["radii"]),
                                                cum, tb, 16)
    return ids, bins, tb


_cache = {}


def case(name):
    """Scene, lists, the kernel's outputs and the float64 / float32 references: computed once per case."""
    if name in _cache:
        return _cache[name]
    import rasterizer.cuda as C

    sc = D.build_case(name)
    H, W = sc["H"], sc["W"]
    ids, bins, tb = gpu_lists(sc)
    xys, conics, opac, values = cu(sc["xys"]), cu(sc["conics"]), cu(sc["opacities"]), cu(sc["values"])
    # (a large scratch allocation filled with NaN and released: what torch.empty hands out next is not zeros)
    scratch = torch.full(((64 << 20) // 4,), float("nan"), device=DEV)
    del scratch
    fwd = C.distortion_forward(tb, (W, H, 1), ids, bins, xys, conics, opac, values)
    bwd = C.distortion_backward(H, W, ids, bins, xys, conics, opac, values, fwd[2], fwd[3], fwd[4],
                                cu(sc["v_distortion"]))
    torch.cuda.synchronize()
    ids_h, bins_h = ids.cpu().numpy(), bins.cpu().numpy().reshape(-1, 2)[:tb[0] * tb[1]]
    args = (H, W, ids_h, bins_h, sc["xys"], sc["conics"], sc["opacities"], sc["values"])
    ref = D.distortion_reference(*args, sc["v_distortion"])
    ref32 = D.distortion_reference(*args, dtype=torch.float32, decisions=ref["decisions"])
    _cache[name] = dict(sc=sc, ids=ids, bins=bins, bins_h=bins_h, tb=tb, fwd=[t.cpu() for t in fwd], bwd=[t.cpu() for t in bwd], ref=ref,
                        ref32=ref32, inputs=(xys, conics, opac, values))
    return _cache[name]


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_forward_maps_and_median_against_float64(name):
    c = case(name)
    sc, ref = c["sc"], c["ref"]
    dist, median, vsum, final_T, final_idx = c["fwd"]
    keep = ~ref["unstable"]
    print(f"{name}: {int(keep.sum())} of {keep.numel()} pixels stable; lists "
          f"{(c['bins_h'][:, 1] - c['bins_h'][:, 0]).tolist()}")
    assert keep.float().mean() >= 0.99
    e32 = D.e32_of(ref, c["ref32"], keep=keep)
    zscale = float(np.abs(sc["values"]).max())
    for key, got in (("distortion", dist), ("vsum", vsum), ("final_T", final_T)):
        want = ref[key][keep]
        err = float((got.double()[keep] - want).abs().max())
        scale = float(want.abs().max())
        if scale == 0.0:
            print(f"{name} {key}: the reference is exactly zero; kernel max |X| = {err:.3e}")
            assert err == 0.0, (name, key)
            continue
        if key == "distortion" and scale < EPS * zscale:  # (noise around a mathematical zero: see the module docstring)
            e32k = float((c["ref32"][key].double()[keep] - want).abs().max()) / zscale
            scale = zscale
        else:
            e32k = e32[key]
        bound = 4.0 * e32k + EPS
        print(f"{name} {key}: e = {err / scale:.3e}, e32 = {e32k:.3e}, bound = {bound:.3e}")
        assert err / scale <= bound, (name, key)
    assert torch.equal(median[keep], ref["median"][keep]), name
    assert torch.equal(final_idx.long()[keep], ref["final_idx"][keep]), name
    # exact zeros where nothing contributes
    nothing = ref["final_idx"] < 0
    for t in (dist, median, vsum):
        assert bool((t[nothing & keep] == 0).all())
    assert bool((final_T[nothing & keep] == 1).all()) and bool((final_idx[nothing & keep] == -1).all())
    for t in c["fwd"][:4]:
        assert bool(torch.isfinite(t).all())
    if name == "empty_tile":
        assert bool(nothing[32:, 48:].all())  # the bottom-right tile
        for t in (dist, median, vsum):
            assert bool((t[32:, 48:] == 0).all())
        assert bool((final_idx[32:, 48:] == -1).all())
    if name == "opaque":  # the stop rule inside the first batch
        assert int(final_idx.max()) < 39 and float(final_T.max()) < 1e-2


def term_scales(sc):
    """Per Gaussian and gradient component, the size of the quantities a gradient is a difference of: with weights
    <= 1, |g_k| <= 4 max|z| and S <= 4 max|z|, so |dD/dalpha| <= 4 max|z| (1 + 1 / (1 - alpha_max)), alpha_max =
    min(0.999, opacity); times sum_p |v_p| |chain factor| over the image.  Where the true gradient vanishes (equal
    depths: every term carries z_2 - z_1 = 0) the float64 reference is rounding noise around zero and the relative
    bound has nothing to hold on to; a float32 evaluation is then within a few roundings of THIS scale."""
    H, W = sc["H"], sc["W"]
    py, px = (a.reshape(-1).astype(np.float64) for a in np.meshgrid(np.arange(H), np.arange(W), indexing="ij"))
    v = np.abs(sc["v_distortion"].astype(np.float64)).reshape(-1)[:, None]
    xy, co = sc["xys"].astype(np.float64), sc["conics"].astype(np.float64)
    op = sc["opacities"].astype(np.float64).reshape(-1)
    a, b, c = co[:, 0][None], co[:, 1][None], co[:, 2][None]
    dx, dy = xy[:, 0][None] - px[:, None], xy[:, 1][None] - py[:, None]
    vis = np.exp(-np.maximum(0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy, 0.0))
    zmax = float(np.abs(sc["values"]).max())
    k = 4.0 * zmax * (1.0 + 1.0 / (1.0 - np.minimum(0.999, op)))
    s = lambda f: k * op * (v * vis * np.abs(f)).sum(axis=0)  # noqa: E731
    return {"v_xy": np.stack([s(a * dx + b * dy), s(b * dx + c * dy)], 1),
            "v_conic": np.stack([s(0.5 * dx * dx), s(dx * dy), s(0.5 * dy * dy)], 1),
            "v_opacity": k * (v * vis).sum(axis=0), "v_values": 2.0 * v.sum() * np.ones_like(op)}


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_gradients_against_autograd_in_float64(name):
    c = case(name)
    ref = c["ref"]
    scales = term_scales(c["sc"])
    for got, key in zip(c["bwd"], D.NAMES):
        want, U = ref[key].numpy(), ref["U"][key].numpy()
        assert bool(torch.isfinite(got).all())
        if float(np.abs(want).max()) <= EPS * float(scales[key].max()) and float(U.max()) == 0.0:
            # (also an exact zero: one Gaussian has no one to differ from, but a backward that rebuilds T_1 by a
            #  division does not return to 1 exactly)
            bound = 16.0 * EPS * scales[key]
            ratio = float((np.abs(got.numpy().reshape(want.shape)) / np.maximum(bound, 1e-300)).max())
            print(f"{name} {key}: the reference is zero or rounding noise ({np.abs(want).max():.3e}) around a vanishing "
                  f"gradient; kernel max |g| = {float(got.abs().max()):.3e}, worst |g| / (16 eps scale) = {ratio:.3e}")
            assert ratio <= 1.0, (name, key)
            continue
        ok, worst = A.within_bound(got.numpy().reshape(want.shape), want, U)
        print(f"{name} {key}: worst error / bound = {worst:.3e} (max |ref| = {np.abs(want).max():.3e})")
        assert ok, (name, key, worst)
    if name == "clamp":  # the clamped pair passes nothing to alpha: Gaussian 0's share of pixel (8, 8)
        import rasterizer.cuda as C

        sc = c["sc"]
        v = torch.zeros((16, 16), device=DEV)
        v[8, 8] = 1.0
        fwd = [t.to(DEV) for t in c["fwd"]]
        g = C.distortion_backward(16, 16, c["ids"], c["bins"], *c["inputs"], fwd[2], fwd[3], fwd[4], v)
        assert float(g[2][0]) == 0.0 and float(g[0][0].abs().max()) == 0.0 and float(g[1][0].abs().max()) == 0.0
        assert float(g[3][0]) != 0.0 and float(g[2][1:].abs().max()) > 0.0
        assert sc["opacities"][0, 0] == np.float32(0.9995)


def test_a_view_with_nothing_on_screen_launches_nothing():
    import rasterizer.cuda as C

    n, H, W = 5, 17, 33
    xys, conics = torch.zeros((n, 2), device=DEV), torch.ones((n, 3), device=DEV)
    opac, values = torch.full((n, 1), 0.5, device=DEV), torch.ones((n,), device=DEV)
    empty_ids, bins = torch.zeros((0,), dtype=torch.int32, device=DEV), torch.zeros((6, 2), dtype=torch.int32, device=DEV)
    dist, median, vsum, T, idx = C.distortion_forward((3, 2, 1), (W, H, 1), empty_ids, bins, xys, conics, opac, values)
    for t in (dist, median, vsum):
        assert t.shape == (H, W) and bool((t == 0).all())
    assert bool((T == 1).all()) and bool((idx == -1).all())
    grads = C.distortion_backward(H, W, empty_ids, bins, xys, conics, opac, values, vsum, T, idx,
                                  torch.ones((H, W), device=DEV))
    assert [tuple(g.shape) for g in grads] == [(n, 2), (n, 3), (n,), (n,)]
    assert all(bool((g == 0).all()) for g in grads)
    # ... and through the op: radii 0, no tile hit
    from gs_fused import depth_distortion

    xys.requires_grad_(True)
    d, m = depth_distortion(xys, values, torch.zeros((n,), dtype=torch.int32, device=DEV), conics,
                            torch.zeros((n,), dtype=torch.int32, device=DEV), values, opac, H, W)
    assert bool((d == 0).all()) and bool((m == 0).all()) and not m.requires_grad
    d.sum().backward()
    assert xys.grad is None or bool((xys.grad == 0).all())


def _view(sc, grad=True):
    t = lambda k: cu(sc[k]).requires_grad_(grad)  # noqa: E731
    return dict(xys=t("xys"), conics=t("conics"), opac=t("opacities"), values=t("values"), depths=cu(sc["depths"]),
                radii=cu(sc["radii"]), tiles=cu(sc["num_tiles_hit"]))


def test_the_op_after_the_rgb_pass_walks_the_cached_lists_and_leaves_the_rgb_pass_alone():
    import rasterizer.cuda as C
    from gs_fused import depth_distortion, distortion_loss
    from rasterizer import rasterize as R
    from rasterizer import rasterize_gaussians

    sc = D.build_case("empty_tile")
    H, W = sc["H"], sc["W"]
    rng = np.random.default_rng(3)
    colors = cu(rng.uniform(0.05, 1.0, (sc["xys"].shape[0], 3)).astype(np.float32))
    bg = cu(np.array([0.2, 0.5, 0.3], np.float32))
    v_img, vD = cu(rng.uniform(-1, 1, (H, W, 3)).astype(np.float32)), cu(sc["v_distortion"])

    def run(with_op, det=False):
        """The RGB pass forward, the op with its backward in between (or not), the RGB backward.  `det`: the RGB pass
        runs in deterministic mode (fixed summation order: its gradients are comparable bit for bit); the mode is off
        again before the op, which refuses it."""
        R._bin_cache["key"] = None
        v = _view(sc)
        col = colors.clone().requires_grad_(True)
        if det:
            R.set_deterministic(True)
        try:
            img = rasterize_gaussians(v["xys"], v["depths"], v["radii"], v["conics"], v["tiles"], col, v["opac"], H, W,
                                      16, background=bg)
        finally:
            if det:
                R.set_deterministic(False)  # (drops the cached lists: after a deterministic pass the op builds its own)
        ids, bins = (img.grad_fn.saved_tensors[i] for i in (0, 1))
        extra = None
        if with_op:
            builds = dict(R.counters)
            dist, med = depth_distortion(v["xys"], v["depths"], v["radii"], v["conics"], v["tiles"], v["values"],
                                         v["opac"], H, W)
            if not det:
                assert dict(R.counters) == builds  # a cache hit: no list was built
            assert not med.requires_grad and dist.requires_grad
            gd = torch.autograd.grad((dist * vD).sum(), [v["xys"], v["conics"], v["opac"], v["values"]])
            extra = (dist.detach(), med, gd, ids, bins, v)
        (img * v_img).sum().backward()
        torch.cuda.synchronize()
        return img.detach(), [t.grad.clone() for t in (v["xys"], v["conics"], v["opac"], col)], extra

    assert not R.is_deterministic()
    img0, g0, _ = run(False)
    img1, g1, (dist, med, gd, ids, bins, v) = run(True)
    assert torch.equal(img0, img1)
    # the RGB pass's gradients, bit for bit: with its backward in the fixed summation order (the atomic sums of the
    # default backward differ in their last bits between two runs of the RGB pass alone)
    imgd0, d0, _ = run(False, det=True)
    imgd1, d1, (distd, medd, _, _, _, _) = run(True, det=True)
    assert torch.equal(imgd0, imgd1) and torch.equal(imgd0, img0)
    for a, b in zip(d0, d1):
        assert torch.equal(a, b)
    assert torch.equal(distd, dist) and torch.equal(medd, med)  # (lists built again: the same lists)
    for a, b in zip(g0, g1):  # the default backward: to the rounding of its atomic sums
        assert float((a - b).abs().max()) <= 1e-5 * max(float(b.abs().max()), 1e-30)
    # the same bits as the low-level call on the cached lists
    tb = ((W + 15) // 16, (H + 15) // 16, 1)
    low = C.distortion_forward(tb, (W, H, 1), ids, bins, v["xys"].detach(), v["conics"].detach(), v["opac"].detach(),
                               v["values"].detach())
    assert torch.equal(low[0], dist) and torch.equal(low[1], med)
    # the op's backward is the low-level backward on the same lists: atomic sums, so to rounding, not to the bit
    lowg = C.distortion_backward(H, W, ids, bins, v["xys"].detach(), v["conics"].detach(), v["opac"].detach(),
                                 v["values"].detach(), low[2], low[3], low[4], vD)
    for a, b, nm in zip(gd, lowg, D.NAMES):
        err = float((a.reshape(b.shape) - b).abs().max()) / max(float(b.abs().max()), 1e-30)
        print(f"op vs low-level {nm}: max relative difference {err:.2e}")
        assert err <= 1e-5
    loss = distortion_loss(dist, mask=torch.ones((H, W), device=DEV))
    assert abs(float(loss) - float(dist.mean())) <= 1e-7 * abs(float(dist.mean()))
    half = torch.zeros((H, W), dtype=torch.bool, device=DEV)
    half[:, : W // 2] = True
    assert abs(float(distortion_loss(dist, mask=half)) - float((dist * half).sum() / (H * W))) <= 1e-6 * float(loss)


def test_refusals_name_the_option():
    from gs_fused import depth_distortion
    from rasterizer import rasterize as R

    sc = D.build_case("clamp")
    v = _view(sc, grad=False)
    args = (v["xys"], v["depths"], v["radii"], v["conics"], v["tiles"], v["values"], v["opac"], 16, 16)
    with pytest.raises(ValueError, match="depth_distortion.*block_width"):
        depth_distortion(*args, block_width=8)
    cpu = tuple(t.cpu() if isinstance(t, torch.Tensor) else t for t in args)
    with pytest.raises(ValueError, match="depth_distortion.*CPU"):
        depth_distortion(*cpu)
    assert not R.is_deterministic()
    R.set_deterministic(True)
    try:
        with pytest.raises(ValueError, match="depth_distortion.*deterministic"):
            depth_distortion(*args)
    finally:
        R.set_deterministic(False)
    d, m = depth_distortion(*args)
    assert d.shape == (16, 16) and m.shape == (16, 16)
