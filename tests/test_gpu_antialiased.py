"""GPU: the antialiased rasterize mode (`rasterize_mode="antialiased"`: the view composites opacities * compensation)
inside the projection kernels -- gsr_project_forward_aa / gsr_project_backward_aa -- and on every route above them:
the one-call view (gs_fused.render_gaussians, ViewGraph), gs_fused.project_gaussians_antialiased, the trainer's three
step bodies and gs_fusion.fuse_views.

Scenes: case A = blob_scene(4000, seed=4) from orbit_cameras(8, 160, 96)[3] (every Gaussian visible, most of them
with a compensation below 0.8); case B = blob_scene(30000, seed=4) at 320 x 176, the scene of tests/test_gpu_render.py.
The kernel-level tests append 99 Gaussians the projection culls (33 behind the camera, 33 off the screen beyond the
guard band, 33 whose 2-D determinant is zero), which also makes n no multiple of the workgroup size."""
import functools

import numpy as np
import pytest
import torch

from harness import scene as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = {"A": (4000, 160, 96), "B": (30_000, 320, 176)}


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def npy(t):
    return t.detach().cpu().numpy()


def _raw(n, K=16):
    from harness.train import blob_scene

    return blob_scene(n, seed=4, sh_degree={1: 0, 4: 1, 9: 2, 16: 3}[K])


def _model(n, K):
    return {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in _raw(n, K).items()}


def _camera_np(W, H, i=3):
    from harness.train import orbit_cameras

    return orbit_cameras(8, W, H)[i]


def _camera(W, H, i=3):
    from harness.pipeline import CameraTensors

    return CameraTensors.from_numpy(_camera_np(W, H, i), DEV)


def _separate_ops(p, cam, bg, deg, render_depth, mode="antialiased"):
    """`_separate_ops` of tests/test_gpu_render.py with the rasterize mode handed on."""
    from gs_fused import activate_gaussians
    from harness.pipeline import render_view

    scales, quats, opac, dirs = activate_gaussians(p["means"], p["scales"], p["quats"], p["opacities"], cam.campos)
    return render_view(p["means"], scales, quats, opac, (p["features_dc"], p["features_rest"]), cam, bg, deg,
                       rasterize_mode=mode, render_depth=render_depth, retain_xys_grad=True, viewdirs=dirs,
                       clamp_rgb=False, fused_depth=True)


# ---- the two entries of csrc/project.hip ----------------------------------------------------------------------------
def _project_args(k, cam):
    return (k["means3d"], k["scales"], 1.0, k["quats"], cu(cam.viewmat[:3]), cu(cam.projmat), cam.fx, cam.fy, cam.cx,
            cam.cy, cam.height, cam.width)


@functools.lru_cache(maxsize=None)
def _kernel_case():
    """Case A, activated, plus the 99 culled rows -> (inputs on the device, camera, the existing entry's forward).
    Shared by the kernel tests; nothing in it is modified."""
    import rasterizer.cuda as C

    n0, W, H = CASES["A"]
    raw, cam = _raw(n0), _camera_np(W, H)
    V = cam.viewmat.astype(np.float64)
    R, eye = V[:3, :3], -V[:3, :3].T @ V[:3, 3]
    rng = np.random.default_rng(99)

    def at(x, y, z):  # camera space -> world
        return (eye + (R.T @ np.stack([x, y, z])).T).astype(np.float32)

    def unit(m):
        q = rng.standard_normal((m, 4))
        return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)

    small = lambda m: rng.uniform(0.01, 0.05, (m, 3)).astype(np.float32)  # noqa: E731
    z = rng.uniform(3, 8, 33)
    behind = (at(rng.uniform(-1, 1, 33), rng.uniform(-1, 1, 33), -z), small(33), unit(33))
    limx = 1.3 * 0.5 * W / cam.fx
    sign = np.where(rng.random(33) < 0.5, -1.0, 1.0)
    beyond = (at(sign * rng.uniform(2.0, 4.0, 33) * limx * z, rng.uniform(-0.1, 0.1, 33) * z, z), small(33), unit(33))
    # needles a thousand scene units long in front of the camera: cov2d is rank one far above the 0.3 blur, and for
    # about one in six of them its float32 determinant comes out exactly zero -- those the projection culls.  Which
    # ones is decided by the entry that exists already (bit-identical to the CPU oracle), not by the code under test.
    m = 600
    zz = rng.uniform(3, 8, m)
    cand = (at(rng.uniform(-0.2, 0.2, m) * zz, rng.uniform(-0.1, 0.1, m) * zz, zz),
            np.tile(np.float32([1e3, 1e-6, 1e-6]), (m, 1)), unit(m))
    radii = C.project_gaussians_forward(m, cu(cand[0]), cu(cand[1]), 1.0, cu(cand[2]), cu(cam.viewmat[:3]),
                                        cu(cam.projmat), cam.fx, cam.fy, cam.cx, cam.cy, H, W, 16, 0.01)[3]
    flat = np.nonzero(npy(radii) == 0)[0][:33]
    assert len(flat) == 33
    zero_det = tuple(a[flat] for a in cand)

    q = raw["quats"] / np.linalg.norm(raw["quats"], axis=1, keepdims=True)
    parts = [(raw["means"], np.exp(raw["scales"]), q), behind, beyond, zero_det]
    k = {"means3d": cu(np.concatenate([p[0] for p in parts]).astype(np.float32)),
         "scales": cu(np.concatenate([p[1] for p in parts]).astype(np.float32)),
         "quats": cu(np.concatenate([p[2] for p in parts]).astype(np.float32))}
    n = n0 + 99
    opac = torch.cat([torch.sigmoid(cu(raw["opacities"])),
                      cu(rng.uniform(0.05, 0.95, (99, 1)).astype(np.float32))]).contiguous()
    fwd = C.project_gaussians_forward(n, *_project_args(k, cam), 16, 0.01)
    assert n % 256 != 0 and not npy(fwd[3])[n0:].any() and (npy(fwd[3])[:n0] > 0).all()
    return n, n0, k, opac, cam, fwd


def test_forward_entry_equals_the_existing_one_and_torchs_product():
    import rasterizer.cuda as C

    n, n0, k, opac, cam, ref = _kernel_case()
    out = C.project_gaussians_forward_aa(n, *_project_args(k, cam), 16, 0.01, opac)
    for a, b, nm in zip(out[:7], ref, ("cov3d", "xys", "depths", "radii", "conics", "compensation", "num_tiles_hit")):
        assert torch.equal(a, b), nm
    comp = ref[5]
    assert out[7].shape == opac.shape and torch.equal(out[7], opac * comp[:, None])
    assert not out[7][n0:].any() and (out[7][:n0] > 0).all()
    flat = C.project_gaussians_forward_aa(n, *_project_args(k, cam), 16, 0.01, opac.view(-1).contiguous())[7]
    assert flat.shape == (n,) and torch.equal(flat, out[7].view(-1))
    frac = float((comp[:n0] < 0.8).float().mean())
    print(f"case A: compensation < 0.8 on {frac:.0%}, median {float(comp[:n0].median()):.2f}")
    assert frac > 0.9  # (the scene is one the mode matters on)


def test_backward_entry_equals_the_existing_one_fed_the_products_cotangent():
    import rasterizer.cuda as C

    n, n0, k, opac, cam, fwd = _kernel_case()
    cov3d, xys, depths, radii, conics, comp, tiles = fwd
    g = torch.Generator(device=DEV).manual_seed(7)
    r = lambda *shape: torch.randn(*shape, device=DEV, generator=g)  # noqa: E731
    v_xy, v_depth, v_conic, v_oaa, v_ext = r(n, 2), r(n), r(n, 3), r(n, 1), r(n)
    saved = (cov3d, radii, conics, comp)
    names = ("v_cov2d", "v_cov3d", "v_mean3d", "v_scale", "v_quat")

    def existing(v_comp):
        return C.project_gaussians_backward(n, *_project_args(k, cam), *saved, v_xy, v_depth, v_conic, v_comp)

    def new(v_comp, v_in, **kw):
        return C.project_gaussians_backward_aa(n, *_project_args(k, cam), *saved, opac, v_xy, v_depth, v_conic, v_comp,
                                               v_in, **kw)

    prod = (v_oaa * opac).view(-1)  # torch, float32: the product's cotangent with respect to the compensation
    want_v_opac = v_oaa * comp[:, None]
    ref = existing(prod)
    # 1. v_opacities written over its input
    buf = v_oaa.clone()
    out = new(None, buf, in_place=True)
    for a, b, nm in zip(out[:5], ref, names):
        assert torch.equal(a, b), nm
    assert out[5].data_ptr() == buf.data_ptr() and torch.equal(buf, want_v_opac) and out[6] is None
    assert not buf[n0:].any()
    # 2. an external v_compensation on top
    ref2 = existing(v_ext + prod)
    out2 = new(v_ext, v_oaa)
    for a, b, nm in zip(out2[:5], ref2, names):
        assert torch.equal(a, b), nm
    assert torch.equal(out2[5], want_v_opac) and out2[5].data_ptr() != v_oaa.data_ptr()
    assert not torch.equal(ref2[2], ref[2])  # (the external term reached the chain)
    # 3. the cotangent the chain took, handed out for the pose pass
    out3 = new(v_ext, v_oaa, want_v_compensation=True)
    assert torch.equal(out3[6], v_ext + prod)
    for a, b, nm in zip(out3[:5], ref2, names):
        assert torch.equal(a, b), nm
    out4 = new(None, v_oaa, want_v_compensation=True)
    assert torch.equal(out4[6], prod) and torch.equal(out4[2], ref[2])


def test_the_opacity_cotangents_path_through_the_compensation_against_float64():
    """Only v_opacities_aa is non-zero: what reaches means, scales and quats went through the compensation.  Held to
    tests/projection_reference.project_vjp_fp64 per row at 1e-3, the bar of tests/test_gpu_kernels.py::
    test_project_backward, on the rows tests/test_project_fp64.py:45-49 names: visible, inside the reference's guard
    band, compensation < 0.9."""
    import rasterizer.cuda as C
    from projection_reference import project_vjp_fp64

    n, n0, k, opac, cam, fwd = _kernel_case()
    cov3d, xys, depths, radii, conics, comp, tiles = fwd
    g = torch.Generator(device=DEV).manual_seed(8)
    v_oaa = torch.randn(n, 1, device=DEV, generator=g)
    out = C.project_gaussians_backward_aa(n, *_project_args(k, cam), cov3d, radii, conics, comp, opac, None, None, None,
                                          None, v_oaa)
    v_comp64 = npy(v_oaa).astype(np.float64)[:, 0] * npy(opac).astype(np.float64)[:, 0]
    ref = project_vjp_fp64(npy(k["means3d"]), npy(k["scales"]), 1.0, npy(k["quats"]), cam.viewmat[:3], cam.projmat,
                           cam.fx, cam.fy, cam.cx, cam.cy, cam.height, cam.width, npy(comp), None, None, None, v_comp64)
    rows = (npy(radii) > 0) & ref[3] & (npy(comp) < 0.9)
    print(f"rows compared: {rows.sum()} of {n0}")
    assert rows.sum() >= 0.5 * n0
    for o, f, nm in zip(out[2:5], ref[:3], ("v_mean3d", "v_scale", "v_quat")):
        o, f = npy(o).astype(np.float64)[rows], f[rows]
        rowmax = np.abs(f).max(axis=-1, keepdims=True)
        e = np.abs(o - f) / np.maximum(rowmax, 1e-6 * np.abs(f).max())
        print(f"{nm}: per row {e.max():.2e}")
        assert np.abs(f).max() > 0 and e.max() < 1e-3, f"{nm}: {e.max():.3e}"


# ---- the one-call view ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,deg,render_depth", [(16, 3, False), (4, 1, True)])
@pytest.mark.parametrize("case", ["A", "B"])
def test_render_gaussians_antialiased_equals_the_separate_ops(case, K, deg, render_depth):
    from gs_fused import DensifyStats, ViewSpec, densify_stats_, render_gaussians

    n, W, H = CASES[case]
    cam = _camera(W, H)
    bg = torch.tensor(S.BACKGROUND, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    v_img = torch.rand(H, W, 3, device=DEV, generator=g) * 2 - 1
    v_alpha = torch.rand(H, W, device=DEV, generator=g) * 2 - 1
    v_dep = torch.rand(H, W, device=DEV, generator=g) * 2 - 1
    cap = 4_000_000

    pa = _model(n, K)
    ref = _separate_ops(pa, cam, bg, deg, render_depth)
    torch.autograd.backward([ref["rgb"], ref["alpha"][..., 0]], [v_img, v_alpha])
    stats_ref = DensifyStats(n, DEV, max(W, H))
    densify_stats_(ref["xys"].grad, ref["radii"], max(W, H), *stats_ref.as_tuple(), first=True)

    def view(p, mode="antialiased", stats=None):
        spec = ViewSpec(H, W, cam.fx, cam.fy, cam.cx, cam.cy, deg, render_depth=render_depth, rasterize_mode=mode)
        return render_gaussians(p["means"], p["scales"], p["quats"], p["opacities"], p["features_dc"],
                                p["features_rest"], cam.viewmat, cam.projmat, cam.campos, bg, spec, capacity=cap,
                                stats=stats)

    pb = _model(n, K)
    stats = DensifyStats(n, DEV, max(W, H))
    out = view(pb, stats=stats)
    torch.cuda.synchronize()
    assert 0 < int(out["count"][0]) < cap
    assert torch.equal(out["rgb"], ref["rgb"]) and torch.equal(out["alpha"], ref["alpha"][..., 0])
    assert torch.equal(out["radii"], ref["radii"])
    torch.autograd.backward([out["rgb"], out["alpha"]], [v_img, v_alpha])
    for k in pa:
        a, b = pa[k].grad, pb[k].grad
        assert (a - b).abs().max().item() <= 2e-5 * a.abs().max().item() + 1e-12, k
    for a, b in zip(stats_ref.as_tuple(), stats.as_tuple()):
        assert torch.allclose(a.float(), b.float(), rtol=1e-5, atol=1e-9)
    if render_depth:  # the accumulated depth and its gradient, as tests/test_gpu_render.py holds them
        d_ref = ref["depth"][..., 0] * ref["alpha"][..., 0]
        ok = ref["alpha"][..., 0] > 0
        assert (out["depth"] - d_ref)[ok].abs().max().item() < 1e-4 * float(out["depth"].max())
        pd = _model(n, K)
        ref2 = _separate_ops(pd, cam, bg, deg, render_depth)
        (ref2["depth"][..., 0] * ref2["alpha"][..., 0]).backward(v_dep * ok)
        pe = _model(n, K)
        view(pe)["depth"].backward(v_dep * ok)
        for k in ("means", "scales", "quats", "opacities"):
            a, b = pd[k].grad, pe[k].grad
            assert (a - b).abs().max().item() <= 1e-3 * a.abs().max().item() + 1e-12, k
        assert pe["means"].grad.abs().sum().item() > 0
    # the mode is not ignored
    with torch.no_grad():
        classic = view(_model(n, K), mode="classic")
    diff = float((classic["rgb"] - out["rgb"]).abs().max())
    print(f"case {case}: antialiased vs classic, worst pixel {diff:.3f}")
    assert diff > {"A": 0.1, "B": 0.05}[case]


def test_an_unknown_rasterize_mode_is_refused():
    from gs_fused import ViewSpec

    with pytest.raises(ValueError, match="Unknown rasterize_mode"):
        ViewSpec(96, 160, 100.0, 100.0, 80.0, 48.0, 3, rasterize_mode="smooth")


def test_view_graph_with_an_antialiased_spec():
    """Three replays over two cameras equal the eager antialiased views, at the bars of
    tests/test_gpu_render.py::test_view_graph_replays_equal_eager_views."""
    from gs_fused import DensifyStats, ViewSpec, l1_ssim_loss, render_gaussians
    from gs_fused.render import ViewGraph

    n, W, H = CASES["A"]
    K, deg, cap = 16, 2, 1_000_000
    bg = torch.tensor(S.BACKGROUND, device=DEV)
    two = [_camera(W, H, 3), _camera(W, H, 5)]
    cams = [two[0], two[1], two[0]]
    spec = ViewSpec(H, W, two[0].fx, two[0].fy, two[0].cx, two[0].cy, deg, rasterize_mode="antialiased")
    g = torch.Generator(device=DEV).manual_seed(1)
    gts = [torch.rand(H, W, 3, device=DEV, generator=g) for _ in cams]
    loss_fn = lambda out, targets: l1_ssim_loss(out["rgb"], targets[0], 0.2, clamp_pred=True)  # noqa: E731

    p = _model(n, K)
    stats = DensifyStats(n, DEV, max(W, H))
    vg = ViewGraph(p, spec, cap, loss_fn, bg, [(H, W, 3)], stats=stats)
    vg.capture(cams[0].viewmat, cams[0].projmat, cams[0].campos, (gts[0],))
    q = _model(n, K)
    stats_e = DensifyStats(n, DEV, max(W, H))
    classic = ViewSpec(H, W, two[0].fx, two[0].fy, two[0].cx, two[0].cy, deg)
    for i, (cam, gt) in enumerate(zip(cams, gts)):
        loss, out = vg.replay(cam.viewmat, cam.projmat, cam.campos, (gt,))
        for t in q.values():
            t.grad = None
        oe = render_gaussians(q["means"], q["scales"], q["quats"], q["opacities"], q["features_dc"],
                              q["features_rest"], cam.viewmat, cam.projmat, cam.campos, bg, spec, cap, stats=stats_e)
        le = loss_fn(oe, (gt,))
        le.backward()
        torch.cuda.synchronize()
        assert vg.fits()
        assert torch.equal(out["rgb"], oe["rgb"]) and abs(float(loss) - float(le)) < 1e-6
        for k in p:
            a, b = q[k].grad, p[k].grad
            assert (a - b).abs().max().item() <= 2e-5 * a.abs().max().item() + 1e-12, (i, k)
        with torch.no_grad():
            oc = render_gaussians(q["means"], q["scales"], q["quats"], q["opacities"], q["features_dc"],
                                  q["features_rest"], cam.viewmat, cam.projmat, cam.campos, bg, classic, cap)
        assert float((oc["rgb"] - out["rgb"]).abs().max()) > 0.1
    for a, b in zip(stats_e.as_tuple(), stats.as_tuple()):
        assert torch.allclose(a.float(), b.float(), rtol=1e-5, atol=1e-9)


# ---- the op for callers that keep the separate ops ------------------------------------------------------------------
def _two_routes(pose: bool, flat_opacities: bool = False):
    """Case A through `project_gaussians` + the multiply line + `rasterize_gaussians`, and through
    `project_gaussians_antialiased` + `rasterize_gaussians` -> per route (image, leaves, xys, cotangents kept)."""
    from gs_fused import project_gaussians_antialiased
    from rasterizer import project_gaussians, rasterize_gaussians

    n, W, H = CASES["A"]
    raw, cam = _raw(n), _camera_np(W, H)
    bg = torch.tensor(S.BACKGROUND, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(3)
    colors = torch.rand(n, 3, device=DEV, generator=g)
    v_img = torch.rand(H, W, 3, device=DEV, generator=g) * 2 - 1
    Pm = cu(S.projection_matrix(0.001, 1000.0, 2 * np.arctan(W / (2 * cam.fx)),
                                2 * np.arctan(H / (2 * cam.fy))).astype(np.float32))
    res = []
    for route in ("two lines", "one node"):
        leaves = {"means": cu(raw["means"]).requires_grad_(), "scales": cu(np.exp(raw["scales"])).requires_grad_(),
                  "quats": cu(raw["quats"] / np.linalg.norm(raw["quats"], axis=1, keepdims=True)).requires_grad_(),
                  "opacities": torch.sigmoid(cu(raw["opacities"])).detach().requires_grad_()}
        viewmat = cu(cam.viewmat).requires_grad_(pose)
        projmat = Pm @ viewmat if pose else cu(cam.projmat)
        leaves["viewmat"] = viewmat
        args = (leaves["means"], leaves["scales"], 1, leaves["quats"], viewmat[:3, :], projmat, cam.fx, cam.fy, cam.cx,
                cam.cy, H, W, 16)
        opac_in = leaves["opacities"].view(-1) if flat_opacities else leaves["opacities"]
        kept = {}
        if route == "two lines":
            xys, depths, radii, conics, comp, tiles, cov3d = project_gaussians(*args)
            opac = opac_in.view(n, 1) * comp[:, None]
            for nm, t in (("conics", conics), ("comp", comp)):
                t.retain_grad()
                kept[nm] = t
        else:
            xys, depths, radii, conics, opac, tiles, cov3d = project_gaussians_antialiased(*args, opac_in)
            assert opac.shape == opac_in.shape
            opac = opac.view(n, 1)
        xys.retain_grad()
        img = rasterize_gaussians(xys, depths, radii, conics, tiles, colors, opac, H, W, 16, background=bg)
        (img * v_img).sum().backward()
        kept.update(xys=xys, radii=radii, cov3d=cov3d)
        res.append((img.detach(), leaves, kept))
    return raw, cam, res


@pytest.mark.parametrize("flat_opacities", [False, True])
def test_project_gaussians_antialiased_equals_the_two_line_form(flat_opacities):
    _, _, ((img_a, la, ka), (img_b, lb, kb)) = _two_routes(pose=False, flat_opacities=flat_opacities)
    assert torch.equal(img_a, img_b)
    for k in ("means", "scales", "quats", "opacities"):
        a, b = la[k].grad, lb[k].grad
        assert a.abs().max().item() > 0
        assert (a - b).abs().max().item() <= 2e-5 * a.abs().max().item() + 1e-12, k
    assert kb["xys"].grad is not None and kb["xys"].grad.abs().max().item() > 0
    assert (ka["xys"].grad - kb["xys"].grad).abs().max().item() <= 2e-5 * ka["xys"].grad.abs().max().item()
    assert la["viewmat"].grad is None and lb["viewmat"].grad is None


def test_project_gaussians_antialiased_delivers_the_pose_gradient():
    """viewmat [4,4] is the leaf, projmat = P @ viewmat: both matrices' gradients reach it.  The bar is that of
    tests/test_gpu_pose_grad.py: every entry within 1e-3 of its mass (tests/pose_reference.py), the mass taken from
    the float64 pose VJP of the cotangents the two-line form saw."""
    import pose_reference as POSE

    raw, cam, ((img_a, la, ka), (img_b, lb, kb)) = _two_routes(pose=True)
    a, b = la["viewmat"].grad, lb["viewmat"].grad
    assert a is not None and b is not None and b.shape == (4, 4) and float(b.abs().max()) > 0
    n = CASES["A"][0]
    Pm = S.projection_matrix(0.001, 1000.0, 2 * np.arctan(cam.width / (2 * cam.fx)),
                             2 * np.arctan(cam.height / (2 * cam.fy))).astype(np.float64)
    comp = npy(ka["comp"])
    ref = POSE.project_pose_vjp_fp64(
        raw["means"], np.exp(raw["scales"]), 1.0, raw["quats"], cam.viewmat[:3], (Pm @ cam.viewmat).astype(np.float32),
        cam.fx, cam.fy, cam.cx, cam.cy, cam.height, cam.width, comp, npy(ka["radii"]) > 0, npy(ka["xys"].grad),
        None, npy(ka["conics"].grad), npy(ka["comp"].grad))
    mass = np.abs(Pm).T @ ref["mass_projmat"]
    mass[:3] += ref["mass_viewmat"]
    ratio = POSE.mass_ratio(npy(b), npy(a).astype(np.float64), mass)
    print(f"pose gradient, one node vs two lines: {ratio:.2e} of the mass")
    assert ratio <= 1e-3
    for k in ("means", "scales", "quats", "opacities"):
        x, y = la[k].grad, lb[k].grad
        assert (x - y).abs().max().item() <= 2e-5 * x.abs().max().item() + 1e-12, k


@pytest.mark.parametrize("mode,render_depth", [("antialiased", False), ("antialiased", True), ("classic", False)])
def test_render_gaussians_is_bit_reproducible_in_deterministic_mode(mode, render_depth):
    """set_deterministic(True) reaches the one-node view: its compositing backward sums in a fixed order
    (gsr_rasterize_backward_det on the view's lists), so two calls give the same gradient bits, and those stay within
    the 2e-5 of the atomics' gradients that tests/test_gpu_render.py allows between two summation orders (1e-3 for
    the depth image's cotangent, as there)."""
    from gs_fused import DensifyStats, ViewSpec, render_gaussians
    from rasterizer import rasterize as R

    n, W, H = CASES["B"]
    K, deg = 4, 1
    cam = _camera(W, H)
    bg = torch.tensor(S.BACKGROUND, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(2)
    v_img = torch.rand(H, W, 3, device=DEV, generator=g) * 2 - 1
    v_alpha = torch.rand(H, W, device=DEV, generator=g) * 2 - 1
    v_dep = torch.rand(H, W, device=DEV, generator=g) * 2 - 1
    spec = ViewSpec(H, W, cam.fx, cam.fy, cam.cx, cam.cy, deg, render_depth=render_depth, rasterize_mode=mode)

    def run():
        p = _model(n, K)
        stats = DensifyStats(n, DEV, max(W, H))
        out = render_gaussians(p["means"], p["scales"], p["quats"], p["opacities"], p["features_dc"],
                               p["features_rest"], cam.viewmat, cam.projmat, cam.campos, bg, spec, capacity=4_000_000,
                               stats=stats)
        outs, cots = [out["rgb"], out["alpha"]], [v_img, v_alpha]
        if render_depth:
            outs, cots = outs + [out["depth"]], cots + [v_dep]
        torch.autograd.backward(outs, cots)
        return out["rgb"].detach(), {k: t.grad for k, t in p.items()}, stats.as_tuple()

    img0, atomics, stats0 = run()
    R.set_deterministic(True)
    try:
        img1, a, stats1 = run()
        img2, b, stats2 = run()
    finally:
        R.set_deterministic(False)
    assert torch.equal(img0, img1) and torch.equal(img1, img2)
    for k in a:
        assert torch.equal(a[k], b[k]), k
        tol = 1e-3 if render_depth else 2e-5
        assert (a[k] - atomics[k]).abs().max().item() <= tol * atomics[k].abs().max().item() + 1e-12, k
        assert a[k].abs().max().item() > 0
    # the statistics: bit-identical between the two deterministic calls; against the atomics' the counts and sizes
    # are equal, and the gradient norm -- of two components, each within 2e-5 of the largest -- within 4e-5 of it
    for y, z in zip(stats1, stats2):
        assert torch.equal(y, z)
    assert torch.equal(stats0[1], stats1[1]) and torch.equal(stats0[2], stats1[2])
    assert (stats0[0] - stats1[0]).abs().max().item() <= 4e-5 * stats0[0].abs().max().item()


# ---- the trainer ---------------------------------------------------------------------------------------------
SMALL = dict(num_gaussians=20_000, width=320, height=180, num_views=8, iters=30, sh_degree=3, sh_degree_interval=30,
             log_every=1)  # the size of SMALL in tests/test_gpu_pose_opt.py, 30 steps
BODIES = {"separate": {}, "fused_render": dict(fused_render=True), "use_graph": dict(fused_render=True, use_graph=True)}
RENDER = {"separate": "separate ops", "fused_render": "one fused op", "use_graph": "hip graph per view"}
_runs = {}


def _train(body, mode, again=False):
    """One 30-step run under set_deterministic(True), kept for the tests that share it (`again`: a second run)."""
    from harness.train import TrainConfig, train
    from rasterizer import rasterize as R

    key = (body, mode, again)
    if key not in _runs:
        R.set_deterministic(True)
        try:
            _runs[key] = train(TrainConfig(rasterize_mode=mode, **BODIES[body], **SMALL), torch.device("cuda", 0))
        finally:
            R.set_deterministic(False)
    return _runs[key]


@pytest.mark.parametrize("body", list(BODIES))
def test_trainer_antialiased_is_reproducible_and_differs_from_classic(body):
    """Under set_deterministic(True) two 30-step runs of one body give the same losses and parameters to the bit --
    the one-node view and its graph included: their compositing backward then sums in a fixed order
    (gs_fused/render.py) -- and differ from the classic run from the first loss on."""
    a, b = _train(body, "antialiased"), _train(body, "antialiased", again=True)
    assert a["render"] == RENDER[body] and a["rasterize_mode"] == "antialiased" and len(a["losses"]) == 30
    c = _train(body, "classic")
    assert "rasterize_mode" not in c
    assert a["losses"][0] != c["losses"][0] and a["losses"][1] != c["losses"][1]
    assert a["psnr_start"] != c["psnr_start"]  # (`evaluate` renders in the mode too)
    worst = max(abs(x - y) for x, y in zip(a["losses"], b["losses"]))
    print(f"{body}: two runs, worst loss difference {worst:.3e}, checksums {a['param_checksum']!r} {b['param_checksum']!r}")
    assert a["losses"] == b["losses"] and a["param_checksum"] == b["param_checksum"]


def test_trainer_bodies_agree_in_antialiased_mode_as_in_classic():
    """The worst difference between two bodies' losses over the 30 steps, antialiased against classic.  Every run is
    under set_deterministic(True), so each figure is a fixed number: antialiased may not exceed classic's, or one
    spacing of float32 at the largest loss where classic's is smaller still (a loss is a float32; two summation
    orders of the same terms cannot be asked to agree beyond its last bit)."""
    spread = {}
    for mode in ("classic", "antialiased"):
        runs = [_train(body, mode)["losses"] for body in BODIES]
        spread[mode] = max(abs(x - y) for i in range(3) for j in range(i) for x, y in zip(runs[i], runs[j]))
    ulp = float(np.spacing(np.float32(max(_train("separate", "classic")["losses"]))))
    print("worst loss difference between bodies:", spread, "float32 spacing at the largest loss:", ulp)
    assert spread["antialiased"] <= max(spread["classic"], ulp), (spread, ulp)


# ---- export ----------------------------------------------------------------------------------------------------
def test_fuse_views_antialiased():
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from export_tsdf import activated

    from gs_fusion import TSDFVolume, fuse_views, view_depth
    from harness.pipeline import CameraTensors, render_view
    from harness.train import orbit_cameras

    n, W, H = CASES["A"]
    params = activated(_raw(n), torch.device(DEV))
    cams = orbit_cameras(8, W, H)[::2]
    assert len(cams) == 4
    bg = torch.zeros(3, device=DEV)
    volume = lambda: TSDFVolume.from_bounds([-2.0] * 3, [2.0] * 3, 4.0 / 64, 0.25, None, DEV)  # noqa: E731
    va, vb, vc = volume(), volume(), volume()
    fuse_views(va, params, cams, bg, 3, alpha_min=0.5, rasterize_mode="antialiased")
    with torch.no_grad():
        for cam in cams:
            out = render_view(params["means3d"], params["scales"], params["quats"], params["opacities"],
                              params["sh_coeffs"], CameraTensors.from_numpy(cam, DEV), bg, 3,
                              rasterize_mode="antialiased", render_depth=True, fused_depth=True, normalise_depth=False)
            depth, valid = view_depth(out["depth_acc"], out["alpha"], 0.5)
            vb.integrate(depth, out["rgb"].contiguous(), cam.fx, cam.fy, cam.cx, cam.cy, cam.viewmat, valid=valid)
    fuse_views(vc, params, cams, bg, 3, alpha_min=0.5)
    a, b, c = va.state_dict(), vb.state_dict(), vc.state_dict()
    assert a["num_allocated"] == b["num_allocated"] > 0
    for k in ("table", "tsdf", "weight", "color"):
        assert torch.equal(a[k], b[k]), k
    occ_a, occ_c = int((a["weight"] > 0).sum()), int((c["weight"] > 0).sum())
    print(f"occupied voxels: antialiased {occ_a}, classic {occ_c}")
    assert occ_c > 0 and not (torch.equal(a["table"], c["table"]) and torch.equal(a["weight"] > 0, c["weight"] > 0))
    with pytest.raises(ValueError, match="Unknown rasterize_mode"):
        fuse_views(vc, params, cams, bg, 3, rasterize_mode="smooth")


def test_inria_facade_honours_antialiasing():
    from rasterizer.inria import GaussianRasterizationSettings, GaussianRasterizer

    n, W, H = CASES["A"]
    raw, cam = _raw(n), _camera_np(W, H)
    bg = torch.tensor(S.BACKGROUND, device=DEV)
    campos = cu((-cam.viewmat[:3, :3].T @ cam.viewmat[:3, 3]).astype(np.float32))
    base = (H, W, W / (2 * cam.fx), H / (2 * cam.fy), bg, 1.0, cu(cam.viewmat).t().contiguous(),
            cu(cam.projmat).t().contiguous(), 3, campos)
    shs = cu(np.concatenate([raw["features_dc"][:, None, :], raw["features_rest"]], 1))
    kw = dict(means3D=cu(raw["means"]), means2D=None, opacities=torch.sigmoid(cu(raw["opacities"])), shs=shs,
              scales=cu(np.exp(raw["scales"])), rotations=cu(raw["quats"]))
    with torch.no_grad():
        classic = GaussianRasterizer(GaussianRasterizationSettings(*base, False, False))(**kw)[0]
        aa = GaussianRasterizer(GaussianRasterizationSettings(*base, antialiasing=True))(**kw)[0]
        # the two-line form on what the façade itself hands to the projection
        from rasterizer import project_gaussians, rasterize_gaussians, spherical_harmonics

        quats = kw["rotations"] / kw["rotations"].norm(dim=-1, keepdim=True)
        xys, depths, radii, conics, comp, tiles, _ = project_gaussians(
            kw["means3D"], kw["scales"], 1.0, quats, cu(cam.viewmat[:3]), cu(cam.projmat), W / (2.0 * base[2]),
            H / (2.0 * base[3]), W / 2.0, H / 2.0, H, W, 16, 0.01)
        dirs = kw["means3D"] - campos
        colors = torch.clamp_min(spherical_harmonics(3, dirs / dirs.norm(dim=-1, keepdim=True), shs) + 0.5, 0.0)
        ref = rasterize_gaussians(xys, depths, radii, conics, tiles, colors, kw["opacities"] * comp[:, None], H, W, 16,
                                  background=bg)
    assert float((classic - aa).abs().max()) > 0.1
    assert torch.equal(aa.permute(1, 2, 0), ref)


# ---- unchanged models: lists built ahead of time in antialiased mode ---------------------------------------------
def _model_sequence(stale_at=None, near_miss_at=None):
    """Five views of the UNCHANGED models' antialiased pattern, with their two read-backs (`render_view(
    caller_syncs=True)`, written out so that something can happen between projection and rasterization):
    project_gaussians -> `radii.sum() == 0` -> `(num_tiles_hit > 0).any()` -> `torch.sigmoid(leaf) * comp[:, None]`
    -> rasterize_gaussians.  `stale_at`: in that view the leaf is written in place (x 1.0: a new version, the same
    values) behind the projection.  `near_miss_at`: in that view the opacity is `torch.sigmoid(leaf) * comp[:1][:, None]`
    -- ONE element of the compensation, broadcast: the graph of the recipe but for a slice, other values.
    -> per view (image, v_means, v_logits)."""
    from rasterizer import project_gaussians, rasterize_gaussians

    n, W, H = 100_000, 320, 176
    raw = _raw(n)
    g = torch.Generator(device=DEV).manual_seed(5)
    colors = torch.rand(n, 3, device=DEV, generator=g)
    v_img = torch.rand(H, W, 3, device=DEV, generator=g) * 2 - 1
    means, logits = cu(raw["means"]).requires_grad_(), cu(raw["opacities"]).requires_grad_()
    scales = cu(np.exp(raw["scales"]))
    quats = cu(raw["quats"] / np.linalg.norm(raw["quats"], axis=1, keepdims=True))
    bg = torch.tensor(S.BACKGROUND, device=DEV)
    views = []
    for v in range(5):
        cam = _camera(W, H, v)
        xys, depths, radii, conics, comp, tiles, _ = project_gaussians(
            means, scales, 1, quats, cam.viewmat[:3, :], cam.projmat, cam.fx, cam.fy, cam.cx, cam.cy, H, W, 16)
        assert radii.sum() != 0
        assert (tiles > 0).any()
        if v == stale_at:
            with torch.no_grad():
                logits.mul_(1.0)
        opac = torch.sigmoid(logits) * (comp[:1][:, None] if v == near_miss_at else comp[:, None])
        img = rasterize_gaussians(xys, depths, radii, conics, tiles, colors, opac, H, W, 16, background=bg)
        gm, gl = torch.autograd.grad((img * v_img).sum(), (means, logits))
        views.append((img.detach(), gm, gl))
    torch.cuda.synchronize()
    return views


@functools.lru_cache(maxsize=None)
def _ahead_runs(deterministic):
    """The sequence three times -- speculated, speculated with a stale leaf in view 4, and with the tuning row
    `no_speculation` set -- and the rasterizer's counters in between; `deterministic`: all of it under
    set_deterministic(True), where the lists built ahead come with the maps the fixed-order backward reduces along.
    The mode is "lists" (build ahead whenever the opacities are predictable), as in the fuzz of tests/test_gpu_api.py:
    under "auto" the side stream is switched on by an observation of the caller's stream that five views do not
    settle."""
    from rasterizer import ahead as A
    from rasterizer import rasterize as R
    from rasterizer.cuda import _tuning

    R._speculation_mode()
    saved, saved_rows = R._spec_knobs["mode"], _tuning.overrides()
    R._spec_knobs["mode"] = "lists"
    st = A._spec.get(torch.device(DEV))
    if st is not None:
        st["recipes_off"], st["unknown_run"] = False, 0
    R.set_deterministic(deterministic)
    try:
        c0 = dict(R.counters)
        on = _model_sequence()
        c1 = dict(R.counters)
        stale = _model_sequence(stale_at=3)
        c2 = dict(R.counters)
        recipe = A._spec[torch.device(DEV)]["recipe"]
        _model_sequence()  # (restores the recipe)
        c4 = dict(R.counters)
        near = _model_sequence(near_miss_at=1)
        c5 = dict(R.counters)
        _tuning.set_overrides(dict(saved_rows, no_speculation=1))
        off = _model_sequence()
        c3 = dict(R.counters)
        off_near = _model_sequence(near_miss_at=1)
    finally:
        R.set_deterministic(False)
        R._spec_knobs["mode"] = saved
        _tuning.set_overrides(saved_rows)
        A._spec[torch.device(DEV)]["unknown_run"] = 0  # (the near miss counted as an unknown producer)
    return (c0, c1, c2, c5, c3), recipe, on, stale, off, (c4, c5, near, off_near)


@pytest.mark.parametrize("deterministic", [False, True])
def test_lists_are_built_ahead_for_the_unchanged_models_antialiased_line(deterministic):
    """`rasterizer/ahead.py` recognises `unary(leaf) * comp[:, None]` with the compensation of the projection that
    queued the lists: they are built on the side stream from the second view on and USED (`ahead_hits`), the images
    are those of the same sequence without speculation, bit for bit, and a leaf written in place between projection
    and rasterization drops the entry (`ahead_misses`) without changing them."""
    (c0, c1, c2, c2b, c3), recipe, on, stale, off, near_miss = _ahead_runs(deterministic)
    d = lambda a, b, k: b[k] - a[k]  # noqa: E731
    print("hits / builds ahead / misses:", [(d(a, b, "ahead_hits"), d(a, b, "list_builds_ahead"), d(a, b, "ahead_misses"))
                                            for a, b in ((c0, c1), (c1, c2), (c2b, c3))])
    assert recipe is not None and recipe[0] == "product" and recipe[1] == "SigmoidBackward0", recipe
    assert d(c0, c1, "ahead_hits") >= 3 and d(c0, c1, "ahead_misses") == 0  # views 2 to 5
    assert d(c1, c2, "ahead_misses") >= 1 and d(c1, c2, "ahead_hits") >= 2  # the stale entry was dropped
    assert d(c2b, c3, "ahead_hits") == 0 and d(c2b, c3, "list_builds_ahead") == 0
    assert c3["ahead_recipes_off"] == c0["ahead_recipes_off"]
    # a near miss: the recipe's graph but for a one-element slice of the compensation, which broadcasts.  The lists
    # queued for view 2 were built from the full product: dropped, not used, and the sequence is the unspeculated one
    c4, c5, near, off_near = near_miss
    print("near miss: hits / builds ahead / misses:", d(c4, c5, "ahead_hits"), d(c4, c5, "list_builds_ahead"),
          d(c4, c5, "ahead_misses"))
    assert d(c4, c5, "list_builds_ahead") >= 1 and d(c4, c5, "ahead_misses") >= 1
    assert d(c4, c5, "ahead_hits") <= 2  # view 2 is dropped, view 3 has no recipe to go by: at most views 4 and 5
    assert not torch.equal(near[1][0], on[1][0])  # (other opacities: another image)
    for v, (a, b) in enumerate(zip(near, off_near)):
        assert torch.equal(a[0], b[0]), ("near miss", v)
        for x, y in zip(a[1:], b[1:]):
            assert (x - y).abs().max() <= 1e-5 * y.abs().max(), ("near miss", v)
    for what, seq in (("speculated", on), ("stale entry", stale)):
        for v, (a, b) in enumerate(zip(seq, off)):
            assert torch.equal(a[0], b[0]), (what, v)
            for x, y in zip(a[1:], b[1:]):  # (the bar tests/test_gpu_api.py holds such gradients to)
                assert (x - y).abs().max() <= 1e-5 * y.abs().max(), (what, v)


def test_gradients_behind_lists_built_ahead_equal_the_unspeculated_ones_bit_for_bit():
    """The same three sequences, gradients `torch.equal`: under set_deterministic(True), the one mode in which a
    gradient's bits are defined at all -- with float atomics two runs of the SAME sequence differ (measured: v_means
    by up to 5.7e-06 in a view where neither leg used lists built ahead)."""
    _, _, on, stale, off, _ = _ahead_runs(True)
    worst = [max(float((x - y).abs().max()) for seq in (on, stale) for a, b in zip(seq, off) for x, y in ((a[k], b[k]),))
             for k in (1, 2)]
    print("v_means / v_logits, worst difference over the ten views:", worst)
    for what, seq in (("speculated", on), ("stale entry", stale)):
        for v, (a, b) in enumerate(zip(seq, off)):
            assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), (what, v, worst)


def test_the_default_mode_builds_ahead_for_the_antialiased_line():
    """The same five views under the DEFAULT mode ("auto"), where the side stream is on only while the caller is seen
    to block.  This caller blocks twice per view -- and has its own multiply in flight when `rasterize_gaussians` is
    entered, so its stream is not idle there; the observation for the product recipe is the projection's event
    (rasterizer/ahead.py), which every view's read-backs have long passed: the average stays above 1/2 and views 3 to
    5 at the least are built ahead and used."""
    from rasterizer import ahead as A
    from rasterizer import rasterize as R

    R._speculation_mode()
    saved = R._spec_knobs["mode"]
    R._spec_knobs["mode"] = "auto"
    st = A._spec.setdefault(torch.device(DEV), {"stream": None, "recipe": None, "entry": None})
    st["recipes_off"], st["unknown_run"], st["idle"] = False, 0, 1.0
    try:
        c0 = dict(R.counters)
        seq = _model_sequence()
        c1 = dict(R.counters)
    finally:
        R._spec_knobs["mode"] = saved
    hits, idle = c1["ahead_hits"] - c0["ahead_hits"], A._spec[torch.device(DEV)]["idle"]
    print(f"auto: {hits} hits in 5 views, idle average {idle:.3f}")
    assert A._spec[torch.device(DEV)].get("projected") is not None
    assert hits >= 3 and idle > 0.5
    assert all(torch.isfinite(img).all() for img, _, _ in seq)
