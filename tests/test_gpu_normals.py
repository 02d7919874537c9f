"""GPU: csrc/normals.hip behind gs_fused.gaussian_normals / depth_to_normal / normal_consistency_loss against the
float64 restatement tests/_normals_ref.py (pinned by tests/test_normals_host.py).

The error measure is e(X) = max |X - X64| / max |X64|.  Per case the same restatement is run in float32 on the CPU, and
the kernel must stay within 4 x that error + 2^-23: the factor 4 allows another association of the cross-product and dot
sums, the 2^-23 one ulp of the normaliser.  Every figure is printed before it is asserted."""
import functools

import pytest
import torch

import _normals_ref as R

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
IMAGES = [(1, 1), (2, 2), (3, 3), (5, 7), (17, 33), (64, 64), (270, 480)]


def bound(e32):
    return 4.0 * e32 + ULP


def held(name, got, want, e32):
    e = R.rel_err(got.cpu(), want)
    print(f"  {name}: e {e:.3g} (float32 restatement {e32:.3g}, bound {bound(e32):.3g})")
    assert e <= bound(e32), name


@functools.lru_cache(maxsize=None)
def gaussians(n):
    case, rounds = R.gaussian_case(n, 200 + n)
    return case, R.gaussian_reference(case, 201 + n), rounds


@functools.lru_cache(maxsize=None)
def image(H, W, masked):
    case = R.image_case(H, W, 100 + H, masked)
    return case, R.image_reference(case)


def dev():
    return torch.device("cuda", 0)


# ---- per-Gaussian normals --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_gaussian_normals_follow_the_restatement(n):
    from gs_fused import gaussian_normals

    case, want, rounds = gaussians(n)
    print(f"N={n}: inputs drawn in {rounds} round(s), {int(case['tied'].sum())} tied rows")
    assert rounds < 64
    norms = case["quats"].double().norm(dim=-1)
    assert float(norms.min()) >= 0.999e-3 and float(norms.max()) <= 1.001e3
    d = dev()
    q = case["quats"].to(d).requires_grad_(True)
    normals, axis = gaussian_normals(q, case["scales"].to(d), case["means"].to(d), case["viewmat"].to(d), return_axis=True)
    assert normals.shape == (n, 3) and axis.shape == (n,) and axis.dtype == torch.int32
    assert torch.equal(axis.cpu().long(), want["axis"])
    (normals * want["v_normals"].to(d)).sum().backward()
    held("normals", normals.detach(), want["normals"], want["e32"]["normals"])
    held("v_quats", q.grad, want["v_quats"], want["e32"]["v_quats"])
    # only the order of the scales is used: exp of the given scales gives the same bits; a second run too
    again = gaussian_normals(case["quats"].to(d), case["scales"].to(d).exp(), case["means"].to(d), case["viewmat"].to(d))
    assert torch.equal(again, normals.detach())
    assert not case["scales"].requires_grad and q.grad.shape == (n, 4)


def test_gaussian_normals_of_no_gaussians():
    from gs_fused import gaussian_normals

    d = dev()
    out = gaussian_normals(torch.zeros(0, 4, device=d), torch.zeros(0, 3, device=d), torch.zeros(0, 3, device=d),
                           torch.eye(4, device=d))
    assert out.shape == (0, 3)


# ---- depth normals and the loss --------------------------------------------------------------------------------------
def run_image(case, mask):
    """-> normals, loss, v_nimg, v_depth on the device, upstream 1."""
    from gs_fused import depth_to_normal, normal_consistency_loss

    d = dev()
    depth, alpha = case["depth"].to(d), case["alpha"].to(d)
    nimg = case["nimg"].to(d).requires_grad_(True)
    dd = depth.clone().requires_grad_(True)
    normals = depth_to_normal(depth, alpha, *case["K"])
    loss = normal_consistency_loss(nimg, dd, alpha, *case["K"], mask=None if mask is None else mask.to(d))
    loss.backward()
    return normals, loss.detach(), nimg.grad, dd.grad


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("H,W", IMAGES, ids=[f"{h}x{w}" for h, w in IMAGES])
def test_depth_normals_and_loss_follow_the_restatement(H, W, masked):
    case, want = image(H, W, masked)
    valid, near = want["valid"], want["near_valid"]
    print(f"{H}x{W} mask={masked}: {int(valid.sum())} of {H * W} pixels valid")
    if H * W >= 35:  # every validity branch occurs: border, a hole of its own, a neighbour's hole, valid
        a0 = case["alpha"] <= 0
        interior = torch.zeros_like(valid)
        interior[1:-1, 1:-1] = True
        assert bool(valid.any()) and bool((interior & a0).any()) and bool((interior & ~a0 & ~valid).any())
        assert bool((~near).any()) and bool((near & ~valid).any())
    # (a large scratch allocation filled with NaN and released: what torch.empty hands out next is not zeros)
    scratch = torch.full(((64 << 20) // 4,), float("nan"), device=dev())
    del scratch
    normals, loss, v_nimg, v_depth = run_image(case, case["mask"])
    assert normals.shape == (H, W, 3) and v_nimg.shape == (H, W, 3) and v_depth.shape == (H, W) and loss.shape == ()
    e = want["e32"]
    held("normals", normals, want["normals"], e["normals"])
    held("loss", loss.reshape(1), want["loss"], e["loss"])
    held("v_nimg", v_nimg, want["v_nimg"], e["v_nimg"])
    held("v_depth", v_depth, want["v_depth"], e["v_depth"])
    # exact: zeros at every invalid pixel of the map, zeros of v_depth where no neighbour is valid
    assert bool((normals.cpu()[~valid] == 0).all()) and bool((normals.cpu()[valid].abs().sum(-1) > 0).all())
    assert bool((v_depth.cpu()[~near] == 0).all())
    if H < 3 or W < 3:  # all border: exact zeros, and the loss is exactly mean(m)
        assert not bool(normals.any()) and not bool(v_depth.any()) and not bool(v_nimg.any())
        m = torch.ones(H, W) if case["mask"] is None else case["mask"]
        assert float(loss) == float(m.double().mean().float())
    # two runs are bit-equal
    again = run_image(case, case["mask"])
    for a, b in zip(again, (normals, loss, v_nimg, v_depth)):
        assert torch.equal(a, b)
    if not masked:  # an all-ones mask is bit-equal to no mask; [H,W,1] and bool masks are taken
        for ones in (torch.ones(H, W), torch.ones(H, W, 1, dtype=torch.bool)):
            for a, b in zip(run_image(case, ones), (normals, loss, v_nimg, v_depth)):
                assert torch.equal(a, b)


def test_upstream_scales_the_gradients_and_depth_keeps_its_shape():
    from gs_fused import normal_consistency_loss

    case, want = image(17, 33, True)
    d = dev()
    nimg = case["nimg"].to(d).requires_grad_(True)
    depth = case["depth"].to(d)[..., None].clone().requires_grad_(True)  # [H,W,1], as the render returns it
    loss = normal_consistency_loss(nimg, depth, case["alpha"].to(d)[..., None], *case["K"], mask=case["mask"].to(d))
    (0.25 * loss).backward()
    assert depth.grad.shape == (17, 33, 1)
    held("v_depth / 4", depth.grad[..., 0], 0.25 * want["v_depth"], want["e32"]["v_depth"])
    held("v_nimg / 4", nimg.grad, 0.25 * want["v_nimg"], want["e32"]["v_nimg"])


# ---- one flat Gaussian through the render route ----------------------------------------------------------------------
def flat_gaussian(quat):
    from harness import scene as S
    from harness.pipeline import CameraTensors, render_view

    d = dev()
    cam = CameraTensors.from_numpy(S.make_camera(48, 40), d)  # at the origin, looking down +z
    t = lambda v: torch.tensor(v, dtype=torch.float32, device=d)  # noqa: E731
    quats = t([quat]).requires_grad_(True)
    out = render_view(t([[0.0, 0.0, 3.0]]), t([[1.0, 1.0, 0.01]]), quats, t([[0.95]]), t([[[0.5, 0.2, -0.1]]]), cam,
                      t([0.1, 0.2, 0.3]), 0, render_depth=True, render_normals=True)
    return cam, quats, out


def test_one_flat_gaussian_facing_the_camera():
    from gs_fused import depth_to_normal, normal_consistency_loss

    cam, quats, out = flat_gaussian([1.0, 0.0, 0.0, 0.0])
    assert out["normals"].shape == (40, 48, 3)
    alpha = out["alpha"][..., 0]
    solid = alpha > 0.5
    assert int(solid.sum()) > 100
    facing = torch.tensor([0.0, 0.0, -1.0], device=alpha.device)
    err = ((out["normals"] / out["alpha"]).detach()[solid] - facing).abs().max()
    n_d = depth_to_normal(out["depth"], out["alpha"], cam.fx, cam.fy, cam.cx, cam.cy)
    valid = solid & (n_d.abs().sum(-1) > 0)
    err_d = (n_d[valid] - facing).abs().max()
    print(f"normals / alpha: {float(err):.3g} from (0,0,-1) on {int(solid.sum())} pixels; depth normals: "
          f"{float(err_d):.3g} on {int(valid.sum())}")
    assert int(valid.sum()) > 100 and float(err) < 1e-3 and float(err_d) < 1e-3
    loss = normal_consistency_loss(out["normals"], out["depth"], out["alpha"], cam.fx, cam.fy, cam.cx, cam.cy)
    loss.backward()
    assert quats.grad is not None and bool(torch.isfinite(quats.grad).all())
    # tilted by 0.2 rad about x the rendered normals leave the depth's: the gradient that reaches quats is not zero
    _, q2, out2 = flat_gaussian([0.995004, 0.099833, 0.0, 0.0])
    normal_consistency_loss(out2["normals"], out2["depth"], out2["alpha"], cam.fx, cam.fy, cam.cx, cam.cy).backward()
    print(f"|v_quats| aligned {float(quats.grad.abs().max()):.3g}, tilted {float(q2.grad.abs().max()):.3g}")
    assert bool(torch.isfinite(q2.grad).all()) and float(q2.grad.abs().max()) > 1e-4


def test_the_default_render_has_no_normals_key():
    from harness import scene as S
    from harness.pipeline import CameraTensors, render_view

    d = dev()
    cam = CameraTensors.from_numpy(S.make_camera(48, 40), d)
    t = lambda v: torch.tensor(v, dtype=torch.float32, device=d)  # noqa: E731
    args = (t([[0.0, 0.0, 3.0]]), t([[1.0, 1.0, 0.01]]), t([[1.0, 0.0, 0.0, 0.0]]), t([[0.95]]), t([[[0.5, 0.2, -0.1]]]),
            cam, t([0.1, 0.2, 0.3]), 0)
    keys = {"rgb", "alpha", "depth", "depth_acc", "xys", "radii", "depths", "conics", "num_tiles_hit", "rgbs"}
    assert set(render_view(*args)) == keys
    assert set(render_view(*args, render_depth=True)) == keys
    assert set(render_view(*args, render_normals=True)) == keys  # (without a depth image there is no normal pass)
    assert set(render_view(*args, render_depth=True, fused_depth=True, render_normals=True)) == keys | {"normals"}
