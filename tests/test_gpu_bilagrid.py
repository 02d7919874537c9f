"""GPU: the bilateral-grid kernels (gs_fused.bilagrid_slice, bilagrid_tv_loss, BilateralGrids; csrc/bilagrid.hip)
against the float64 CPU restatement of tests/_bilagrid_ref.py (torch's own grid_sample + the affine map).

The error measure, for the output and both gradients alike: e(X) = max |X - X64| / max |X64|.  The tolerance is not a
constant: per case the SAME restatement is run in float32 on the CPU, and the kernel must stay within
4 x that error + 2^-23 (4: another association of the 8-corner and 4-term sums; 2^-23: one float32 ulp of the
normaliser).  Inputs: rgb uniform in [-0.3, 1.4], so both border clamps of the guide occur; a pixel whose guide lies
within 1e-3 of a level or of 0 or 1 is drawn again (the guide's gradient jumps there) -- a condition on the inputs, no
pixel is left out of any comparison.  Every figure is printed before it is asserted (run with -s)."""
import pytest
import torch

import _bilagrid_ref as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMAGES = [(1, 1), (5, 7), (37, 53), (64, 64), (270, 480)]
GRIDS = [(2, 2, 2), (3, 2, 5), (16, 16, 8), (64, 64, 16)]   # (Gw, Gh, L)
VIEWS = [0, 1, 2]                                            # first, middle, last of V = 3


def _run(grids, rgb, view, v_out):
    """-> (out, v_rgb, v_grids) of the HIP ops, on the device."""
    from gs_fused import bilagrid_slice

    a = grids.to(DEV).requires_grad_(True)
    x = rgb.to(DEV).requires_grad_(True)
    out = bilagrid_slice(a, x, view)
    assert out.shape == x.shape and out.dtype == torch.float32 and out.is_cuda
    out.backward(v_out.to(DEV))
    assert a.grad.shape == a.shape and x.grad.shape == x.shape
    return out.detach(), x.grad, a.grad


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "g%dx%dx%d" % g)
@pytest.mark.parametrize("image", IMAGES, ids=lambda s: "%dx%d" % s)
def test_slice_against_float64(image, grid, view):
    (H, W), (gw, gh, gl) = image, grid
    (grids, rgb, v_out), want, base = B.slice_case(H, W, gw, gh, gl, view)
    if H * W >= 3:  # (the inputs are drawn so: both clamps and the interior of the guide)
        g = B.guide64(rgb)
        assert bool((g < 0).any()) and bool((g > 1).any()) and bool(((g > 0) & (g < 1)).any())
    got = _run(grids, rgb, view, v_out)
    fails = []
    for name, x, w, b in zip(("out", "v_rgb", "v_grids"), got, want, base):
        e, e32 = B.rel_err(x, w), B.rel_err(b, w)
        bound = 4.0 * e32 + B.ULP
        print(f"{H}x{W} grid {gw}x{gh}x{gl} view {view} {name}: e = {e:.3e}, float32 restatement {e32:.3e}, bound {bound:.3e}")
        assert bool(torch.isfinite(x).all())
        if not e <= bound:
            fails.append((name, e, bound))
    assert not fails, fails
    # the grids of the two views not sliced get exact zeros
    for v in range(3):
        if v != view:
            assert int(torch.count_nonzero(got[2][v])) == 0


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "g%dx%dx%d" % g)
@pytest.mark.parametrize("image", IMAGES, ids=lambda s: "%dx%d" % s)
def test_identity_grids_return_the_image(image, grid):
    from gs_fused import bilagrid_slice

    (H, W), (gw, gh, gl) = image, grid
    rgb = B.draw_rgb(H, W, gl, torch.Generator().manual_seed(17 * H + W)).to(DEV)
    out = bilagrid_slice(B.identity_grids(3, gw, gh, gl).to(DEV), rgb, 1)
    e = float((out - rgb).abs().max()) / float(rgb.abs().max())
    print(f"{H}x{W} grid {gw}x{gh}x{gl}: identity e = {e:.3e}")
    assert e <= 2.0 ** -22


def test_vertices_of_empty_cells_are_exactly_zero():
    """5x7 under a 16x16x8 grid: most cells hold no pixel.  A vertex gets a gradient only from the pixels whose cell it
    is a corner of, at the two levels around the pixel's guide; every other vertex must be an exact zero (not workspace
    garbage), whatever the workspace held."""
    H, W, gw, gh, gl, view = 5, 7, 16, 16, 8, 1
    (grids, rgb, v_out), want, _ = B.slice_case(H, W, gw, gh, gl, view)
    torch.empty(1 << 22, dtype=torch.float64, device=DEV).fill_(float("nan"))  # (what a fresh workspace may hold)
    got = _run(grids, rgb, view, v_out)[2]
    reached = torch.zeros((gl, gh, gw), dtype=torch.bool)
    g = B.guide64(rgb).clamp(0, 1)
    for py in range(H):
        for px in range(W):
            ix, iy, iz = (px + 0.5) / W * (gw - 1), (py + 0.5) / H * (gh - 1), float(g[py, px]) * (gl - 1)
            x0, y0, z0 = min(int(ix), gw - 2), min(int(iy), gh - 2), min(int(iz), gl - 2)
            reached[z0:z0 + 2, y0:y0 + 2, x0:x0 + 2] = True
    assert 0 < int(reached.sum()) < reached.numel() // 4
    assert int(torch.count_nonzero(got[view].cpu()[~reached])) == 0
    assert int(torch.count_nonzero(want[2][view][~reached])) == 0  # (the restatement agrees on which)
    assert bool((got[view].cpu()[reached].abs().amax(-1) > 0).any())


@pytest.mark.parametrize("image", [(37, 53), (270, 480)], ids=lambda s: "%dx%d" % s)
def test_two_runs_are_bit_equal(image):
    (grids, rgb, v_out), _, _ = B.slice_case(image[0], image[1], 16, 16, 8, 2)
    first = _run(grids, rgb, 2, v_out)
    torch.empty(1 << 22, dtype=torch.float64, device=DEV).normal_()  # (another workspace content for the second run)
    second = _run(grids, rgb, 2, v_out)
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_non_contiguous_inputs():
    """The ops take what autograd hands them: a non-contiguous rgb (a permuted render) and a non-contiguous cotangent."""
    from gs_fused import bilagrid_slice

    (grids, rgb, v_out), want, base = B.slice_case(37, 53, 3, 2, 5, 1)
    a = grids.to(DEV).requires_grad_(True)
    x = rgb.to(DEV).permute(2, 0, 1).contiguous().permute(1, 2, 0).requires_grad_(True)
    assert not x.is_contiguous()
    out = bilagrid_slice(a, x, 1)
    out.backward(v_out.to(DEV).permute(1, 0, 2).contiguous().permute(1, 0, 2))
    for x_, w, b in zip((out.detach(), x.grad, a.grad), want, base):
        assert B.rel_err(x_, w) <= 4.0 * B.rel_err(b, w) + B.ULP


def test_wrong_dtype_and_device_raise():
    from gs_fused import bilagrid_slice, bilagrid_tv_loss

    grids, rgb = B.identity_grids(3, 4, 3, 2).to(DEV), torch.zeros(5, 7, 3, device=DEV)
    with pytest.raises(RuntimeError, match="grids"):
        bilagrid_slice(grids.double(), rgb, 0)
    with pytest.raises(RuntimeError, match="rgb"):
        bilagrid_slice(grids, rgb.half(), 0)
    with pytest.raises(RuntimeError, match="rgb"):
        bilagrid_slice(grids, rgb.cpu(), 0)
    with pytest.raises(RuntimeError, match="grids"):
        bilagrid_tv_loss(grids.double())
    with pytest.raises(ValueError, match="view"):
        bilagrid_slice(grids, rgb, 3)


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "g%dx%dx%d" % g)
@pytest.mark.parametrize("V", [1, 3])
def test_tv_against_float64(V, grid):
    from gs_fused import bilagrid_tv_loss

    gw, gh, gl = grid
    gen = torch.Generator().manual_seed(101 * gw + 11 * gh + gl + V)
    grids = B.identity_grids(V, gw, gh, gl) + 0.25 * torch.randn((V, gl, gh, gw, 12), generator=gen)
    res = []
    for dt in (torch.float64, torch.float32):
        a = grids.to(dt).clone().requires_grad_(True)
        t = B.tv_ref(a)
        (-1.5 * t).backward()
        res.append((t.detach().reshape(1), a.grad))
    runs = []
    for _ in range(2):
        a = grids.to(DEV).requires_grad_(True)
        t = bilagrid_tv_loss(a)
        assert t.dtype == torch.float32 and t.dim() == 0 and t.is_cuda
        (-1.5 * t).backward()
        runs.append((t.detach().reshape(1), a.grad))
    fails = []
    for name, x, w, b in zip(("tv", "v_grids"), runs[0], res[0], res[1]):
        e, e32 = B.rel_err(x, w), B.rel_err(b, w)
        print(f"V {V} grid {gw}x{gh}x{gl} {name}: e = {e:.3e}, float32 restatement {e32:.3e}, bound {4 * e32 + B.ULP:.3e}")
        if not e <= 4.0 * e32 + B.ULP:
            fails.append((name, e, 4.0 * e32 + B.ULP))
    assert not fails, fails
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert float(bilagrid_tv_loss(B.identity_grids(V, gw, gh, gl).to(DEV))) == 0.0


def test_module_step_equals_torch_adam():
    """BilateralGrids under gs_fused.FusedAdam (the existing kernel, a new caller): one step from the gradient of
    slice + TV equals torch.optim.Adam on the same gradient, to float32 rounding of the update."""
    from gs_fused import BilateralGrids, FusedAdam

    (_, rgb, v_out), _, _ = B.slice_case(37, 53, 16, 16, 8, 1)
    m = BilateralGrids(3, 16, 16, 8, device=DEV)
    assert m.grids.is_cuda and torch.equal(m.grids.detach().cpu(), B.identity_grids(3, 16, 16, 8))
    with torch.no_grad():
        m.grids.add_(0.05 * torch.randn(m.grids.shape, generator=torch.Generator().manual_seed(1)).to(DEV))
    twin = torch.nn.Parameter(m.grids.detach().clone())
    ours, theirs = FusedAdam([m.grids], lr=2e-3, eps=1e-15), torch.optim.Adam([twin], lr=2e-3, eps=1e-15)
    loss = (m.slice(rgb.to(DEV), 1) * v_out.to(DEV)).sum() + 10.0 * m.tv_loss()
    loss.backward()
    assert int(torch.count_nonzero(m.grids.grad[1])) > 0
    twin.grad = m.grids.grad.clone()
    before = m.grids.detach().clone()
    ours.step()
    theirs.step()
    step = (twin.detach() - before).abs().max()
    assert float(step) == pytest.approx(2e-3, rel=1e-3)  # (the first Adam step moves every touched element by lr)
    # both round p - update once (half an ulp of p each); the update itself, 2e-3 at most, differs far below that
    assert float((m.grids.detach() - twin.detach()).abs().max()) <= 2.0 ** -22 * float(twin.detach().abs().max())
    assert set(ours.state[m.grids]) == {"step", "exp_avg", "exp_avg_sq"}
