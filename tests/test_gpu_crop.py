"""GPU: the oriented crop box inside the projection kernel (gsr_project_forward_crop, gsr_crop_mask) and on every
route above it: the separate ops (gs_fused.project_gaussians_cropped, harness.pipeline.render_view), the one-call view
(gs_fused.render_gaussians), its HIP graph (ViewGraph.set_crop) and the export (crop_gaussians, fuse_views,
tools/export_gaussians.py).

Scenes: N in {1, 257, 1000} Gaussians (a single thread, one thread past a workgroup, a partial last workgroup) with
means uniform in [-2, 2]^3, seen at 64 x 48 (4 x 3 tiles) from orbit_cameras(8, 64, 48)[3]; SH degree 3, degree 0
once.  The boxes are tests/crop_reference.BOXES: (a) axis-aligned, about half; (b) rpy = (0.3, -0.7, 1.1), S = (1.5,
0.8, 2.5), off-centre; (c) a rotation times diag(1, 2, 0.5); (d) everything; (e) nothing; (f) S_y = 0, nothing.

The reference everywhere is the SAME route run on the gathered subset (what the toolkit's `get_outputs` does,
vanilla_gs.py:703-757): images at the project's image tolerance of 1e-4 absolute, gradients at its 1e-3 relative.
Largest image difference seen on an MI355X, over all routes, sizes and boxes: 0."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import crop_reference as CR
from harness import scene as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H = 64, 48
SIZES = (1, 257, 1000)
NAMES = tuple(CR.BOXES)
IMG_TOL, GRAD_TOL = 1e-4, 1e-3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cu(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)


def npy(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _raw(n, K=16):
    from harness.train import blob_scene

    raw = dict(blob_scene(n, seed=4, sh_degree={1: 0, 4: 1, 9: 2, 16: 3}[K], scale_lo=0.05, scale_hi=0.3))
    raw["means"] = CR.uniform_means(n, 100 + n)
    return raw


def _model(n, K=16, rows=None):
    """The raw parameters as leaves on the device; `rows`: only those (the gathered subset)."""
    return {k: cu(v if rows is None else v[rows]).requires_grad_(True) for k, v in _raw(n, K).items()}


def _camera_np():
    from harness.train import orbit_cameras

    return orbit_cameras(8, W, H)[3]


def _camera():
    from harness.pipeline import CameraTensors

    return CameraTensors.from_numpy(_camera_np(), DEV)


def _box(name):
    from gs_fused import CropBox

    return CropBox(*CR.BOXES[name])


def _keep(name, n):
    """Which rows of `_raw(n)` the box keeps, by the numpy.float32 restatement."""
    return CR.within_f32(CR.crop_values(*CR.BOXES[name]), _raw(n)["means"])


@functools.lru_cache(maxsize=None)
def _cotangents():
    g = torch.Generator(device=DEV).manual_seed(0)
    r = lambda *s: torch.rand(*s, device=DEV, generator=g) * 2 - 1  # noqa: E731
    return r(H, W, 3), r(H, W), r(H, W)


def _background():
    return torch.tensor(S.BACKGROUND, device=DEV)


# ---- 1. the rule, exactly ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_mask_kernel_equals_the_float32_restatement_bit_for_bit(name):
    import rasterizer.cuda as C

    pts = CR.rule_points()
    values = CR.crop_values(*CR.BOXES[name])
    box = _box(name)
    crop = box.tensor(DEV)
    assert npy(crop).tobytes() == values.tobytes()
    for n in (len(pts),) + SIZES:
        p = cu(pts[-n:])  # (the tail: the NaN means and the face points are in every slice but the shortest)
        want = CR.within_f32(values, pts[-n:])
        mask, count = C.crop_mask(p, crop)
        assert mask.dtype == torch.uint8 and mask.shape == (n,) and count.dtype == torch.int32
        assert np.array_equal(npy(mask).astype(bool), want), (name, n)
        assert int(count[0]) == int(mask.sum()) == int(want.sum())
        assert C.crop_mask(p, crop, want_count=False)[1] is None
        assert np.array_equal(npy(box.within(p)), want)
    assert not want[-3:].any()  # the NaN means


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_mask_kernel_on_the_faces(name):
    """Exactly on a face is outside; the float32 neighbour inside is inside, the one outside is outside."""
    import rasterizer.cuda as C

    on, inside, outside, _ = CR.face_points(name)
    crop = _box(name).tensor(DEV)
    for pts, want in ((on, False), (inside, True), (outside, False)):
        mask, count = C.crop_mask(cu(pts), crop)
        assert bool((mask.bool() == want).all()) and int(count[0]) == (64 if want else 0)


# ---- 2. the rule against the reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_mask_kernel_equals_orientedbox_within_away_from_the_faces(name):
    """`OrientedBox.within` as the reference writes it (tests/crop_reference.within_reference: the module itself
    needs viser and jaxtyping) on points 1e-3 away from every face: zero disagreements.  That the two host
    restatements agree on these very points is checked in tests/test_crop_host.py."""
    import rasterizer.cuda as C

    pts = CR.margin_points(name, 4000, seed=11)
    want = CR.within_reference(*CR.BOXES[name], pts)
    mask, count = C.crop_mask(cu(pts), _box(name).tensor(DEV))
    wrong = int((npy(mask).astype(bool) != want).sum())
    print(f"box {name}: {int(want.sum())} of 4000 inside, {wrong} disagreements")
    assert wrong == 0 and int(count[0]) == int(want.sum())


# ---- 3. the projection -------------------------------------------------------------------------------------------
def _project_inputs(n):
    raw, cam = _raw(n), _camera_np()
    q = raw["quats"] / np.linalg.norm(raw["quats"], axis=1, keepdims=True)
    k = (cu(raw["means"]), cu(np.exp(raw["scales"])), 1.0, cu(q.astype(np.float32)), cu(cam.viewmat[:3]), cu(cam.projmat),
         cam.fx, cam.fy, cam.cx, cam.cy, H, W)
    opac = torch.sigmoid(cu(raw["opacities"])).contiguous()
    return k, opac


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n", SIZES)
def test_cropped_projection_is_the_uncropped_one_inside_and_zero_outside(n, name):
    import rasterizer.cuda as C

    args, opac = _project_inputs(n)
    keep = torch.from_numpy(_keep(name, n)).to(DEV)
    crop = _box(name).tensor(DEV)
    ref = C.project_gaussians_forward_aa(n, *args, 16, 0.01, opac)
    assert (ref[3] > 0).float().mean() > 0.9 or n == 1  # (the scene is in view)
    names = ("cov3d", "xys", "depths", "radii", "conics", "compensation", "num_tiles_hit", "opacities_aa")
    for with_opacities in (False, True):
        out = C.project_gaussians_forward_crop(n, *args, 16, 0.01, crop, opac if with_opacities else None)
        assert (out[7] is not None) == with_opacities
        for a, b, nm in zip(out, ref, names):
            if a is None:
                continue
            assert a.shape == b.shape and a.dtype == b.dtype, nm
            assert torch.equal(a[keep], b[keep]), (nm, "inside")
            assert not a[~keep].any(), (nm, "outside")
        assert bool(((out[3] > 0) <= keep).all())
    if name == "d":
        assert bool(keep.all())
    if name in ("e", "f"):
        assert not bool(keep.any())


# ---- 4. the lists --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
@pytest.mark.parametrize("n", SIZES[1:])
def test_lists_of_the_cropped_projection_are_the_gathered_subsets(n, name):
    import rasterizer.cuda as C
    from rasterizer.utils import bin_and_sort_gaussians, compute_cumulative_intersects

    args, _ = _project_inputs(n)
    keep = _keep(name, n)
    assert keep.any()
    rows = cu(np.nonzero(keep)[0])
    tb = ((W + 15) // 16, (H + 15) // 16, 1)

    def lists(m, a):
        _, xys, depths, radii, _, _, tiles = a
        total, cum = compute_cumulative_intersects(tiles)
        assert total > 0
        return bin_and_sort_gaussians(m, total, xys, depths, radii, cum, tb, 16)[3:]

    ids, bins = lists(n, C.project_gaussians_forward_crop(n, *args, 16, 0.01, _box(name).tensor(DEV))[:7])
    sub = tuple(t[rows].contiguous() if torch.is_tensor(t) and t.dim() == 2 and t.shape[0] == n else t for t in args)
    m = int(keep.sum())
    ids_s, bins_s = lists(m, C.project_gaussians_forward(m, *sub, 16, 0.01))
    assert torch.equal(bins, bins_s)
    assert torch.equal(ids.long(), rows[ids_s.long()])


# ---- 5 / 6. images and gradients on the separate ops and the one-call view ------------------------------------------
def _separate(p, crop, deg, mode="classic", fused_depth=True, **kw):
    from gs_fused import activate_gaussians
    from harness.pipeline import render_view

    cam = _camera()
    scales, quats, opac, dirs = activate_gaussians(p["means"], p["scales"], p["quats"], p["opacities"], cam.campos)
    out = render_view(p["means"], scales, quats, opac, (p["features_dc"], p["features_rest"]), cam, _background(), deg,
                      rasterize_mode=mode, render_depth=True, fused_depth=fused_depth, normalise_depth=False,
                      clamp_rgb=False, viewdirs=dirs, crop=crop, **kw)
    return out["rgb"], out["alpha"][..., 0], out["depth_acc"][..., 0]


def _one_call(p, crop, deg, mode="classic"):
    from gs_fused import ViewSpec, render_gaussians

    cam = _camera()
    spec = ViewSpec(H, W, cam.fx, cam.fy, cam.cx, cam.cy, deg, render_depth=True, rasterize_mode=mode)
    out = render_gaussians(p["means"], p["scales"], p["quats"], p["opacities"], p["features_dc"], p["features_rest"],
                           cam.viewmat, cam.projmat, cam.campos, _background(), spec, capacity=200_000, crop=crop)
    return out["rgb"], out["alpha"], out["depth"]


ROUTES = {"separate ops": _separate, "render_gaussians": _one_call}


def _nothing():
    return _background().expand(H, W, 3), torch.zeros(H, W, device=DEV), torch.zeros(H, W, device=DEV)


def _backward(outs):
    torch.autograd.backward(list(outs), list(_cotangents()))


def _compare(route, n, name, K=16, deg=3, mode="classic"):
    """Images and gradients of `route` with the crop against the same route on the gathered subset."""
    fn = ROUTES[route]
    keep = _keep(name, n)
    full = _model(n, K)
    got = fn(full, _box(name).tensor(DEV), deg, mode)
    _backward(got)
    if keep.any():
        sub = _model(n, K, rows=keep)
        want = fn(sub, None, deg, mode)
        _backward(want)
    else:
        sub, want = None, _nothing()
    worst = 0.0
    for a, b, nm in zip(got, want, ("rgb", "alpha", "depth")):
        d = float((a.detach() - b.detach()).abs().max())
        worst = max(worst, d)
        assert d <= IMG_TOL, (route, n, name, nm, d)
    rows = torch.from_numpy(keep).to(DEV)
    for k, t in full.items():
        if t.numel() == 0:  # (features_rest at SH degree 0)
            continue
        assert t.grad is not None, k
        assert not t.grad[~rows].any(), (route, n, name, k, "outside rows must be exactly zero")
        if sub is not None:
            a, b = t.grad[rows], sub[k].grad
            assert float((a - b).abs().max()) <= GRAD_TOL * float(b.abs().max()) + 1e-12, (route, n, name, k)
    if sub is not None and name in ("a", "d") and n > 1:
        assert float(full["means"].grad.abs().max()) > 0
    print(f"{route}, n = {n}, box {name} ({int(keep.sum())} kept, {mode}): worst image difference {worst:.3e}")
    return got, worst


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("route", list(ROUTES))
def test_route_with_a_crop_equals_the_route_on_the_gathered_subset(route, n, name):
    got, _ = _compare(route, n, name)
    if name == "d":  # everything: the uncropped render, bit for bit
        with torch.no_grad():
            plain = ROUTES[route](_model(n), None, 3)
        for a, b in zip(got, plain):
            assert torch.equal(a, b)
    if name in ("e", "f"):  # nothing: the background with alpha 0
        for a, b in zip(got, _nothing()):
            assert torch.equal(a, b)


@pytest.mark.parametrize("route", list(ROUTES))
def test_routes_at_sh_degree_zero_and_in_antialiased_mode(route):
    _compare(route, 257, "a", K=1, deg=0)
    _compare(route, 1000, "c", mode="antialiased")


def test_separate_ops_with_two_compositing_passes():
    """`render_view(fused_depth=False)`: `rasterize_gaussians(return_alpha=True)` and a second pass for the depth,
    the branch the reference's models take.  Part of a box against the gathered subset, and the empty boxes: the
    background with alpha 0 and depth 0."""
    n = 257
    with torch.no_grad():
        got = _separate(_model(n), _box("a").tensor(DEV), 3, fused_depth=False)
        want = _separate(_model(n, rows=_keep("a", n)), None, 3, fused_depth=False)
        for a, b, nm in zip(got, want, ("rgb", "alpha", "depth")):
            assert float((a - b).abs().max()) <= IMG_TOL, nm
        assert float(got[1].max()) > 0
        for name in ("e", "f"):
            for a, b, nm in zip(_separate(_model(n), _box(name), 3, fused_depth=False), _nothing(), ("rgb", "alpha", "depth")):
                assert torch.equal(a, b), (name, nm)


def test_cropped_projection_backward_with_every_cotangent_and_the_pose():
    """`project_gaussians_cropped(opacities=...)` with cotangents on xys, depths, conics, the compensation AND
    opacities_aa at once, the camera a leaf (viewmat [4,4], projmat = P @ viewmat): inside rows and the camera
    gradient against `project_gaussians` + the multiply line on the gathered subset, at the 1e-3 bar; outside rows
    exactly zero."""
    from gs_fused import project_gaussians_cropped
    from rasterizer import project_gaussians

    n, name = 1000, "a"
    raw, cam = _raw(n), _camera_np()
    keep = _keep(name, n)
    rows = torch.from_numpy(keep).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(6)
    cot = {k: torch.randn(n, *shape, device=DEV, generator=g)
           for k, shape in (("xys", (2,)), ("depths", ()), ("conics", (3,)), ("comp", ()), ("oaa", (1,)))}
    Pm = cu(S.projection_matrix(0.001, 1000.0, 2 * np.arctan(W / (2 * cam.fx)),
                                2 * np.arctan(H / (2 * cam.fy))).astype(np.float32))
    q = (raw["quats"] / np.linalg.norm(raw["quats"], axis=1, keepdims=True)).astype(np.float32)

    def leaves(sel):
        pick = (lambda a: a) if sel is None else (lambda a: a[sel])
        return {"means": cu(pick(raw["means"])).requires_grad_(), "scales": cu(pick(np.exp(raw["scales"]))).requires_grad_(),
                "quats": cu(pick(q)).requires_grad_(),
                "opacities": torch.sigmoid(cu(pick(raw["opacities"]))).detach().requires_grad_(),
                "viewmat": cu(cam.viewmat).requires_grad_()}

    def loss(xys, depths, conics, comp, oaa, sel):
        c = cot if sel is None else {k: v[sel] for k, v in cot.items()}
        return ((xys * c["xys"]).sum() + (depths * c["depths"]).sum() + (conics * c["conics"]).sum()
                + (comp * c["comp"]).sum() + (oaa * c["oaa"]).sum())

    full = leaves(None)
    args = lambda L: (L["means"], L["scales"], 1, L["quats"], L["viewmat"][:3, :], Pm @ L["viewmat"], cam.fx, cam.fy,  # noqa: E731
                      cam.cx, cam.cy, H, W, 16)
    xys, depths, radii, conics, comp, tiles, cov3d, oaa = project_gaussians_cropped(
        *args(full), _box(name), opacities=full["opacities"])
    loss(xys, depths, conics, comp, oaa, None).backward()
    sub = leaves(keep)
    xys, depths, radii_s, conics, comp, tiles, cov3d = project_gaussians(*args(sub))
    loss(xys, depths, conics, comp, sub["opacities"] * comp[:, None], rows).backward()
    assert int((radii_s > 0).sum()) > 100
    for k in ("means", "scales", "quats", "opacities"):
        a, b = full[k].grad, sub[k].grad
        assert not a[~rows].any(), (k, "outside rows must be exactly zero")
        assert float(b.abs().max()) > 0
        assert float((a[rows] - b).abs().max()) <= GRAD_TOL * float(b.abs().max()), k
    a, b = full["viewmat"].grad, sub["viewmat"].grad
    assert a.shape == (4, 4) and float(b.abs().max()) > 0
    assert float((a - b).abs().max()) <= GRAD_TOL * float(b.abs().max()), "viewmat"


def test_an_empty_crop_with_the_read_back_gives_the_references_dict():
    """`caller_syncs=True`: the `radii.sum() == 0` branch -- what the reference returns for `crop_ids.sum() == 0`
    (vanilla_gs.py:750-757): the background, depth 10, accumulation 0."""
    from gs_fused import activate_gaussians
    from harness.pipeline import render_view

    cam, bg = _camera(), _background()
    with torch.no_grad():
        p = _model(257)
        scales, quats, opac, dirs = activate_gaussians(p["means"], p["scales"], p["quats"], p["opacities"], cam.campos)
        for name in ("e", "f"):
            out = render_view(p["means"], scales, quats, opac, (p["features_dc"], p["features_rest"]), cam, bg, 3,
                              render_depth=True, viewdirs=dirs, caller_syncs=True, crop=_box(name))
            assert torch.equal(out["rgb"], bg.expand(H, W, 3)) and out["rgb"].shape == (H, W, 3)
            assert out["alpha"].shape == (H, W, 1) and not out["alpha"].any()
            assert out["depth"].shape == (H, W, 1) and bool((out["depth"] == 10).all())
            assert not out["radii"].any()


def test_crop_arguments_are_checked():
    from gs_fused import ViewSpec, project_gaussians_cropped, render_gaussians

    p = _model(257)
    cam = _camera()
    spec = ViewSpec(H, W, cam.fx, cam.fy, cam.cx, cam.cy, 3)
    args = (p["means"], p["scales"], p["quats"], p["opacities"], p["features_dc"], p["features_rest"], cam.viewmat,
            cam.projmat, cam.campos, _background(), spec, 100_000)
    with pytest.raises(RuntimeError, match="crop"):
        render_gaussians(*args, crop=torch.zeros(12, device=DEV))
    with pytest.raises(RuntimeError, match="crop"):
        render_gaussians(*args, crop=torch.zeros(16))
    with pytest.raises(ValueError, match="crop"):
        project_gaussians_cropped(p["means"], p["scales"].exp(), 1, p["quats"], cam.viewmat[:3], cam.projmat, cam.fx,
                                  cam.fy, cam.cx, cam.cy, H, W, 16, torch.zeros(4, device=DEV))


# ---- 7. the graph --------------------------------------------------------------------------------------------------
def _loss(out, targets):
    return ((out["rgb"] - targets[0]) ** 2).sum() + 0.5 * out["alpha"].sum() + 0.1 * out["depth"].sum()


def _graph(n, K, deg, crop):
    from gs_fused import ViewSpec
    from gs_fused.render import ViewGraph

    cam = _camera()
    spec = ViewSpec(H, W, cam.fx, cam.fy, cam.cx, cam.cy, deg, render_depth=True)
    p = _model(n, K)
    vg = ViewGraph(p, spec, 200_000, _loss, _background(), [(H, W, 3)], crop=crop)
    target = (torch.rand(H, W, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2)),)
    vg.capture(cam.viewmat, cam.projmat, cam.campos, target)
    return vg, p, cam, target


@pytest.mark.parametrize("n,K,deg", [(1000, 16, 3), (257, 1, 0), (1, 16, 3)])
def test_view_graph_moves_its_crop_box_without_capturing_again(n, K, deg):
    """Captured with (a), replayed, moved to (b), replayed: loss, image and .grad equal those of a graph captured with
    (b).  Then the box goes through all six on the same graph: every replay equals the eager view of the gathered
    subset."""
    from gs_fused import ViewSpec, render_gaussians

    vg, p, cam, target = _graph(n, K, deg, _box("a"))
    graph = vg.graph
    loss, out = vg.replay(cam.viewmat, cam.projmat, cam.campos, target)
    first = float(loss.detach())
    vg.set_crop(_box("b"))
    loss, out = vg.replay(cam.viewmat, cam.projmat, cam.campos, target)
    torch.cuda.synchronize()
    assert vg.graph is graph and vg.fits()
    vb, pb, _, _ = _graph(n, K, deg, _box("b").tensor(DEV))
    loss_b, out_b = vb.replay(cam.viewmat, cam.projmat, cam.campos, target)
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - float(loss_b.detach())) <= 1e-6 * max(1.0, abs(float(loss_b.detach())))
    if _keep("a", n).sum() != _keep("b", n).sum():
        assert first != float(loss.detach())
    for k in ("rgb", "alpha", "depth"):
        assert float((out[k] - out_b[k]).abs().max()) <= IMG_TOL, k
    for k in p:
        if p[k].numel() == 0:  # (features_rest at SH degree 0)
            continue
        a, b = p[k].grad, pb[k].grad
        assert float((a - b).abs().max()) <= GRAD_TOL * float(b.abs().max()) + 1e-12, k
        assert not a[~torch.from_numpy(_keep("b", n)).to(DEV)].any(), k
    # the same graph, every box
    spec = ViewSpec(H, W, cam.fx, cam.fy, cam.cx, cam.cy, deg, render_depth=True)
    plain_graph, _, _, _ = _graph(n, K, deg, None)  # the same route without a box
    _, plain = plain_graph.replay(cam.viewmat, cam.projmat, cam.campos, target)
    plain = {k: plain[k].clone() for k in ("rgb", "alpha", "depth")}
    worst = 0.0
    for name in NAMES:
        vg.set_crop(_box(name).tensor("cpu"))
        _, out = vg.replay(cam.viewmat, cam.projmat, cam.campos, target)
        keep = _keep(name, n)
        if keep.any():
            with torch.no_grad():
                s = _model(n, K, rows=keep)
                e = render_gaussians(s["means"], s["scales"], s["quats"], s["opacities"], s["features_dc"],
                                     s["features_rest"], cam.viewmat, cam.projmat, cam.campos, _background(), spec,
                                     capacity=200_000)
            want = (e["rgb"], e["alpha"], e["depth"])
        else:
            want = _nothing()
        for k, b in zip(("rgb", "alpha", "depth"), want):
            d = float((out[k] - b).abs().max())
            worst = max(worst, d)
            assert d <= IMG_TOL, (name, k, d)
        if name == "d":  # everything: the replay of the graph without a box, bit for bit
            for k in ("rgb", "alpha", "depth"):
                assert torch.equal(out[k], plain[k]), k
        if name in ("e", "f"):  # nothing: the background with alpha 0
            for k, b in zip(("rgb", "alpha", "depth"), _nothing()):
                assert torch.equal(out[k], b), (name, k)
        assert vg.graph is graph
    print(f"ViewGraph replay, n = {n}: worst image difference over the six boxes {worst:.3e}")


def test_view_graph_without_a_crop_refuses_set_crop():
    from gs_fused import ViewSpec
    from gs_fused.render import ViewGraph

    cam = _camera()
    spec = ViewSpec(H, W, cam.fx, cam.fy, cam.cx, cam.cy, 3, render_depth=True)
    vg = ViewGraph(_model(257), spec, 200_000, _loss, _background(), [(H, W, 3)])
    assert vg.crop is None
    with pytest.raises(ValueError, match="without a crop"):
        vg.set_crop(_box("a"))
    with pytest.raises(ValueError, match="float32"):
        ViewGraph(_model(257), spec, 200_000, _loss, _background(), [(H, W, 3)], crop=torch.zeros(3))


# ---- 8. export -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_crop_gaussians_returns_the_rows_of_within(name):
    from gs_fused import crop_gaussians

    n = 1000
    params = {k: cu(v) for k, v in _raw(n).items()}
    keep = _keep(name, n)
    out, mask = crop_gaussians(params, _box(name), return_mask=True)
    assert mask.dtype == torch.bool and np.array_equal(npy(mask), keep)
    assert set(out) == set(params)
    for k, v in params.items():
        assert torch.equal(out[k], v[torch.from_numpy(keep).to(DEV)]), k
    assert out["means"].shape[0] == int(keep.sum())


def test_export_gaussians_writes_the_kept_rows(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import export_gaussians as G
    from gs_io import read_gaussian_ply

    n = 1000
    raw = _raw(n)
    ckpt = tmp_path / "step-000000007.ckpt"
    torch.save({"step": 7, "pipeline": {"_model.gauss_params." + k: torch.from_numpy(v) for k, v in raw.items()},
                "optimizers": {}, "schedulers": {}, "scalers": {}}, str(ckpt))
    out = tmp_path / "gaussians.ply"
    G.main([str(ckpt), str(out), "--device", DEV, "--obb-pos", "0.3", "-0.2", "0.4", "--obb-rpy", "0.3", "-0.7", "1.1",
            "--obb-scale", "1.5", "0.8", "2.5"])
    keep = _keep("b", n)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["gaussians"] == n and line["written"] == int(keep.sum()) > 0
    back = read_gaussian_ply(str(out))
    for k, v in raw.items():
        assert np.array_equal(np.asarray(back[k]).reshape(v[keep].shape), v[keep]), k


def test_fuse_views_with_a_crop_box_equals_fusing_the_gathered_parameters():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from export_tsdf import activated

    from gs_fusion import TSDFVolume, fuse_views
    from harness.train import orbit_cameras

    n = 1000
    raw = _raw(n)
    cams = orbit_cameras(8, W, H)[::2]
    bg = torch.zeros(3, device=DEV)
    volume = lambda: TSDFVolume.from_bounds([-2.5] * 3, [2.5] * 3, 5.0 / 64, 0.3, None, DEV)  # noqa: E731
    keep = _keep("b", n)
    params = activated(raw, torch.device(DEV))
    sub = activated({k: v[keep] for k, v in raw.items()}, torch.device(DEV))
    va, vb, ve = volume(), volume(), volume()
    fuse_views(va, params, cams, bg, 3, alpha_min=0.05, crop_box=_box("b"))
    fuse_views(vb, sub, cams, bg, 3, alpha_min=0.05)
    fuse_views(ve, params, cams, bg, 3, alpha_min=0.05, crop_box=_box("e"))
    a, b, e = va.state_dict(), vb.state_dict(), ve.state_dict()
    assert a["num_allocated"] == b["num_allocated"] > 0 and torch.equal(a["table"], b["table"])
    d_tsdf = float((a["tsdf"] - b["tsdf"]).abs().max())
    d_weight = float((a["weight"] - b["weight"]).abs().max())
    print(f"fuse_views(crop_box=b) against the gathered parameters: tsdf {d_tsdf:.3e}, weight {d_weight:.3e}, "
          f"{a['num_allocated']} blocks")
    assert d_weight == 0 and d_tsdf < 1e-4  # (the bars of tests/test_gpu_tsdf.py: no weight mismatch, 1e-4)
    assert e["num_allocated"] == 0
    full = volume()
    fuse_views(full, params, cams, bg, 3, alpha_min=0.05)
    assert full.state_dict()["num_allocated"] > a["num_allocated"]  # (the crop is not ignored)
