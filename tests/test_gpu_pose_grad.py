"""GPU: the camera's gradient through the projection (csrc/project.hip's pose pass, `rasterizer.cuda.
project_gaussians_backward_pose`, and `project_gaussians`' autograd slots for `viewmat` / `projmat`) against the float64
reference of tests/pose_reference.py, on the cases of tests/projection_cases.py and on sizes chosen for the reduction:
0, 1, the 256-lane block +- 1, one workgroup's share (1024 Gaussians) +- 1, and 64 * 1024 + 1 -- the smallest n that
hands the final kernel more partials (65) than one wave holds.

The bound: every entry within 1e-3 of its MASS (the sum over the Gaussians of the magnitudes of their terms).  The
project holds each per-Gaussian backward row to 1e-3 of its row (tests/test_gpu_projection.py); a sum of rows held
to that cannot be asked for more than 1e-3 of the summed magnitudes.  The achieved ratios are printed."""
import functools

import numpy as np
import pytest
import torch

import pose_reference as POSE
import projection_cases as PC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHARE = 1024  # Gaussians per workgroup of the pose pass (GSR_POSE_SHARE)
SIZES = (1, 255, 256, 257, SHARE - 1, SHARE, SHARE + 1, 64 * SHARE + 1)
RUNNABLE = [n for n in PC.names() if not n.endswith("-exact")]
FWD = ("cov3d", "xys", "depths", "radii", "conics", "compensation", "num_tiles_hit")
BOUND = 1e-3


def cu(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def npy(t):
    return None if t is None else t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def get_case(name):
    if name.startswith("reduce-"):
        n = int(name.split("-")[1])
        return PC._case(name, np.random.default_rng(300 + n % 97), n, 200, 120, 16, scale=(0.02, 0.05))
    if name == "all-culled":  # every centre behind the camera
        return PC._case(name, np.random.default_rng(299), 700, 200, 120, 16, z_range=(-9.0, -1.0))
    return PC.case(name)


@functools.lru_cache(maxsize=None)
def forward(name):
    """-> the GPU forward's outputs as device tensors (shared, read-only)."""
    import rasterizer.cuda as C

    c = get_case(name)
    a = [cu(x) if isinstance(x, np.ndarray) else x for x in c.forward_args()]
    return dict(zip(FWD, C.project_gaussians_forward(*a, **({"cov3d_precomp": cu(c.cov3d)} if c.precomputed else {}))))


def pose(name, cot, fwd=None):
    import rasterizer.cuda as C

    c, o = get_case(name), forward(name) if fwd is None else fwd
    return tuple(npy(t) for t in C.project_gaussians_backward_pose(
        c.n, cu(c.means3d), cu(c.viewmat[:3]), cu(c.projmat), c.fx, c.fy, c.H, c.W, o["cov3d"], o["radii"], o["conics"],
        o["compensation"], *(cu(v) for v in cot)))


def reference(name, cot):
    c, o = get_case(name), forward(name)
    sq = (None, None) if c.precomputed else (c.scales, c.quats)
    return POSE.project_pose_vjp_fp64(c.means3d, sq[0], c.glob_scale, sq[1], c.viewmat[:3], c.projmat, c.fx, c.fy, c.cx,
                                      c.cy, c.H, c.W, npy(o["compensation"]), npy(o["radii"]) > 0, *cot,
                                      cov3d=c.cov3d if c.precomputed else None)


@functools.lru_cache(maxsize=None)
def full_reference(name):
    return reference(name, PC.cotangents(get_case(name)))


def check(name, cot, ref, what):
    vv, vp = pose(name, cot)
    rv = POSE.mass_ratio(vv, ref["v_viewmat"], ref["mass_viewmat"])
    rp = POSE.mass_ratio(vp, ref["v_projmat"], ref["mass_projmat"])
    print(f"{name} [{what}]: |HIP - fp64| / mass: viewmat {rv:.3e}, projmat {rp:.3e}")
    assert vv.shape == (3, 4) and vp.shape == (4, 4)
    assert np.all(vp[2] == 0), "row 2 of v_projmat is exactly zero"
    assert rv <= BOUND and rp <= BOUND, (what, rv, rp)
    return vv, vp


@pytest.mark.parametrize("name", RUNNABLE + [f"reduce-{n}" for n in SIZES])
def test_against_float64(name):
    c = get_case(name)
    ref = full_reference(name)
    assert (npy(forward(name)["radii"]) > 0).mean() >= 0.2
    assert ref["mass_viewmat"].min() > 0  # every path carries something
    check(name, PC.cotangents(c), ref, "all cotangents")


@pytest.mark.parametrize("name", ["everything", "everything-precomputed", "guardband", f"reduce-{SHARE + 1}"])
def test_one_cotangent_at_a_time(name):
    """A missing or mis-signed path cannot hide behind another's mass; a null cotangent is a zero cotangent."""
    c = get_case(name)
    cot = PC.cotangents(c)
    for k, what in enumerate(("v_xy", "v_depth", "v_conic", "v_compensation")):
        only = tuple(v if j == k else None for j, v in enumerate(cot))
        ref = reference(name, only)
        # v_xy reaches rows 0, 1, 3 of the projection matrix alone, v_depth row 2 of the view matrix alone, the other
        # two the whole view matrix alone; the entries of zero mass must then be exact zeros (`mass_ratio`)
        mv, mp = ref["mass_viewmat"] > 0, ref["mass_projmat"] > 0
        assert mp[[0, 1, 3]].all() == (k == 0) and mp.any() == (k == 0)
        assert mv[2].all() == (k != 0) and mv[:2].all() == (k >= 2) and mv[:2].any() == (k >= 2)
        got = check(name, only, ref, what + " only")
        zeros = pose(name, tuple(v if j == k else np.zeros_like(v) for j, v in enumerate(cot)))
        assert all(np.array_equal(a, b) for a, b in zip(got, zeros)), what
    none = pose(name, (None,) * 4)
    assert not none[0].any() and not none[1].any()


def test_nothing_to_sum_gives_exact_zeros():
    import rasterizer.cuda as C

    assert not (npy(forward("all-culled")["radii"]) > 0).any()
    vv, vp = pose("all-culled", PC.cotangents(get_case("all-culled")))
    assert not vv.any() and not vp.any()
    e = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device=DEV)  # noqa: E731
    c = get_case("blockedge-1")
    vv, vp = C.project_gaussians_backward_pose(0, e(0, 3), cu(c.viewmat[:3]), cu(c.projmat), c.fx, c.fy, c.H, c.W,
                                               e(0, 6), e(0, dt=torch.int32), e(0, 3), e(0), e(0, 2), e(0), e(0, 3),
                                               e(0))
    assert vv.shape == (3, 4) and vp.shape == (4, 4) and not npy(vv).any() and not npy(vp).any()


def test_translation_columns_agree_with_the_sum_of_v_mean3d():
    """sum_i v_mean3d_i = P[:, :3]^T v_projmat[:, 3] + W^T v_viewmat[:, 3]: the existing backward's rows against the
    pose pass' translation columns (a transposed accumulation shows here), each side a sum of rows held to 1e-3."""
    import rasterizer.cuda as C

    name = "everything"
    c, o, cot = get_case(name), forward(name), PC.cotangents(get_case(name))
    ref = full_reference(name)
    vv, vp = check(name, cot, ref, "translation columns")
    grads = C.project_gaussians_backward(c.n, cu(c.means3d), cu(c.scales), c.glob_scale, cu(c.quats), cu(c.viewmat[:3]),
                                         cu(c.projmat), c.fx, c.fy, c.cx, c.cy, c.H, c.W, o["cov3d"], o["radii"],
                                         o["conics"], o["compensation"], *(cu(v) for v in cot))
    lhs = npy(grads[2]).astype(np.float64).sum(axis=0)
    W, P3 = c.viewmat[:3, :3].astype(np.float64), c.projmat[:, :3].astype(np.float64)
    rhs = P3.T @ vp[:, 3].astype(np.float64) + W.T @ vv[:, 3].astype(np.float64)
    mass = np.abs(P3).T @ ref["mass_projmat"][:, 3] + np.abs(W).T @ ref["mass_viewmat"][:, 3]
    print(f"sum v_mean3d vs translation columns, of the mass: {(np.abs(lhs - rhs) / mass).max():.3e}")
    assert np.all(np.abs(lhs - rhs) <= 2 * BOUND * mass)  # (both sides carry the bound)
    for got, key in ((vv[:, 3], "viewmat"), (vp[:, 3], "projmat")):
        assert POSE.mass_ratio(got, ref["v_" + key][:, 3], ref["mass_" + key][:, 3]) <= BOUND


@pytest.mark.parametrize("name", ["everything", f"reduce-{64 * SHARE + 1}"])
def test_two_calls_give_the_same_bits_and_leave_the_backward_alone(name):
    import rasterizer.cuda as C

    c, o, cot = get_case(name), forward(name), PC.cotangents(get_case(name))

    def backward():
        return [npy(t) for t in C.project_gaussians_backward(
            c.n, cu(c.means3d), cu(c.scales), c.glob_scale, cu(c.quats), cu(c.viewmat[:3]), cu(c.projmat), c.fx, c.fy,
            c.cx, c.cy, c.H, c.W, o["cov3d"], o["radii"], o["conics"], o["compensation"], *(cu(v) for v in cot))]

    before = backward()
    a, b = pose(name, cot), pose(name, cot)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].any() and a[1].any()
    after = backward()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))


def test_precomputed_covariances_give_the_same_matrices():
    import rasterizer.cuda as C

    name = "everything"
    c, o, cot = get_case(name), forward(name), PC.cotangents(get_case(name))
    a = [cu(x) if isinstance(x, np.ndarray) else x for x in c.forward_args()]
    a[2] = a[4] = None
    pre = dict(zip(FWD, C.project_gaussians_forward(*a, cov3d_precomp=o["cov3d"].clone())))
    full, handed = pose(name, cot), pose(name, cot, fwd=pre)
    assert np.array_equal(full[0], handed[0]) and np.array_equal(full[1], handed[1]) and full[0].any()


def _autograd_case():
    c = get_case("anamorphic-317x203-bw16")
    Pm = PC._projection(0.001, 1000.0, 0.5 * c.W / c.fx, 0.5 * c.H / c.fy).astype(np.float32)
    return c, cu(Pm)


def test_autograd_delivers_both_gradients_to_the_view_matrix():
    import rasterizer.cuda as C
    from rasterizer import project_gaussians

    c, Pm = _autograd_case()
    cot = [cu(v) for v in PC.cotangents(c)]
    viewmat4 = cu(c.viewmat).requires_grad_()
    projmat = Pm @ viewmat4
    means = cu(c.means3d).requires_grad_()
    xys, depths, radii, conics, comp, _, cov3d = project_gaussians(
        means, cu(c.scales), c.glob_scale, cu(c.quats), viewmat4, projmat, c.fx, c.fy, c.cx, c.cy, c.H, c.W, c.bw, c.clip)
    ((xys * cot[0]).sum() + (depths * cot[1]).sum() + (conics * cot[2]).sum() + (comp * cot[3]).sum()).backward()
    assert viewmat4.grad is not None and viewmat4.grad.shape == (4, 4)
    vv, vp = C.project_gaussians_backward_pose(c.n, means.detach(), viewmat4.detach(), projmat.detach(), c.fx, c.fy, c.H,
                                               c.W, cov3d, radii, conics.detach(), comp.detach(), *cot)
    want = Pm.t().mm(vp)
    want[:3] += vv  # (v_viewmat with a zero last row)
    # the same float32 numbers through one more 4-term dot product and one addition, in whatever order torch's
    # matmul takes them: round-off of the largest magnitude involved
    scale = float((Pm.abs().t().mm(vp.abs())).max() + vv.abs().max())
    assert torch.allclose(viewmat4.grad, want, rtol=0.0, atol=4 * 2.0 ** -24 * scale), (viewmat4.grad - want).abs().max()
    assert float(vv.abs().max()) > 0 and means.grad is not None

    # a [3,4] view matrix gets a [3,4] gradient: the pose pass' own output
    v3 = cu(c.viewmat[:3]).requires_grad_()
    out = project_gaussians(cu(c.means3d), cu(c.scales), c.glob_scale, cu(c.quats), v3, projmat.detach(), c.fx, c.fy,
                            c.cx, c.cy, c.H, c.W, c.bw, c.clip)
    ((out[0] * cot[0]).sum() + (out[1] * cot[1]).sum() + (out[3] * cot[2]).sum() + (out[4] * cot[3]).sum()).backward()
    assert v3.grad.shape == (3, 4) and torch.equal(v3.grad, vv)


def test_autograd_answers_only_what_is_asked():
    from rasterizer import project_gaussians

    c, Pm = _autograd_case()
    cot = [cu(v) for v in PC.cotangents(c)]
    viewmat, projmat = cu(c.viewmat), cu(c.projmat).requires_grad_()
    out = project_gaussians(cu(c.means3d), cu(c.scales), c.glob_scale, cu(c.quats), viewmat, projmat, c.fx, c.fy,
                            c.cx, c.cy, c.H, c.W, c.bw, c.clip)
    ((out[0] * cot[0]).sum() + (out[1] * cot[1]).sum()).backward()
    assert viewmat.grad is None
    assert projmat.grad is not None and projmat.grad.shape == (4, 4) and bool(projmat.grad[[0, 1, 3]].any())
    assert not projmat.grad[2].any()
    # no camera gradient asked for: None for both, as before
    means = cu(c.means3d).requires_grad_()
    viewmat, projmat = cu(c.viewmat), cu(c.projmat)
    out = project_gaussians(means, cu(c.scales), c.glob_scale, cu(c.quats), viewmat, projmat, c.fx, c.fy, c.cx, c.cy,
                            c.H, c.W, c.bw, c.clip)
    (out[0] * cot[0]).sum().backward()
    assert viewmat.grad is None and projmat.grad is None and means.grad is not None


def test_a_short_workspace_is_refused():
    import ctypes

    from rasterizer.cuda._backend import lib

    L = lib()
    assert L.gsr_project_backward_pose_workspace(ctypes.c_int(0)) == 0
    assert L.gsr_project_backward_pose_workspace(ctypes.c_int(SHARE + 1)) == 2 * 24 * 8
    c, o = get_case("blockedge-257"), forward("blockedge-257")
    t = [cu(c.means3d), cu(c.viewmat[:3]), cu(c.projmat)]
    ws, vv, vp = (torch.zeros(s, dtype=torch.float64, device=DEV) for s in (24, 6, 8))
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    rc = L.gsr_project_backward_pose(
        ctypes.c_int(c.n), p(t[0]), p(t[1]), p(t[2]), ctypes.c_float(c.fx), ctypes.c_float(c.fy), ctypes.c_uint(c.H),
        ctypes.c_uint(c.W), p(o["cov3d"]), p(o["radii"]), p(o["conics"]), p(o["compensation"]), None, None, None, None,
        p(ws), ctypes.c_size_t(24 * 8 - 8), p(vv), p(vp), None)
    assert rc != 0 and b"workspace" in L.gsr_last_error()
