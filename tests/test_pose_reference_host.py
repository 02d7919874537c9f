"""CPU: tests/pose_reference.py (the camera gradient's float64 reference, autograd) against central differences of
`project_forward_fp64`'s float outputs contracted with the cotangents, over each of the 12 + 16 matrix entries, on
the cases of tests/projection_cases.py restricted to rows inside the guard band.

The contraction follows the backward's one convention that is not the forward's derivative: the compensation enters
as compensation^2 weighted by v_compensation * 0.5 / (compensation_0 + 1e-6), with compensation_0 the unperturbed
value (the rule of tests/projection_reference.py's header).  Rows within 1e-3 (relative) of a discrete boundary of
the forward (near plane, guard band, radius, tile edges) are left out: a finite step may carry them across it.

Tolerance: 1e-6 of the entry's mass.  The differences are float64 Richardson-extrapolated central differences with
steps 1e-4 and 5e-5 of max(1, |entry|): truncation O(h^4), rounding 1e-16 |F| / h -- both far below 1e-6 of the
mass on these cases (the achieved ratio is printed)."""
import numpy as np
import pytest

import pose_reference as POSE
import projection_cases as PC
import projection_reference as PR

CASES = [n for n in PC.names() if not n.endswith("-exact")]


def _forward(c, viewmat, projmat, eps=PR.AMBIG_EPS):
    sq = (None, None) if c.precomputed else (c.scales, c.quats)
    return PR.project_forward_fp64(c.means3d, sq[0], c.glob_scale, sq[1], viewmat, projmat, c.fx, c.fy, c.cx, c.cy,
                                   c.H, c.W, c.bw, c.clip, cov3d=c.cov3d if c.precomputed else None, eps=eps)


def _contract(f, rows, cot, wcomp):
    v_xy, v_depth, v_conic, _ = (np.asarray(v, np.float64) for v in cot)
    assert f["visible"][rows].all()  # the step moved no row across a boundary
    return ((f["xys"][rows] * v_xy[rows]).sum() + (f["depths"][rows] * v_depth[rows]).sum()
            + (f["conics"][rows] * v_conic[rows]).sum() + (f["compensation"][rows] ** 2 * wcomp[rows]).sum())


@pytest.mark.parametrize("name", CASES)
def test_reference_against_central_differences(name):
    c = PC.case(name)
    cot = PC.cotangents(c)
    V0, P0 = c.viewmat.astype(np.float64)[:3], c.projmat.astype(np.float64)
    f0 = _forward(c, V0, P0, eps=1e-3)
    sq = (None, None) if c.precomputed else (c.scales, c.quats)
    args = (c.means3d, sq[0], c.glob_scale, sq[1], V0, P0, c.fx, c.fy, c.cx, c.cy, c.H, c.W, f0["compensation"])
    guard = POSE.project_pose_vjp_fp64(*args, f0["visible"], *cot, cov3d=c.cov3d if c.precomputed else None)["guard"]
    rows = f0["visible"] & guard & ~f0["ambiguous"]
    assert rows.sum() >= 0.3 * min(c.n, 100)
    ref = POSE.project_pose_vjp_fp64(*args, rows, *cot, cov3d=c.cov3d if c.precomputed else None)
    wcomp = np.asarray(cot[3], np.float64) * 0.5 / (f0["compensation"] + 1e-6)

    def F(V, P):
        return _contract(_forward(c, V, P), rows, cot, wcomp)

    def diff(which, idx):
        def central(h):
            Vp, Vm, Pp, Pm = V0.copy(), V0.copy(), P0.copy(), P0.copy()
            (Vp if which == "v" else Pp)[idx] += h
            (Vm if which == "v" else Pm)[idx] -= h
            return (F(Vp, Pp) - F(Vm, Pm)) / (2 * h)
        h = 1e-4 * max(1.0, abs((V0 if which == "v" else P0)[idx]))
        return (4.0 * central(0.5 * h) - central(h)) / 3.0

    fd_v = np.array([[diff("v", (r, q)) for q in range(4)] for r in range(3)])
    fd_p = np.array([[diff("p", (r, q)) for q in range(4)] for r in range(4)])
    rv = POSE.mass_ratio(ref["v_viewmat"], fd_v, ref["mass_viewmat"])
    rp = POSE.mass_ratio(ref["v_projmat"], fd_p, ref["mass_projmat"])
    print(f"{name}: reference vs central differences, of the mass: viewmat {rv:.3e}, projmat {rp:.3e} "
          f"on {int(rows.sum())} rows")
    assert np.all(ref["v_projmat"][2] == 0) and np.all(ref["mass_projmat"][2] == 0) and np.all(fd_p[2] == 0)
    assert ref["mass_viewmat"].min() > 0 and ref["mass_projmat"][[0, 1, 3]].min() > 0
    assert rv <= 1e-6 and rp <= 1e-6


def test_one_cotangent_at_a_time_adds_up_and_nothing_visible_is_zero():
    """Linearity in the cotangents, None = zero, and no visible row = exact zeros with zero mass."""
    c = PC.case("everything")
    cot = PC.cotangents(c)
    f0 = _forward(c, c.viewmat[:3], c.projmat)
    args = (c.means3d, c.scales, c.glob_scale, c.quats, c.viewmat[:3], c.projmat, c.fx, c.fy, c.cx, c.cy, c.H, c.W,
            f0["compensation"], f0["visible"])
    full = POSE.project_pose_vjp_fp64(*args, *cot)
    parts = [POSE.project_pose_vjp_fp64(*args, *(v if j == k else None for j, v in enumerate(cot))) for k in range(4)]
    for key in ("v_viewmat", "v_projmat"):
        total = sum(p[key] for p in parts)
        assert np.abs(total - full[key]).max() <= 1e-12 * full["mass_" + key[2:]].max()
    assert not parts[1]["v_projmat"].any() and not parts[2]["v_projmat"].any()  # depth, conic: the view matrix alone
    none = POSE.project_pose_vjp_fp64(*args[:-1], np.zeros(c.n, bool), *cot)
    assert all(not none[k].any() for k in ("v_viewmat", "v_projmat", "mass_viewmat", "mass_projmat"))
