"""CPU: the projection off the one camera family the rest of the suite uses (tests/projection_cases.py).

Three parties: the float64 restatement of the CUDA source's rules (tests/projection_reference.py), the reference's
own torch code on rows of the cases (tests/golden/project.npz, made by make_golden_project.py) and the C oracle that
csrc/project.hip is held bit-identical to (tests/test_gpu_projection.py).  float64 is pinned on the reference's data;
that comparison also measures how far an fp32 implementation -- the reference's -- is from float64 on each case, and
the oracle's forward may be twice as far, plus 1e-6 of the row.  Discrete outputs must be equal wherever float64 does
not call the row ambiguous (within 1e-5 relative of the near plane, a guard-band limit, an integer radius or a tile
edge)."""
import functools
import os

import numpy as np
import pytest

import projection_cases as PC
import projection_reference as PR
from oracle import oracle as O

FWD = ("cov3d", "xys", "depths", "radii", "conics", "compensation", "num_tiles_hit")
COTANGENTS = {"v_xy": (1, 0, 0, 0), "v_depth": (0, 1, 0, 0), "v_conic": (0, 0, 1, 0), "v_compensation": (0, 0, 0, 1),
              "all": (1, 1, 1, 1)}


def _precomp(c):
    return c.cov3d if c.precomputed else None


@functools.lru_cache(maxsize=None)
def fp64_forward(name):
    c = PC.case(name)
    sq = (None, None) if c.precomputed else (c.scales, c.quats)
    return PR.project_forward_fp64(c.means3d, sq[0], c.glob_scale, sq[1], c.viewmat, c.projmat, c.fx, c.fy, c.cx, c.cy,
                                   c.H, c.W, c.bw, c.clip, cov3d=_precomp(c))


@functools.lru_cache(maxsize=None)
def oracle_forward(name):
    c = PC.case(name)
    return dict(zip(FWD, O.project_gaussians_forward(*c.forward_args(), cov3d_precomp=_precomp(c))))


@functools.lru_cache(maxsize=None)
def golden(name):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "project.npz")
    with np.load(path) as z:
        return {k.split("__", 1)[1]: z[k] for k in z.files if k.startswith(name + "__")}


@functools.lru_cache(maxsize=None)
def golden_fp64(name):
    """float64 on the rows the reference's torch code ran."""
    c, g = PC.case(name), golden(name)
    return PR.project_forward_fp64(g["means3d"], g["scales"], c.glob_scale, g["quats"], c.viewmat, c.projmat, c.fx,
                                   c.fy, c.cx, c.cy, c.H, c.W, c.bw, c.clip)


@functools.lru_cache(maxsize=None)
def fp32_distance():
    """{(case, output): the largest per-row distance of the reference's fp32 results from float64, relative to the
    row's largest magnitude} -- the table of DESIGN.md, "Projection: distance of an fp32 implementation from float64"
    (run this module with -s to print it)."""
    out = {}
    for name in PC.names(in_golden=True):
        g, f = golden(name), golden_fp64(name)
        vis = f["visible"] & g["mask"]
        for k in PR.OUTPUTS:
            out[name, k] = float((PR.row_err(g[k][vis], f[k][vis]) / PR.row_max(f[k][vis])).max())
            print(f"fp32 reference vs float64, {name} {k}: {out[name, k]:.2e}")
    return out


def bar(name, output):
    """The measured distance for the case; the largest over the cases the torch code can run for the others."""
    d = fp32_distance()
    return d[name, output] if (name, output) in d else max(v for (_, k), v in d.items() if k == output)


@pytest.mark.parametrize("name", PC.names())
def test_cases_keep_their_populations(name):
    c, f = PC.case(name), fp64_forward(name)
    vis, clamped = float(f["visible"].mean()), float((f["visible"] & f["clamped"]).mean())
    print(f"{name}: n {c.n}, visible {vis:.3f}, visible and clamped {clamped:.3f}, ambiguous "
          f"{float(f['ambiguous'].mean()):.4f} " + str({k: int(v.sum()) for k, v in f["why"].items()}))
    assert c.min_visible <= vis <= c.max_visible
    assert clamped >= c.min_clamped_visible
    if name.endswith("-exact"):
        # tz == clip to the bit: on the boundary by construction (and exactly so in any precision: identity view)
        assert f["why"]["near_plane"].all() and c.n == 16
    else:
        assert f["ambiguous"].mean() <= 0.02


@pytest.mark.parametrize("name", PC.names(in_golden=True))
def test_golden_inputs_are_rows_of_the_cases(name):
    c, g = PC.case(name), golden(name)
    for k in ("means3d", "scales", "quats"):
        assert np.array_equal(g[k], getattr(c, k)[g["rows"]]), k
    assert np.array_equal(g["viewmat"], c.viewmat) and np.array_equal(g["projmat"], c.projmat)
    assert np.array_equal(g["intrinsics"], [c.fx, c.fy, c.cx, c.cy]) and list(g["img_size"]) == [c.W, c.H]
    assert int(g["block_width"]) == c.bw and float(g["glob_scale"]) == np.float32(c.glob_scale)
    assert float(g["clip_thresh"]) == np.float32(c.clip)


@pytest.mark.parametrize("name", PC.names(in_golden=True))
def test_fp64_forward_equals_the_reference_golden(name):
    """Floats per row: an fp32 evaluation rounds every operation to one part in 2^24 and the chain to an output is
    some tens of operations long, so a row may be 64 x 2^-24 of its largest magnitude away -- times the factor by
    which the row's own cancellations amplify rounding (projection_reference.forward_condition_fp64: float64 alone)."""
    c, g, f = PC.case(name), golden(name), golden_fp64(name)
    ok = ~f["ambiguous"]
    assert np.array_equal(g["mask"][ok], f["visible"][ok])
    assert np.array_equal(g["radii"][ok], f["radii"][ok])
    assert np.array_equal(g["num_tiles_hit"][ok], f["num_tiles_hit"][ok])
    cond = PR.forward_condition_fp64(g["means3d"], g["scales"], c.glob_scale, g["quats"], c.viewmat, c.projmat, c.fx,
                                     c.fy, c.cx, c.cy, c.H, c.W)
    vis = f["visible"] & g["mask"]
    assert vis.sum() >= 40
    for k in PR.OUTPUTS:
        e = PR.row_err(g[k][vis], f[k][vis]) / PR.row_max(f[k][vis])
        allowed = 64 * 2.0 ** -24 * np.maximum(1.0, cond[k][vis] if k in cond else 1.0)
        print(f"{name} {k}: reference vs float64 per row {e.max():.2e}, {float((e / allowed).max()):.2f} of the bound")
        assert (e <= allowed).all(), f"{k}: {float((e / allowed).max()):.2f} of the bound"
    assert np.all(g["xys"][~g["mask"]] == 0) and np.all(f["xys"][~f["visible"]] == 0)


@pytest.mark.parametrize("name", PC.names(in_golden=True))
def test_fp64_vjp_equals_the_reference_golden(name):
    """The reference's fp32 autograd for the cotangents g_xys / g_conics, on the guard band's visible rows: the rule of
    tests/test_project_fp64.py::test_fp64_projection_vjp_equals_the_goldens (2e-3 per element, floored at 1e-3 of the
    largest).  g_quats is the gradient with respect to the unit quaternion (make_golden_project.py)."""
    c, g, f = PC.case(name), golden(name), golden_fp64(name)
    ref = PR.project_vjp_fp64(g["means3d"], g["scales"], c.glob_scale, g["quats"], c.viewmat[:3], c.projmat, c.fx, c.fy,
                              c.cx, c.cy, c.H, c.W, None, g["g_xys"], None, g["g_conics"], None)
    rows = g["mask"] & f["visible"] & ref[3]
    assert rows.sum() >= 30
    for mine, key in zip(ref[:3], ("g_means3d", "g_scales", "g_quats")):
        gold = g[key][rows].astype(np.float64)
        floor = 1e-3 * max(1.0, float(np.abs(gold).max()))
        e = np.abs(mine[rows] - gold) / np.maximum(np.abs(gold), floor)
        print(f"{name} {key}: float64 vs the reference's autograd {e.max():.2e} on {int(rows.sum())} rows")
        assert e.max() < 2e-3, f"{key}: {e.max():.3e}"


@pytest.mark.parametrize("name", PC.names())
def test_oracle_forward_against_fp64(name):
    c, f, o = PC.case(name), fp64_forward(name), oracle_forward(name)
    ok = ~f["ambiguous"]
    vis_o = o["radii"] > 0
    assert np.array_equal(vis_o[ok], f["visible"][ok])
    assert np.array_equal(o["radii"][ok], f["radii"][ok])
    assert np.array_equal(o["num_tiles_hit"][ok], f["num_tiles_hit"][ok])
    for k in ("xys", "depths", "compensation", "num_tiles_hit"):  # what the consumers read of a culled Gaussian
        assert np.all(o[k][~vis_o] == 0), k
    vis = vis_o & f["visible"]
    for k in PR.OUTPUTS:
        if not vis.any():
            break
        e, fm = PR.row_err(o[k][vis], f[k][vis]), PR.row_max(f[k][vis])
        allowed = 2 * bar(name, k) * fm + 1e-6 * fm
        print(f"{name} {k}: oracle vs float64 per row {float((e / fm).max()):.2e}, "
              f"{float((e / allowed).max()):.2f} of the bar")
        assert (e <= allowed).all(), f"{k}: {float((e / allowed).max()):.2f} of the bar"
    if c.precomputed:
        assert np.array_equal(o["cov3d"], c.cov3d)  # handed in, handed back


@pytest.mark.parametrize("name", PC.names(max_visible=0.0))
def test_rows_on_the_near_plane_are_culled(name):
    """tz == clip_thresh to the bit: culled (`z <= clip`, helpers.cuh:212-219; the torch restatement's `<` keeps them)."""
    c, f, o = PC.case(name), fp64_forward(name), oracle_forward(name)
    assert np.array_equal(c.means3d[:, 2], np.full(16, np.float32(c.clip)))
    assert not f["visible"].any() and not (o["radii"] > 0).any() and not o["num_tiles_hit"].any()
    for k in ("xys", "depths", "conics", "compensation"):
        assert not o[k].any() and not f[k].any(), k


def oracle_vjp(c, o, cot):
    sq = (None, None) if c.precomputed else (c.scales, c.quats)
    out = O.project_gaussians_backward(c.n, c.means3d, sq[0], c.glob_scale, sq[1], c.viewmat[:3], c.projmat, c.fx, c.fy,
                                       c.cx, c.cy, c.H, c.W, o["cov3d"], o["radii"], o["conics"], o["compensation"],
                                       *cot)
    return out  # (v_cov2d, v_cov3d, v_mean3d, v_scale, v_quat)


def fp64_vjp(c, comp, cot):
    """-> ({name: float64 gradient}, guard)"""
    sq = (None, None) if c.precomputed else (c.scales, c.quats)
    r = PR.project_vjp_fp64(c.means3d, sq[0], c.glob_scale, sq[1], c.viewmat[:3], c.projmat, c.fx, c.fy, c.cx, c.cy,
                            c.H, c.W, comp, *cot, cov3d=_precomp(c))
    names = ("v_mean3d", "v_cov3d") if c.precomputed else ("v_mean3d", "v_scale", "v_quat")
    return dict(zip(names, r[:-1])), r[-1]


@pytest.mark.parametrize("which", list(COTANGENTS))
@pytest.mark.parametrize("name", PC.names(max_visible=1.0) + PC.names(max_visible=0.5))
def test_oracle_vjp_against_fp64_inside_the_guard_band(name, which):
    """The 1e-5 per-row rule of test_project_fp64.py::test_fp64_projection_vjp_equals_the_oracle_on_a_well_conditioned_
    scene, for each cotangent alone (the others None) and all together; with the compensation's cotangent in play only
    rows with compensation < 0.9 (that test's reason: the oracle forms 1 - compensation^2), of which more than 20 %
    of the comparable rows must remain.

    The bar is one for well-conditioned rows; tests/projection_cases.py says how the cases are kept that (definite
    axis ratios, no splat below a fifth of a pixel: the compensation of every compared row is above 0.1, asserted)."""
    c, o = PC.case(name), oracle_forward(name)
    cot = tuple(v if keep else None for v, keep in zip(PC.cotangents(c), COTANGENTS[which]))
    ref, guard = fp64_vjp(c, o["compensation"], cot)
    orc = dict(zip(("v_cov2d", "v_cov3d", "v_mean3d", "v_scale", "v_quat"), oracle_vjp(c, o, cot)))
    rows = (o["radii"] > 0) & guard
    comparable = int(rows.sum())
    assert comparable >= min(c.n, 100) * 0.3
    if COTANGENTS[which][3]:
        rows &= o["compensation"] < 0.9
        assert rows.sum() > 0.2 * comparable and (o["compensation"][rows] > 0.1).all()
    for nm, f in ref.items():
        assert np.all(orc[nm][o["radii"] <= 0] == 0), nm
        e = PR.row_err(orc[nm][rows], f[rows]) / np.maximum(PR.row_max(f[rows]), 1e-12)
        print(f"{name} {which} {nm}: oracle vs float64 per row {e.max():.2e} on {int(rows.sum())} rows")
        assert e.max() < 1e-5, f"{nm}: {e.max():.3e}"


def test_fp64_vjp_without_cotangents_is_zero():
    c = PC.case("blockedge-257")
    ref, _ = fp64_vjp(c, oracle_forward(c.name)["compensation"], (None, None, None, None))
    assert all(not g.any() for g in ref.values())
    orc = oracle_vjp(c, oracle_forward(c.name), (None, None, None, None))
    assert all(not g.any() for g in orc)
