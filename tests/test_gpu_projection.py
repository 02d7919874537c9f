"""GPU: csrc/project.hip, through `rasterizer.cuda`, on the cases of tests/projection_cases.py -- anamorphic and
off-centre cameras, glob_scale != 1, the near plane, the guard band, raw quaternions, covariances handed in, the
block edges of the one-lane-per-Gaussian launch -- against the C oracle (forward: bit-identical, the project's rule;
backward: 1e-3 per row) and the float64 restatement (tests/projection_reference.py; backward: stage (c)'s rule of
tests/test_gpu_heldout.py).  tests/test_projection_host.py holds the oracle itself to float64 and to the reference."""
import functools

import numpy as np
import pytest
import torch

import projection_cases as PC
import projection_reference as PR
from oracle import oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FWD = ("cov3d", "xys", "depths", "radii", "conics", "compensation", "num_tiles_hit")
BWD = ("v_cov2d", "v_cov3d", "v_mean3d", "v_scale", "v_quat")
RUNNABLE = [n for n in PC.names() if not n.endswith("-exact")]  # (cases with visible rows: the backward's)


def cu(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def npy(t):
    return None if t is None else t.detach().cpu().numpy()


def gpu_forward(c, cov3d_precomp=None, scales="case", glob=None):
    import rasterizer.cuda as C

    a = list(c.forward_args())
    if not isinstance(scales, str):
        a[2] = scales
    if glob is not None:
        a[3] = glob
    a = [cu(x) if isinstance(x, np.ndarray) else x for x in a]
    return C.project_gaussians_forward(*a, **({} if cov3d_precomp is None else {"cov3d_precomp": cov3d_precomp}))


@functools.lru_cache(maxsize=None)
def oracle_forward(name):
    c = PC.case(name)
    return dict(zip(FWD, O.project_gaussians_forward(*c.forward_args(),
                                                     cov3d_precomp=c.cov3d if c.precomputed else None)))


def gpu_backward(c, o, cot, precomputed=None, scales="case", glob=None):
    import rasterizer.cuda as C

    pre = c.precomputed if precomputed is None else precomputed
    sc = c.scales if isinstance(scales, str) else scales
    sq = (None, None) if pre else (cu(sc), cu(c.quats))
    out = C.project_gaussians_backward(c.n, cu(c.means3d), sq[0], c.glob_scale if glob is None else glob, sq[1],
                                       cu(c.viewmat[:3]), cu(c.projmat), c.fx, c.fy, c.cx, c.cy, c.H, c.W,
                                       cu(o["cov3d"]), cu(o["radii"]), cu(o["conics"]), cu(o["compensation"]),
                                       *(cu(v) for v in cot))
    return dict(zip(BWD, (npy(t) for t in out)))


def oracle_backward(c, o, cot):
    sq = (None, None) if c.precomputed else (c.scales, c.quats)
    return dict(zip(BWD, O.project_gaussians_backward(
        c.n, c.means3d, sq[0], c.glob_scale, sq[1], c.viewmat[:3], c.projmat, c.fx, c.fy, c.cx, c.cy, c.H, c.W,
        o["cov3d"], o["radii"], o["conics"], o["compensation"], *cot)))


@pytest.mark.parametrize("name", PC.names())
def test_forward_is_bit_identical_to_the_oracle(name):
    c, r = PC.case(name), oracle_forward(name)
    handed = cu(c.cov3d) if c.precomputed else None
    o = dict(zip(FWD, gpu_forward(c, cov3d_precomp=handed)))
    if c.precomputed:
        assert o["cov3d"] is handed and np.array_equal(npy(handed), c.cov3d)  # the caller's, untouched
    o = {k: npy(v) for k, v in o.items()}
    for k in FWD:
        assert np.array_equal(o[k], r[k]), f"{k}: {(o[k] != r[k]).sum()} elements differ"
    cul = o["radii"] == 0
    assert c.min_visible <= 1.0 - cul.mean() <= c.max_visible
    for k in ("xys", "depths", "compensation", "num_tiles_hit"):
        assert np.all(o[k][cul] == 0), k


@pytest.mark.parametrize("name", RUNNABLE)
def test_backward_against_the_oracle_and_fp64(name):
    c, o = PC.case(name), oracle_forward(name)
    cot = PC.cotangents(c)
    hip, orc = gpu_backward(c, o, cot), oracle_backward(c, o, cot)
    radii = o["radii"]
    for nm in BWD:
        if c.precomputed and nm in ("v_scale", "v_quat"):
            assert hip[nm] is None
            continue
        h, r = hip[nm], orc[nm]
        assert np.all(h[radii <= 0] == 0), nm
        rowmax = np.abs(r).max(axis=-1, keepdims=True)
        e = np.abs(h - r) / np.maximum(rowmax, 1e-6 * np.abs(r).max())
        print(f"{name} {nm}: HIP vs oracle per row {e.max():.3e}")
        assert e.max() < 1e-3, f"{nm}: {e.max():.3e}"
    # float64, on the guard band's rows: HIP no further from it than twice the oracle, plus 1e-6 of the row
    sq = (None, None) if c.precomputed else (c.scales, c.quats)
    f64 = PR.project_vjp_fp64(c.means3d, sq[0], c.glob_scale, sq[1], c.viewmat[:3], c.projmat, c.fx, c.fy, c.cx, c.cy,
                              c.H, c.W, o["compensation"], *cot, cov3d=c.cov3d if c.precomputed else None)
    rows = (radii > 0) & f64[-1]
    assert rows.sum() >= 0.3 * min(c.n, 100)
    for nm, f in zip(("v_mean3d", "v_cov3d") if c.precomputed else ("v_mean3d", "v_scale", "v_quat"), f64[:-1]):
        eh, eo, fm = PR.row_err(hip[nm][rows], f[rows]), PR.row_err(orc[nm][rows], f[rows]), PR.row_max(f[rows])
        print(f"{name} {nm}: vs fp64 per row, HIP {float((eh / np.maximum(fm, 1e-30)).max()):.3e}, oracle "
              f"{float((eo / np.maximum(fm, 1e-30)).max()):.3e} on {int(rows.sum())} rows")
        over = eh > 2 * eo + 1e-6 * fm
        assert not over.any(), f"{nm}: {int(over.sum())} rows further from fp64 than the oracle allows"


@pytest.mark.parametrize("name", ["everything", "everything-precomputed", "blockedge-257"])
def test_a_null_cotangent_is_a_zero_cotangent(name):
    c, o = PC.case(name), oracle_forward(name)
    cot = PC.cotangents(c)
    for k in range(4):
        null = gpu_backward(c, o, tuple(None if j == k else v for j, v in enumerate(cot)))
        zero = gpu_backward(c, o, tuple(np.zeros_like(v) if j == k else v for j, v in enumerate(cot)))
        for nm in BWD:
            assert (null[nm] is None and zero[nm] is None) or np.array_equal(null[nm], zero[nm]), (k, nm)
    none = gpu_backward(c, o, (None, None, None, None))
    assert all(v is None or not v.any() for v in none.values())


def test_precomputed_covariances_end_the_chain_at_v_cov3d():
    import rasterizer.cuda as C

    c = PC.case("everything")
    full = dict(zip(FWD, (npy(t) for t in gpu_forward(c))))
    handed = cu(full["cov3d"])
    a = [cu(x) if isinstance(x, np.ndarray) else x for x in c.forward_args()]
    a[2] = a[4] = None
    pre = dict(zip(FWD, (npy(t) for t in C.project_gaussians_forward(*a, cov3d_precomp=handed))))
    for k in FWD:
        assert np.array_equal(pre[k], full[k]), k
    cot = PC.cotangents(c)
    g_full, g_pre = gpu_backward(c, full, cot), gpu_backward(c, full, cot, precomputed=True)
    assert g_pre["v_scale"] is None and g_pre["v_quat"] is None  # no such buffers were handed to the kernel
    for nm in ("v_cov2d", "v_cov3d", "v_mean3d"):
        assert np.array_equal(g_pre[nm], g_full[nm]), nm
    assert g_full["v_cov3d"][full["radii"] > 0].any()


@pytest.mark.parametrize("g", [0.25, 4.0])
def test_glob_scale_folds_into_the_scales(g):
    """A power of two: glob_scale * s is exact, so project(s, g) and project(g s, 1) see the same numbers."""
    c = PC.case("anamorphic-317x203-bw16")
    a = dict(zip(FWD, (npy(t) for t in gpu_forward(c, glob=g))))
    b = dict(zip(FWD, (npy(t) for t in gpu_forward(c, scales=(c.scales * np.float32(g)), glob=1.0))))
    for k in FWD:
        assert np.array_equal(a[k], b[k]), k
    assert (a["radii"] > 0).mean() > 0.9
    cot = PC.cotangents(c)
    ga = gpu_backward(c, a, cot, glob=g)
    gb = gpu_backward(c, a, cot, scales=c.scales * np.float32(g), glob=1.0)
    assert np.array_equal(ga["v_scale"], gb["v_scale"] * np.float32(g)) and ga["v_scale"].any()
    for nm in ("v_cov2d", "v_cov3d", "v_mean3d", "v_quat"):
        assert np.array_equal(ga[nm], gb[nm]), nm


def test_cov2d_bounds_on_near_singular_and_boundary_inputs():
    import rasterizer.cuda as C

    rng = np.random.default_rng(4)
    n = 1000
    a, c = rng.uniform(0.3, 50, n), rng.uniform(0.3, 50, n)
    b = rng.uniform(-0.9, 0.9, n) * np.sqrt(a * c)
    near = rng.choice([-1.0, 1.0], n) * (1.0 - 10.0 ** rng.uniform(-6, -1, n)) * np.sqrt(a * c)  # up to 0.999999
    a3 = np.where(np.arange(n) % 2 == 0, 0.3, a)  # a or c at the blur's 0.3 exactly
    c3 = np.where(np.arange(n) % 2 == 1, 0.3, c)
    sing = np.stack([[1.0, 1.0, 1.0], [4.0, 2.0, 1.0], [0.25, -0.5, 1.0], [0.0, 0.0, 0.0], [2.0, 0.0, 0.0]])
    cov = np.concatenate([np.stack([a, b, c], -1), np.stack([a, near, c], -1),
                          np.stack([a3, rng.uniform(-0.9, 0.9, n) * np.sqrt(a3 * c3), c3], -1), sing]).astype(np.float32)
    det32 = cov[:, 0] * cov[:, 2] - cov[:, 1] * cov[:, 1]
    assert (det32[-len(sing):] == 0).all()  # det == 0 exactly, in fp32 as in float64
    m = len(cov)
    ref = O.compute_cov2d_bounds(m, cov)
    got = C.compute_cov2d_bounds(m, cu(cov))
    assert got[1].shape == (m, 1)
    conics, radii = npy(got[0]), npy(got[1])
    # the kernel and the oracle share gsr_cov2d_bounds' expression order (-ffp-contract=off on both sides)
    assert np.array_equal(conics, ref[0]) and np.array_equal(radii, ref[1])
    k64, _, r64, valid, ambiguous = PR.cov2d_bounds_fp64(cov)
    assert not valid[-len(sing):].any() and not conics[-len(sing):].any() and not radii[-len(sing):].any()
    ok = valid & ~ambiguous
    assert ok.mean() > 0.98 and np.array_equal(radii[ok, 0], r64[ok])
