"""GPU: surface distance (gs_fusion.MeshDistance, csrc/mesh_distance.hip) against the float64 brute force of
tests/surface_distance_reference.py, the float32 restatement, the exhaustive kernel and the toolkit tool's recorded output.

Held at every case (`_held`): |d_gpu - d64| <= tol with tol = 4 r 2^-24 S (r = 3.36, measured and pinned by
tests/test_surface_distance_host.py; S the largest |coordinate| of the inputs); the returned face's own float64 distance
<= d64 + tol (faces are never compared by index); the exhaustive path bit-equal to the float32 restatement's minimum;
the tree's result >= the exhaustive one and within tol of it (the number of results that differ in bits is printed;
the prune slack is derived to make it 0); the closest point on the returned face and |closest - p| = d within tol;
guard rows around every output untouched; tree and workspaces handed in pre-filled with 0xFF.
"""
import functools
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import surface_distance_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "surface_distance")
GUARD = -7.0


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _dirty(nbytes):
    return torch.full((max(int(nbytes), 1),), 0xFF, dtype=torch.uint8, device=DEV)


def _build(v, t):
    """MeshDistance on a tree buffer and a workspace full of 0xFF."""
    from gs_fusion import MeshDistance
    from gs_fusion.distance import BYTES_BUILD, BYTES_TREE, _bytes

    F = len(t)
    return MeshDistance(_t(v), _t(t), _tree=_dirty(_bytes(BYTES_TREE, F, 0)), _workspace=_dirty(_bytes(BYTES_BUILD, F, 0)))


@functools.lru_cache(maxsize=None)
def _mesh(name):
    v, t, _ = R.case(name)
    return _build(v, t)


def _query(mesh, p, exhaustive):
    """-> (d, face, closest) as NumPy, through outputs with a guard row either side and a 0xFF workspace."""
    from gs_fusion.distance import BYTES_QUERY, _bytes

    n = len(p)
    d = torch.full((n + 2,), GUARD, dtype=torch.float32, device=DEV)
    f = torch.full((n + 2,), int(GUARD), dtype=torch.int32, device=DEV)
    c = torch.full((n + 2, 3), GUARD, dtype=torch.float32, device=DEV)
    ws = None if exhaustive or n == 0 else _dirty(_bytes(BYTES_QUERY, 0, n))
    out = mesh.query(_t(p), return_closest=True, exhaustive=exhaustive, _workspace=ws, _out=(d[1:-1], f[1:-1], c[1:-1]))
    torch.cuda.synchronize()
    assert out[0].data_ptr() == d[1:-1].data_ptr()
    for buf in (d, f, c):
        assert bool((buf[0] == GUARD).all()) and bool((buf[-1] == GUARD).all()), "a guard row was written"
    return d[1:-1].cpu().numpy(), f[1:-1].cpu().numpy(), c[1:-1].cpu().numpy()


def _held(name, n=None, what=""):
    """Everything the header lists, for the first n points of a named case -> (d_tree, face_tree, tol)."""
    v, t, p = R.case(name)
    p = p[:n]
    d64, d32 = R.truth(name)[0][:len(p)], R.restated(name)[0][:len(p)]
    tol = R.tolerance(p, v, t)
    ok = np.isfinite(d64)
    mesh = _mesh(name)
    keep = R.usable(v, t)
    got = {}
    for path in ("exhaustive", "tree"):
        d, f, c = got[path] = _query(mesh, p, path == "exhaustive")
        label = f"{name} {what} {path}"
        assert d.dtype == np.float32 and f.dtype == np.int32 and d.shape == (len(p),) and c.shape == (len(p), 3)
        assert np.array_equal(np.isfinite(d), ok) and np.isnan(d[~ok]).all() and (f[~ok] == -1).all(), label
        assert np.isnan(c[~ok]).all(), label
        err = np.abs(d[ok].astype(np.float64) - d64[ok])
        print(f"{label}: n={len(p)} F={len(t)} max |d - d64| = {err.max(initial=0):.3e}, tol = {tol:.3e}")
        assert (err <= tol).all(), label
        assert ((f[ok] >= 0) & (f[ok] < len(t))).all() and keep[f[ok]].all(), label
        own = R.face_distance(p[ok], v, t, f[ok])
        assert (own <= d64[ok] + tol).all(), label
        assert (np.abs(np.sqrt(((c[ok].astype(np.float64) - p[ok]) ** 2).sum(1)) - d64[ok]) <= 2 * tol).all(), label
        assert (R.face_distance(c[ok], v, t, f[ok]) <= 2 * tol).all(), label
    de, dt = got["exhaustive"][0], got["tree"][0]
    differ = int((_bits(de[ok]) != _bits(d32[ok])).sum())
    print(f"{name} {what}: exhaustive differs from the float32 restatement in {differ} of {int(ok.sum())} results")
    assert differ == 0
    differ = int((_bits(de[ok]) != _bits(dt[ok])).sum())
    print(f"{name} {what}: tree differs from exhaustive in {differ} of {int(ok.sum())} results")
    assert (dt[ok] >= de[ok]).all() and (dt[ok].astype(np.float64) - de[ok] <= tol).all()
    return got["tree"][0], got["tree"][1], tol


# ---- 1 shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SHAPE_N)
@pytest.mark.parametrize("F", R.SHAPE_F)
def test_shapes(F, n):
    _held(f"shape {F}", n, f"n={n}")


# ---- 2 one triangle, all seven regions; equidistant triangles ----------------------------------------------------------
def test_seven_regions_and_ties():
    d, f, tol = _held("seven regions")
    want = np.array([w for _, w in R.SEVEN_POINTS])
    assert (np.abs(d - want) <= tol).all()
    assert (d[:4] == np.float32([0.5, 5, 1, 2])).all() and (d[8:13] == 0).all()  # dyadic: exact
    d, f, tol = _held("two triangles")
    assert set(f.tolist()) <= {0, 1}


# ---- 3 trees that break naive builders ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["identical", "line", "plane", "one large"])
def test_awkward_trees(name):
    _held(name)


# ---- 4 degenerate and poisoned input -----------------------------------------------------------------------------------
def test_degenerate_triangles():
    d, f, tol = _held("degenerate")
    assert np.isfinite(d).all()
    v, t, p = R.case("degenerate")
    only = _build(v, t[60:])  # the collinear and single-point triangles alone: the segment / point rule, exactly
    for exhaustive in (False, True):
        got = _query(only, p[100:106], exhaustive)[0]
        assert (got == np.float32([0.5, 2.0, 1.0, 0.5, 0.25, 2.0])).all(), got


def test_poisoned_input():
    from gs_fusion import surface_distance

    d, f, tol = _held("poisoned")
    v, t, p = R.case("poisoned")
    mesh = _mesh("poisoned")
    assert mesh.skipped_triangles == len(R.POISONED_TRIANGLES)
    assert tuple(np.nonzero(np.isnan(d))[0]) == R.POISONED_POINTS and not np.isin(f, R.POISONED_TRIANGLES).any()
    clean = np.delete(p, R.POISONED_POINTS, 0)
    alone = _query(mesh, clean, False)[0]
    assert np.array_equal(_bits(alone), _bits(np.delete(d, R.POISONED_POINTS)))  # neighbours unaffected
    s = mesh.stats(_t(d), 0.1)
    assert s["invalid"] == len(R.POISONED_POINTS) and s["count"] == len(p) - len(R.POISONED_POINTS)
    assert s == surface_distance(_t(p), _t(v), _t(t), 0.1)


def test_bad_meshes_and_no_points():
    from gs_fusion import MeshDistance
    from rasterizer.cuda._backend import lib

    v, t, p = R.case("shape 257")
    dv, dp = _t(v), _t(p[:10])
    for bad in (-1, len(v)):
        t2 = t.copy()
        t2[[40, 200], [1, 2]] = bad
        with pytest.raises(ValueError, match=r"triangle 40 has a vertex index outside \[0, %d\)" % len(v)):
            MeshDistance(dv, _t(t2))
        assert b"triangle 40" in lib().gsr_last_error()
    with pytest.raises(ValueError):
        MeshDistance(dv, _t(t[:0]))
    with pytest.raises(ValueError):
        MeshDistance(torch.full_like(dv, float("nan")), _t(t))
    torch.cuda.synchronize()
    mesh = _mesh("shape 257")  # and the device is fine afterwards
    for exhaustive in (False, True):
        d, f, c = mesh.query(dp[:0], return_closest=True, exhaustive=exhaustive)
        assert d.shape == (0,) and f.shape == (0,) and c.shape == (0, 3) and f.dtype == torch.int32
    s = mesh.stats(d)
    assert s["count"] == 0 and s["invalid"] == 0 and s["mean"] == 0 and s["within_threshold"] is None
    for args in ((dv.double(), _t(t)), (dv, _t(t).long()), (dv.cpu(), _t(t)), (dv, _t(t).cpu()), (dv[:, :2].contiguous(), _t(t)),
                 (dv, _t(t).reshape(-1))):
        with pytest.raises(RuntimeError):
            MeshDistance(*args)
    for q in (dp.double(), dp.cpu(), dp[:, :2].contiguous(), dp.t().contiguous().t()):
        with pytest.raises(RuntimeError):
            mesh.query(q)
    with pytest.raises(ValueError):
        mesh.stats(mesh.query(dp)[0], -1.0)
    q = lib().gsr_mesh_distance_workspace_bytes
    assert q(0, 0, 0) == 0 and q(0, (1 << 28) + 1, 0) == 0 and q(2, 0, 0) == 0 and q(3, 0, -1) == 0 and q(9, 5, 5) == 0
    assert 0 < q(0, 1, 0) < q(0, 1000, 0) and 0 < q(1, 1, 0) < q(1, 100000, 0) and 0 < q(2, 0, 1) < q(2, 0, 100000)
    assert len(_query(mesh, p[:10], False)[0]) == 10


# ---- 5 precision -------------------------------------------------------------------------------------------------------
def test_far_from_the_origin():
    v, t, p = R.case("far")
    assert 1000 < R.scale_of(p, v, t) < 1002
    _held("far")


# ---- 6 medium, on the device only --------------------------------------------------------------------------------------
def test_medium_tree_against_exhaustive():
    v, t, p = R.medium()
    assert len(t) == 50000 and len(p) == 100000
    tol = R.tolerance(p, v, t)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mesh = _build(v, t)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    dp = _t(p)
    mesh.query(dp)  # (warm-up of the shape)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    dt, ft = mesh.query(dp)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    de, fe = mesh.query(dp, exhaustive=True)
    torch.cuda.synchronize()
    t4 = time.perf_counter()
    print(f"medium: build {1e3 * (t1 - t0):.2f} ms (with allocation), tree query {1e3 * (t3 - t2):.2f} ms, "
          f"exhaustive {1e3 * (t4 - t3):.2f} ms")
    dt, de, ft = dt.cpu().numpy(), de.cpu().numpy(), ft.cpu().numpy()
    differ = int((_bits(dt) != _bits(de)).sum())
    print(f"medium: tree differs from exhaustive in {differ} of {len(p)} results")
    assert np.isfinite(de).all() and (dt >= de).all() and (dt.astype(np.float64) - de <= tol).all()
    rows = np.arange(0, len(p), 500)  # a sample against float64
    d64 = R.distance(p[rows], v, t)[0]
    assert (np.abs(dt[rows] - d64) <= tol).all() and (R.face_distance(p[rows], v, t, ft[rows]) <= d64 + tol).all()


# ---- 7 statistics ------------------------------------------------------------------------------------------------------
def test_statistics():
    from gs_fusion import distance_stats
    from gs_fusion.distance import BYTES_STATS, _bytes

    g = np.random.default_rng(3)
    for n in (1, 255, 257, 300001):
        d = g.uniform(0, 2, n).astype(np.float32)
        if n > 1:
            d[g.integers(0, n, max(n // 50, 1))] = np.nan
            d[1] = np.inf
        tau = 0.75
        ok = np.isfinite(d)
        x = d[ok].astype(np.float64)
        want = {"count": int(ok.sum()), "invalid": int((~ok).sum()), "mean": x.mean(), "rms": np.sqrt((x * x).mean()),
                "max": x.max(), "within_threshold": int((d[ok] <= np.float32(tau)).sum()), "sum": x.sum(),
                "sum_squares": (x * x).sum()}
        dd = _t(d)
        a = distance_stats(dd, tau)
        b = distance_stats(dd, tau, _workspace=_dirty(_bytes(BYTES_STATS, 0, n)))
        assert a == b, n  # two runs, one on a dirty workspace: the same bits
        for k, w in want.items():
            assert a[k] == w if isinstance(w, int) else abs(a[k] - w) <= 1e-12 * abs(w), (n, k, a[k], w)
        assert distance_stats(dd)["within_threshold"] is None
    a = distance_stats(_t(np.float32([np.nan, np.nan])), 1.0)
    assert a["count"] == 0 and a["invalid"] == 2 and a["mean"] == 0 and a["max"] == 0 and a["within_threshold"] == 0
    d1 = _query(_mesh("shape 4096"), R.case("shape 4096")[2], False)[0]
    d2 = _query(_mesh("shape 4096"), R.case("shape 4096")[2], False)[0]
    assert np.array_equal(_bits(d1), _bits(d2))


# ---- 8 golden ----------------------------------------------------------------------------------------------------------
def _fixture(name):
    from gs_io import read_mesh_ply, read_stl

    e = json.load(open(os.path.join(GOLDEN, "expected.json")))[name]
    tri = read_stl(os.path.join(GOLDEN, e["ground_truth"]))
    p = read_mesh_ply(os.path.join(GOLDEN, e["points"]))["vertices"]
    return e, tri.reshape(-1, 3), np.arange(3 * len(tri), dtype=np.int32).reshape(-1, 3), p


@pytest.mark.parametrize("name", ["soup", "sphere", "decades"])
def test_golden_average_error(name):
    from gs_fusion import surface_distance

    e, v, t, p = _fixture(name)
    s = surface_distance(_t(p), _t(v), _t(t))
    unit = 10.0 ** (np.floor(np.log10(float(e["average_error"]))) - 5)  # one unit of the sixth significant digit
    tol = R.tolerance(p, v, t)
    print(f"{name}: GPU mean {s['mean']!r}, the tool printed {e['average_error']}, tol {tol:.2e}")
    assert abs(s["mean"] - float(e["average_error"])) <= tol + 0.5 * unit
    assert s["count"] == len(p) and s["invalid"] == 0


# ---- 9 tool ------------------------------------------------------------------------------------------------------------
def test_command_line(tmp_path):
    from gs_io import write_mesh_ply

    e, v, t, p = _fixture("soup")
    tool = os.path.join(ROOT, "tools", "eval_surface.py")

    def run(*args):
        res = subprocess.run(["timeout", "-k", "10", "300", sys.executable, tool, *args], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
        return json.loads(res.stdout.strip().splitlines()[-1])

    tol = R.tolerance(p, v, t)
    for gt in (e["ground_truth"],):  # (the ASCII twin holds the same triangles: tests/test_surface_distance_host.py)
        row = run("--gt", os.path.join(GOLDEN, gt), "--mesh", os.path.join(GOLDEN, e["points"]), "--threshold", "0.1")
        assert abs(row["average_error"] - float(e["average_error"])) <= tol + 0.5e-6
        assert row["invalid"] == 0 and 0 < row["within_threshold"] < len(p) and row["max"] >= row["rms"] >= row["average_error"]
        assert not any(k.startswith("completeness_") for k in row)
    # both directions: a generated mesh with faces (the sphere, moved a little) against the sphere fixture
    sv, st = R.sphere(2)
    moved = (sv * np.float32(1.05) + np.float32([0.01, 0, 0])).astype(np.float32)
    write_mesh_ply(str(tmp_path / "mesh.ply"), moved, st)
    row = run("--gt", os.path.join(GOLDEN, "sphere.stl"), "--mesh", str(tmp_path / "mesh.ply"), "--both")
    gv, gt_ = _fixture("sphere")[1:3]
    tol = R.tolerance(moved, gv, gt_)
    assert abs(row["average_error"] - R.distance(moved, gv, gt_)[0].mean()) <= tol
    assert abs(row["completeness_average_error"] - R.distance(gv, moved, st)[0].mean()) <= tol
    assert row["within_threshold"] is None and row["completeness_invalid"] == 0
