"""GPU: k nearest neighbours (gs_fused.KNN, csrc/knn.hip) against the float64 brute force and the float32 restatement
of tests/knn_reference.py, the exhaustive kernel, and the reference's recorded output (tests/golden/knn.npz).

Held at every case (`_held`): |d_gpu - d64| <= 4 r 2^-24 d64 (r = 3.08, measured and pinned by tests/test_knn_host.py);
the returned index's own float64 distance within that of the k-th d64; the exhaustive path bit-equal to the float32
restatement, indices included; the tree bit-equal to the exhaustive path, indices included; rows ascending; no self
index in self mode; guard rows around both outputs untouched; tree and workspaces handed in pre-filled with 0xFF and
reused after another cloud; two runs bit-equal.

Log-scales are held to float64 at 4x the largest difference between the reference's own golden log-scales and float64
(recomputed by tests/test_knn_host.py::golden_log_scale_error, not fixed here): one figure for the fixture, because it
estimates what forming mean and log in float32 costs the reference, and a five-point cloud alone estimates that poorly.
"""
import functools
import os
import time

import numpy as np
import pytest
import torch

import knn_reference as R
from test_knn_host import golden_log_scale_error

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = -7.0


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _dirty(nbytes):
    return torch.full((max(int(nbytes), 1),), 0xFF, dtype=torch.uint8, device=DEV)


@functools.lru_cache(maxsize=None)
def _spaces():
    """One tree buffer and one workspace for every small case, full of 0xFF at first and never cleaned in between:
    each build and query finds what the previous cloud left."""
    from gs_fused.knn import BYTES_BUILD, BYTES_QUERY, BYTES_TREE, _bytes

    n = 4097
    return (_dirty(_bytes(BYTES_TREE, n, 0)), _dirty(_bytes(BYTES_BUILD, n, 0)), _dirty(_bytes(BYTES_QUERY, 0, n, 16)))


def _build(P):
    from gs_fused import KNN

    tree, build_ws, _ = _spaces()
    return KNN(_t(P), _tree=tree, _workspace=build_ws)


def _query(knn, Q, k, exhaustive):
    """-> (d, idx) as NumPy, through outputs with a guard row either side and the shared dirty workspace."""
    m = knn.num_points if Q is None else len(Q)
    d = torch.full((m + 2, k), GUARD, dtype=torch.float32, device=DEV)
    i = torch.full((m + 2, k), int(GUARD), dtype=torch.int32, device=DEV)
    out = knn.query(None if Q is None else _t(Q), k, exhaustive=exhaustive, _workspace=_spaces()[2], _out=(d[1:-1], i[1:-1]))
    torch.cuda.synchronize()
    assert out[0].data_ptr() == d[1:-1].data_ptr()
    for buf in (d, i):
        assert bool((buf[0] == GUARD).all()) and bool((buf[-1] == GUARD).all()), "a guard row was written"
    return d[1:-1].cpu().numpy(), i[1:-1].cpu().numpy()


def _held(case):
    P, Q, k = R.case_inputs(case)
    (d64, _), (d32, i32) = R.truth(case)
    tol = R.tolerance(d64)
    knn = _build(P)
    assert knn.usable == len(P) and knn.skipped_points == 0
    got = {}
    for path in ("exhaustive", "tree", "tree again"):
        d, idx = got[path] = _query(knn, Q, k, path == "exhaustive")
        assert int(knn.invalid_queries) == 0
        assert d.dtype == np.float32 and idx.dtype == np.int32 and d.shape == d64.shape == idx.shape, (case, path)
        err = np.abs(d.astype(np.float64) - d64)
        print(f"{case} {path}: max |d - d64| / (2^-24 d64) = {(err[d64 > 0] / (R.U * d64[d64 > 0])).max(initial=0):.3f}")
        assert (err <= tol).all(), (case, path)
        assert (idx >= 0).all() and (idx < len(P)).all() and (np.diff(d, axis=1) >= 0).all(), (case, path)
        assert (np.abs(R.own_distance64(P, Q, idx) - d64) <= tol).all(), (case, path)
        if Q is None:
            assert not (idx == np.arange(len(P))[:, None]).any(), (case, path)
    de, ie = got["exhaustive"]
    assert np.array_equal(_bits(de), _bits(d32)) and np.array_equal(ie, i32), f"{case}: exhaustive != float32 restatement"
    for path in ("tree", "tree again"):
        assert np.array_equal(_bits(got[path][0]), _bits(de)) and np.array_equal(got[path][1], ie), f"{case}: {path} != exhaustive"
    return got["tree"]


# ---- 1 shapes, self mode -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", R.shape_cases())
def test_shapes(n, k):
    _held(("uniform", n, None, k))


# ---- 2 separate queries ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", R.KS)
@pytest.mark.parametrize("m", R.QUERY_M)
def test_separate_queries(m, k):
    d, idx = _held(("uniform", R.CLOUD_N, m, k))
    assert d[0, 0] == 0 and idx[0, 0] == R.CLOUD_N // 2  # the first query is that reference point: it is returned


# ---- 3 clouds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", R.KS)
@pytest.mark.parametrize("name", [c for c in R.CLOUDS if c != "uniform"])
def test_clouds(name, k):
    d, idx = _held((name, R.CLOUD_N, None, k))
    if name == "identical":
        assert (d == 0).all() and (idx == np.where(np.arange(k)[None, :] < np.arange(R.CLOUD_N)[:, None],
                                                   np.arange(k)[None, :], np.arange(k)[None, :] + 1)).all()
    if name == "lattice":
        assert (d == np.sqrt(np.round(d.astype(np.float64) ** 2)).astype(np.float32)).all()  # exact roots of integers: ties are exact ties
    if k == 3:
        _held((name, R.CLOUD_N, 65, 3))


# ---- 4 medium, on the device only --------------------------------------------------------------------------------------
def test_medium_tree_against_exhaustive():
    from gs_fused import KNN

    g = np.random.default_rng(5)
    u = g.standard_normal((100_000, 3))
    P = (u / np.linalg.norm(u, axis=1, keepdims=True) * (1 + 0.01 * g.standard_normal((len(u), 1)))).astype(np.float32)
    dp = _t(P)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    knn = KNN(dp)
    knn.query(None, 3)  # (warm-up of the shape)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    dt, it = knn.query(None, 3)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    de, ie = knn.query(None, 3, exhaustive=True)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    print(f"medium: build + first query {1e3 * (t1 - t0):.2f} ms, tree query {1e3 * (t2 - t1):.2f} ms, "
          f"exhaustive {1e3 * (t3 - t2):.2f} ms")
    assert torch.equal(dt.view(torch.int32), de.view(torch.int32)) and torch.equal(it, ie)
    rows = np.arange(0, len(P), 500)  # a sample against float64
    d64, _ = R.brute64(P, P[rows], 4)
    d64 = d64[:, 1:]  # (column 0 is the query itself at distance 0; no duplicates in this cloud)
    d, idx = dt.cpu().numpy()[rows], it.cpu().numpy()[rows]
    assert (np.abs(d - d64) <= R.tolerance(d64)).all() and (np.abs(R.own_distance64(P, P[rows], idx) - d64) <= R.tolerance(d64)).all()


# ---- 5 non-finite input, too few points, degenerate sizes, wrong arguments ------------------------------------------------
def test_non_finite_input_and_counts():
    P = R.cloud("uniform", 65).copy()
    P[[3, 40]] = [[np.nan, 0, 0], [0, np.inf, 0]]
    Q = R.queries("uniform", 65, 63).copy()
    Q[5, 2], Q[62, 0] = -np.inf, np.nan
    knn = _build(P)
    assert knn.usable == 63 and knn.skipped_points == 2
    for q, bad in ((Q, [5, 62]), (None, [3, 40])):
        d32, i32 = R.brute32(P, q, 3)
        for exhaustive in (True, False):
            d, idx = _query(knn, q, 3, exhaustive)
            assert int(knn.invalid_queries) == 2
            assert np.isnan(d[bad]).all() and (idx[bad] == -1).all() and np.isfinite(np.delete(d, bad, 0)).all()
            assert np.array_equal(_bits(d), _bits(d32)) and np.array_equal(idx, i32)
            assert not np.isin(idx, [3, 40]).any()


def test_too_few_points_and_degenerate_sizes():
    from gs_fused import KNN, knn as knn_call
    from rasterizer.cuda._backend import lib

    P = R.cloud("uniform", 65).copy()
    P[4:] = np.nan
    knn = _build(P)
    assert knn.usable == 4
    for exhaustive in (False, True):
        with pytest.raises(ValueError, match="4 usable reference points"):
            knn.query(None, 4, exhaustive=exhaustive)
        with pytest.raises(ValueError, match="4 usable reference points"):
            knn.query(_t(P[:2]), 5, exhaustive=exhaustive)
        assert knn.query(None, 3, exhaustive=exhaustive)[0].shape == (65, 3)
        assert knn.query(_t(P[:2]), 4, exhaustive=exhaustive)[0].shape == (2, 4)
    with pytest.raises(ValueError):
        KNN(_t(np.full((5, 3), np.nan, np.float32))).query(None, 1)
    with pytest.raises(ValueError):
        KNN(_t(np.zeros((0, 3), np.float32)))  # n = 0
    with pytest.raises(ValueError):
        knn_call(_t(P[:1]), 1)  # one point has no neighbour
    good = _build(R.cloud("uniform", 65))
    for exhaustive in (False, True):
        d, idx = good.query(_t(np.zeros((0, 3), np.float32)), 3, exhaustive=exhaustive)  # m = 0
        assert d.shape == (0, 3) and idx.shape == (0, 3) and d.dtype == torch.float32 and idx.dtype == torch.int32
    for k in (0, 17, -1):
        with pytest.raises(ValueError):
            good.query(None, k)
    torch.cuda.synchronize()
    q = lib().gsr_knn_workspace_bytes
    assert q(0, 0, 0, 1) == 0 and q(0, (1 << 28) + 1, 0, 1) == 0 and q(2, 0, 0, 3) == 0 and q(2, 0, 5, 0) == 0
    assert q(2, 0, 5, 17) == 0 and q(9, 5, 5, 3) == 0
    assert 0 < q(0, 1, 0, 0) < q(0, 1000, 0, 0) and 0 < q(1, 1, 0, 0) < q(1, 100000, 0, 0) and 0 < q(2, 0, 1, 3) < q(2, 0, 100000, 3)


def test_wrong_arguments_and_non_contiguous_input():
    from gs_fused import KNN

    P = R.cloud("uniform", 65)
    dp, good = _t(P), _build(P)
    for bad in (dp.double(), dp.cpu(), dp[:, :2].contiguous(), dp.reshape(-1), P):
        with pytest.raises(RuntimeError):
            KNN(bad)
        with pytest.raises(RuntimeError):
            good.query(bad, 3)
    wide = torch.zeros((65, 4), dtype=torch.float32, device=DEV)
    wide[:, :3] = dp
    cols = _t(np.ascontiguousarray(P.T)).t()
    assert not wide[:, :3].is_contiguous() and not cols.is_contiguous()
    want = good.query(None, 3)
    for view in (wide[:, :3], cols):
        d, idx = KNN(view).query(None, 3)
        assert torch.equal(d, want[0]) and torch.equal(idx, want[1])
        d, idx = good.query(view, 3)
        assert bool((d[:, 0] == 0).all()) and bool((idx[:, 0] == torch.arange(65, device=DEV)).all())


# ---- 6 golden, the reference's return types, the trainer's seeds ------------------------------------------------------------
def test_golden_clouds_and_log_scales():
    from gs_fused import initial_log_scales, knn_mean_distance

    g = np.load(os.path.join(ROOT, "tests", "golden", "knn.npz"))
    ref_err, per = golden_log_scale_error()
    print(f"reference's log-scales differ from float64 by {ref_err:.3e} at most: {per}")
    for name in g["cases"]:
        P, dref, lref = g[f"{name}_points"], g[f"{name}_dist"], g[f"{name}_log_scales"]
        d64 = R.brute64(P, None, 3)[0]
        d, idx = (x.cpu().numpy() for x in _build(P).query(None, 3))
        assert (np.abs(d - d64) <= R.tolerance(d64)).all() and (np.abs(d - dref) <= R.tolerance(d64) + 4 * R.U * d64).all()
        assert np.array_equal(d == 0, dref == 0)
        ls = initial_log_scales(_t(P), 3).cpu().numpy()
        assert ls.dtype == np.float32 and ls.shape == (len(P), 3) and (ls == ls[:, :1]).all()
        with np.errstate(divide="ignore"):
            l64 = np.log(d64.mean(1))
        fin = np.isfinite(l64)
        assert np.array_equal(np.isneginf(ls[:, 0]), ~fin) and np.array_equal(np.isneginf(lref[:, 0]), ~fin)
        err = np.abs(ls[fin, 0] - l64[fin]).max()
        print(f"{name}: log-scales against float64 {err:.3e} (bound {4 * ref_err:.3e}), against the reference "
              f"{np.abs(ls[fin] - lref[fin]).max():.3e}")
        assert err <= 4 * ref_err
        floored = initial_log_scales(_t(P), 3, floor=1e-7).cpu().numpy()
        assert np.isfinite(floored).all() and np.array_equal(floored[fin], ls[fin])
        # (the floored entries: one value, log(float32(1e-7)) to the log-scales' bound -- the device's logf and NumPy's
        # differ by a unit in the last place there, -16.118097 / -16.118095, so the bits are not compared)
        assert (floored[~fin] == floored[~fin][:1]).all()
        assert (np.abs(floored[~fin].astype(np.float64) - np.log(np.float64(np.float32(1e-7)))) <= 4 * ref_err).all()
        assert torch.equal(knn_mean_distance(_t(P), 3), _t(d).mean(dim=-1))


def test_k_nearest_has_the_reference_methods_return_types():
    from gs_fused import k_nearest

    P = R.cloud("uniform", 257)
    d32, i32 = R.truth(("uniform", 257, None, 3))[1]
    for x in (torch.from_numpy(P), _t(P), torch.nn.Parameter(_t(P)).data):
        d, idx = k_nearest(x, 3)
        assert isinstance(d, np.ndarray) and isinstance(idx, np.ndarray) and d.dtype == np.float32 and idx.dtype == np.float32
        assert d.shape == idx.shape == (257, 3)
        assert np.array_equal(_bits(d), _bits(d32)) and np.array_equal(idx, i32.astype(np.float32))


def _seeds(kind, **kw):
    from harness.train import blob_scene, seed_model

    return seed_model(blob_scene(6000, seed=3), 2000, kind, 11, **kw)


@pytest.mark.parametrize("kind", ["sfm", "random"])
def test_seed_model_gpu(kind):
    a, b = _seeds(kind, knn="gpu", device=DEV), _seeds(kind, knn="gpu")
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    l64 = np.log(np.maximum(R.brute64(a["means"], None, 3)[0].mean(1), 1e-7))
    ref_err, _ = golden_log_scale_error()
    assert a["scales"].dtype == np.float32 and a["scales"].shape == (2000, 3) and (a["scales"] == a["scales"][:, :1]).all()
    err = np.abs(a["scales"][:, 0] - l64).max()
    print(f"{kind}: log-scales against float64 {err:.3e} (bound {4 * ref_err:.3e})")
    assert err <= 4 * ref_err
    with pytest.raises(ValueError):
        _seeds(kind, knn="cpu")


@pytest.mark.parametrize("kind", ["sfm", "random"])
def test_seed_model_gpu_against_sklearn(kind):
    pytest.importorskip("sklearn")  # (the one comparison that needs scikit-learn where the test runs)
    a, c = _seeds(kind, knn="gpu", device=DEV), _seeds(kind)
    assert all(np.array_equal(a[k], c[k]) for k in a if k != "scales")
    l64 = np.log(np.maximum(R.brute64(a["means"], None, 3)[0].mean(1), 1e-7))
    ref_err, _ = golden_log_scale_error()
    print(f"{kind}: max |scale_gpu - scale_sklearn| = {np.abs(a['scales'] - c['scales']).max():.3e}, bound {4 * ref_err:.3e} each "
          f"against float64")
    for got in (a, c):
        assert np.abs(got["scales"][:, 0] - l64).max() <= 4 * ref_err
