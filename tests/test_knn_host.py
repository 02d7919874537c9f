"""Host: the restatements of the k-nearest-neighbour rule (tests/knn_reference.py) against the reference's recorded
output (tests/golden/knn.npz, written by make_golden_knn.py from `k_nearest_sklearn` itself) and against one another.
No GPU: what the device tests (tests/test_gpu_knn.py) are judged by is checked here first.
"""
import os

import numpy as np
import pytest

import knn_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn.npz")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def golden_log_scale_error():
    """max |reference's log-scale - float64 log-scale| over the golden clouds (finite ones), and per cloud: what the
    reference's own float32 forming of mean and log costs.  The GPU test holds the device to 4x the maximum."""
    g = np.load(GOLDEN)
    per = {}
    for name in g["cases"]:
        d64 = R.brute64(g[f"{name}_points"], None, 3)[0]
        with np.errstate(divide="ignore"):
            l64 = np.log(d64.mean(1))
        fin = np.isfinite(l64)
        ls = g[f"{name}_log_scales"]
        assert np.array_equal(np.isneginf(ls[:, 0]), ~fin) and (ls == ls[:, :1]).all()
        per[str(name)] = float(np.abs(ls[fin, 0] - l64[fin]).max())
    return max(per.values()), per


def test_float64_rule_reproduces_the_golden_distances():
    g = np.load(GOLDEN)
    assert len(g["cases"]) >= 4 and os.path.getsize(GOLDEN) < 100_000
    for name in g["cases"]:
        p, d = g[f"{name}_points"], g[f"{name}_dist"]
        assert p.dtype == np.float32 and d.dtype == np.float32 and len(p) <= 2000 and d.shape == (len(p), 3)
        d64, idx = R.brute64(p, None, 3)
        err = np.abs(d.astype(np.float64) - d64)
        print(f"{name}: n={len(p)} max |golden - d64| / (2^-24 d64) = {(err[d64 > 0] / (R.U * d64[d64 > 0])).max():.3f}, "
              f"bit-equal to float32(d64): {np.array_equal(_bits(d), _bits(d64))}")
        assert (err <= 4 * R.U * d64).all() and (d[d64 == 0] == 0).all()
        assert not (idx == np.arange(len(p))[:, None]).any()  # self left out by index, twins kept
    assert (g["duplicates_400_dist"] == 0).any()
    worst, per = golden_log_scale_error()
    print("reference's log-scales against float64:", {k: f"{v:.3e}" for k, v in per.items()}, f"max {worst:.3e}")
    assert 0 < worst < 1e-5


def test_walk_returns_the_float32_brute_force_bit_for_bit():
    trees = {}
    for case in R.small_cases():
        P, Q, k = R.case_inputs(case)
        tree = trees.setdefault(case[:2], R.Tree(P))
        d, idx, _ = R.walk(tree, P if Q is None else Q, k, Q is None)
        (d64, _), (d32, i32) = R.truth(case)
        assert np.array_equal(_bits(d), _bits(d32)) and np.array_equal(idx, i32), case
        assert (np.diff(d, axis=1) >= 0).all() and (idx >= 0).all() and (idx < len(P)).all(), case
        if Q is None:
            assert not (idx == np.arange(len(P))[:, None]).any(), case
        assert (np.abs(d - d64) <= R.tolerance(d64)).all(), case
        own = R.own_distance64(P, Q, idx)
        assert (np.abs(own - d64) <= R.tolerance(d64)).all(), case


def test_measured_rounding_of_the_float32_rule():
    """r = max |d32 - d64| / (2^-24 d64) over every small input of the GPU tests (d64 = 0 left out: d32 is exactly 0
    there).  Expected from the operations: three differences (u each), three squares, two sums, a root: < 3.5."""
    worst, at = 0.0, None
    for case in R.small_cases():
        (d64, _), (d32, _) = R.truth(case)
        nz = d64 > 0
        assert (d32[~nz] == 0).all()
        r = (np.abs(d32.astype(np.float64) - d64)[nz] / (R.U * d64[nz])).max(initial=0.0)
        if r > worst:
            worst, at = r, case
    print(f"r = {worst:.4f} at {at}; pinned {R.R_PINNED}")
    assert R.R_PINNED - 0.05 <= worst <= R.R_PINNED < 3.5


def test_walk_prunes():
    P = R.cloud("uniform", 4097)
    tree = R.Tree(P)
    assert tree.L == 513 and tree.Lp == 1024 and tree.nu == 4097
    for k in R.KS:
        tests = R.walk(tree, P, k, True)[2]
        print(f"uniform 4097, k={k}: leaf tests per query mean {tests.mean():.1f}, max {tests.max()} of {tree.L} leaves")
        assert tests.mean() * R.LEAF < 4097 / 10 and tests.max() < tree.L / 4
    P = R.cloud("identical", R.CLOUD_N)
    tree = R.Tree(P)
    tests = R.walk(tree, P, 3, True)[2]
    assert (tests == tree.L).all()  # every bound is 0 = the k-th d2: nothing may be skipped


def test_inverted_comparison_loses_neighbours():
    case = ("uniform", R.CLOUD_N, None, 3)
    P, _, k = R.case_inputs(case)
    d, idx, _ = R.walk(R.Tree(P), P, k, True, invert=True)
    (_, _), (d32, i32) = R.truth(case)
    wrong = int((idx != i32).any(1).sum())
    print(f"prune comparison inverted: {wrong} of {len(P)} rows lose a neighbour")
    assert wrong > len(P) // 10 and (d >= d32).all()


def test_non_finite_and_too_few():
    P = R.cloud("uniform", 65).copy()
    P[[3, 40]] = [[np.nan, 0, 0], [0, np.inf, 0]]
    Q = R.queries("uniform", 65, 63).copy()
    Q[5, 2] = -np.inf
    tree = R.Tree(P)
    assert tree.skipped == 2 and tree.nu == 63
    for q, self_mode in ((Q, False), (P, True)):
        d, idx, _ = R.walk(tree, q, 3, self_mode)
        d32, i32 = R.brute32(P, None if self_mode else q, 3)
        assert np.array_equal(_bits(d), _bits(d32)) and np.array_equal(idx, i32)
        bad = ~np.isfinite(q).all(1)
        assert np.isnan(d[bad]).all() and (idx[bad] == -1).all() and not np.isin(idx, [3, 40]).any()
    with pytest.raises(ValueError):
        R.brute32(P[:3], None, 3)
