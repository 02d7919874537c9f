"""CPU: the surface-distance rule (tests/surface_distance_reference.py) against an independent formulation and against
what the toolkit's own tool printed for the fixtures of tests/golden/surface_distance/; `read_stl`; the command line;
the logic of the tree build and the stackless walk of csrc/mesh_distance.hip, restated in Python; and `r`.

r: the worst |d32 - d64| / (2^-24 S) of the float32 restatement over every input of the GPU tests (S: the largest
|coordinate| of mesh and points).  MEASURED 3.356 (on "shape 1": one triangle, 4 097 points; 3.18 on "identical", 2.34
on "shape 2", 2.15 on "line", at most 1.6 elsewhere, 0.0004 on the case moved by (1000, -1000, 500), where the
translation a - p is exact and S is large); pinned as R_PINNED = 3.36 in the reference module.  The GPU tests allow
tol = 4 * 3.36 * 2^-24 S.
"""
import json
import os
import sys

import numpy as np
import pytest

import surface_distance_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "surface_distance")
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _expected():
    return json.load(open(os.path.join(GOLDEN, "expected.json")))


def test_the_rule_agrees_with_projection_or_nearest_edge():
    for name in R.CASES:
        if name in ("shape 4096", "one large"):
            continue  # (the same generator at sizes the dense formulation takes long for)
        v, t, p = R.case(name)
        d64 = R.truth(name)[0]
        ok = np.isfinite(d64)
        other = R.distance_by_projection(p[ok], v, t[R.usable(v, t)])
        assert np.abs(other - d64[ok]).max() <= 1e-12 * max(1.0, R.scale_of(p, v, t)), name
    for (p, want), got in zip(R.SEVEN_POINTS, R.truth("seven regions")[0]):
        assert abs(got - want) <= 1e-15, p
    d = R.truth("two triangles")[0]
    v, t, p = R.case("two triangles")
    assert np.allclose(R.face_distance(p, v, t, np.zeros(len(p), int)), R.face_distance(p, v, t, np.ones(len(p), int)),
                       rtol=0, atol=1e-15) and (d > 0).all()


def test_degenerate_and_poisoned_inputs_of_the_rule():
    v, t, p = R.case("degenerate")
    for dtype in (np.float64, np.float32):
        d, f = R.distance(p, v, t, dtype)
        assert np.isfinite(d).all()
    # the hand-made points against the hand-made degenerate triangles alone (faces 60 .. 63)
    want = {100: 0.5, 101: 2.0, 102: 1.0, 103: 0.5, 104: 0.25, 105: 2.0}
    d = R.distance(p, v, t[60:], np.float64)[0]
    for i, x in want.items():
        assert d[i] == x, (i, d[i])
    v, t, p = R.case("poisoned")
    assert tuple(np.nonzero(~R.usable(v, t))[0]) == R.POISONED_TRIANGLES
    d, f = R.truth("poisoned")
    assert tuple(np.nonzero(np.isnan(d))[0]) == R.POISONED_POINTS and (f[list(R.POISONED_POINTS)] == -1).all()
    assert not np.isin(f, R.POISONED_TRIANGLES).any()
    with pytest.raises(ValueError):
        R.distance(p, np.full((3, 3), np.nan, np.float32), np.array([[0, 1, 2]]))


def test_float64_matches_what_the_toolkit_tool_printed():
    from gs_io import read_mesh_ply, read_stl

    for name, e in _expected().items():
        tri = read_stl(os.path.join(GOLDEN, e["ground_truth"]))
        p = read_mesh_ply(os.path.join(GOLDEN, e["points"]))["vertices"]
        assert tri.shape == (e["triangles"], 3, 3) and p.shape == (e["num_points"], 3)
        d = R.distance(p, tri.reshape(-1, 3), np.arange(3 * len(tri)).reshape(-1, 3))[0]
        assert "%.6g" % d.mean() == e["average_error"], name  # (what `std::cout << double` prints)
        unit = 10.0 ** (np.floor(np.log10(d.mean())) - 5)
        assert abs(d.mean() - float(e["average_error"])) <= 0.45 * unit, name


def test_read_stl(tmp_path):
    from gs_io import read_stl

    e = _expected()["soup"]
    binary = read_stl(os.path.join(GOLDEN, e["ground_truth"]))
    text = read_stl(os.path.join(GOLDEN, e["ground_truth_ascii"]))
    assert binary.dtype == np.float32 and binary.shape == (200, 3, 3)
    assert text.dtype == np.float32 and np.array_equal(binary.view(np.int32), text.view(np.int32))
    assert open(os.path.join(GOLDEN, e["ground_truth"]), "rb").read(5) == b"solid"  # told by size, not by this word
    for src, cut in ((e["ground_truth"], 10084 - 7), (e["ground_truth"], 60), (e["ground_truth_ascii"], 30000)):
        path = str(tmp_path / "cut.stl")
        open(path, "wb").write(open(os.path.join(GOLDEN, src), "rb").read()[:cut])
        with pytest.raises(ValueError):
            read_stl(path)
    tri = np.arange(18, dtype=np.float32).reshape(2, 3, 3) / 8
    R.write_binary_stl(str(tmp_path / "b.stl"), tri)
    R.write_ascii_stl(str(tmp_path / "a.stl"), tri)
    assert np.array_equal(read_stl(str(tmp_path / "b.stl")), tri) and np.array_equal(read_stl(str(tmp_path / "a.stl")), tri)
    R.write_binary_stl(str(tmp_path / "e.stl"), tri[:0])
    assert read_stl(str(tmp_path / "e.stl")).shape == (0, 3, 3)


def test_command_line_arguments(capsys):
    import eval_surface
    import export_tsdf

    a = eval_surface.parse_args(["--gt", "a.stl", "--mesh", "m.ply"])
    assert (a.gt, a.mesh, a.both, a.threshold, a.device) == ("a.stl", "m.ply", False, None, "cuda:0")
    a = eval_surface.parse_args(["--gt", "a.PLY", "--mesh", "m.ply", "--both", "--threshold", "0.01"])
    assert a.both and a.threshold == 0.01
    for bad in (["--mesh", "m.ply"], ["--gt", "a.stl"], ["--gt", "a.obj", "--mesh", "m.ply"],
                ["--gt", "a.stl", "--mesh", "m.ply", "--threshold", "-1"]):
        with pytest.raises(SystemExit):
            eval_surface.parse_args(bad)
    capsys.readouterr()
    base = ["--ply", "m.ply", "--poses", "p.json", "--out", "o"]
    a = export_tsdf.parse_args(base)
    assert a.gt is None and a.gt_threshold is None
    a = export_tsdf.parse_args(base + ["--gt", "g.stl", "--gt-threshold", "0.5"])
    assert a.gt == "g.stl" and a.gt_threshold == 0.5
    with pytest.raises(SystemExit):
        export_tsdf.parse_args(base + ["--gt-threshold", "-2"])
    capsys.readouterr()
    v, t = eval_surface.load_mesh(os.path.join(GOLDEN, "sphere.stl"))
    assert v.shape == (192, 3) and v.dtype == np.float32 and np.array_equal(t, np.arange(192).reshape(64, 3))
    v, t = eval_surface.load_mesh(os.path.join(GOLDEN, "sphere_points.ply"))
    assert v.shape == (500, 3) and t.shape == (0, 3) and t.dtype == np.int32


def test_r_of_the_float32_restatement():
    worst = 0.0
    for name in R.CASES:
        v, t, p = R.case(name)
        d64, d32 = R.truth(name)[0], R.restated(name)[0]
        ok = np.isfinite(d64)
        assert np.array_equal(ok, np.isfinite(d32)), name
        r = float(np.abs(d32[ok].astype(np.float64) - d64[ok]).max() / (R.U * R.scale_of(p, v, t)))
        print(f"r[{name}] = {r:.4f}")
        worst = max(worst, r)
    print(f"r = {worst:.4f}, pinned {R.R_PINNED}")
    assert worst <= R.R_PINNED          # the pin holds ...
    assert worst >= 0.9 * R.R_PINNED    # ... and is the measurement, not a loose guess


def test_the_tree_and_the_walk_restated():
    """Karras' nodes over the unique keys, the ropes, the refit's arrival counters and the pruned walk, in Python: an
    unpruned walk meets every leaf once and in order, the refit reaches the root, and the pruned walk returns the
    float32 restatement's minimum bit for bit."""
    for name, rows in (("shape 1", 40), ("shape 2", 40), ("shape 63", 60), ("shape 65", 60), ("shape 257", 60),
                       ("identical", 30), ("line", 60), ("plane", 60), ("degenerate", 107), ("poisoned", 300),
                       ("far", 60), ("two triangles", 9), ("seven regions", 14)):
        v, t, p = R.case(name)
        tree = R.Tree(v, t)
        assert tree.n == int(R.usable(v, t).sum())
        assert tree.leaves_reached() == list(range(tree.n)) and tree.refit_complete, name
        assert len(set(tree.key)) == tree.n
        for i in range(tree.n - 1):  # every box holds the boxes of its children
            for c in (tree.left[i], tree.right[i]):
                lo, hi = (tree.tri[~c].min(0), tree.tri[~c].max(0)) if c < 0 else (tree.box_lo[c], tree.box_hi[c])
                assert (tree.box_lo[i] <= lo).all() and (tree.box_hi[i] >= hi).all(), (name, i)
        d, f, tests = tree.query(p[:rows])
        want = R.restated(name)[0][:rows]
        assert np.array_equal(d.view(np.int32), want.view(np.int32)), name
        if name == "shape 257":
            assert np.mean(tests) < 0.2 * tree.n  # (the walk prunes)
    # without the index in the low bits equal codes are equal keys, and the nodes above them are no tree
    v, t, p = R.case("identical")
    broken = R.Tree(v, t, tie_break=False)
    assert broken.leaves_reached() != list(range(broken.n)) or not broken.refit_complete
    # with the slack's sign turned the walk loses minima
    v, t, p = R.case("shape 257")
    d, _, _ = R.Tree(v, t).query(p[:200], slack=-0.25)
    assert (d.view(np.int32) != R.restated("shape 257")[0][:200].view(np.int32)).any()
