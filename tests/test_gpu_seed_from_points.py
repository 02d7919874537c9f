"""GPU: tools/seed_from_points.py -- a point-cloud PLY in, the model's start out (populate_modules, vanilla_gs.py:126-174),
round-tripped through gs_io.read_gaussian_ply; the log-scales held to float64 like those of tests/test_gpu_knn.py."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import knn_reference as R
from test_knn_host import golden_log_scale_error

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "seed_from_points.py")
SH_C0 = 0.28209479177387814


def _run(*args):
    res = subprocess.run(["timeout", "-k", "10", "300", sys.executable, TOOL, *args], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def test_round_trip(tmp_path):
    from gs_io import read_gaussian_ply, write_point_cloud_ply

    g = np.random.default_rng(8)
    pts = g.uniform(-1, 1, (1500, 3)).astype(np.float32)
    pts[700] = pts[20]  # a twin: -inf log-scales for neither (the other two neighbours keep the mean positive)
    rgb = g.integers(0, 256, (1500, 3)).astype(np.uint8)
    write_point_cloud_ply(str(tmp_path / "cloud.ply"), pts, rgb)
    row = _run("--points", str(tmp_path / "cloud.ply"), "--out", str(tmp_path / "seed.ply"), "--sh-degree", "2", "--seed", "4")
    assert row["gaussians"] == 1500 and row["dropped_points"] == 0 and row["coloured"] and row["duplicate_points"] == 0
    m = read_gaussian_ply(str(tmp_path / "seed.ply"))
    assert np.array_equal(m["means"], pts) and m["features_rest"].shape == (1500, 8, 3) and not m["features_rest"].any()
    l64 = np.log(R.brute64(pts, None, 3)[0].mean(1))
    ref_err, _ = golden_log_scale_error()
    assert m["scales"].shape == (1500, 3) and (m["scales"] == m["scales"][:, :1]).all()
    assert np.abs(m["scales"][:, 0] - l64).max() <= 4 * ref_err
    assert np.allclose(np.linalg.norm(m["quats"], axis=1), 1, atol=1e-6) and len(np.unique(m["quats"], axis=0)) == 1500
    assert (m["opacities"] == np.float32(math.log(0.1 / 0.9))).all() and m["opacities"].shape == (1500, 1)
    want_dc = (rgb.astype(np.float32) / np.float32(255) - np.float32(0.5)) / np.float32(SH_C0)
    assert np.array_equal(m["features_dc"], want_dc)
    again = _run("--points", str(tmp_path / "cloud.ply"), "--out", str(tmp_path / "seed2.ply"), "--sh-degree", "2", "--seed", "4")
    assert again["median_scale"] == row["median_scale"]
    assert open(tmp_path / "seed.ply", "rb").read() == open(tmp_path / "seed2.ply", "rb").read()
