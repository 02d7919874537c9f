"""CPU: the oriented crop box on the host -- `gs_fused.CropBox` against the two restatements of tests/crop_reference.py,
`from_params`, `crop_gaussians` on host tensors, the view descriptor left as it was, the declared symbols, the tools' argument
parsing and every ValueError."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import crop_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _box(name):
    from gs_fused import CropBox

    return CropBox(*CR.BOXES[name])


@pytest.mark.parametrize("name", list(CR.BOXES))
def test_cropbox_equals_the_float32_restatement_bit_for_bit(name):
    box, pts = _box(name), CR.rule_points()
    want = CR.crop_values(*CR.BOXES[name])
    assert box.values().dtype == np.float32 and box.values().tobytes() == want.tobytes()
    t = box.tensor("cpu")
    assert t.dtype == torch.float32 and t.shape == (16,) and t.numpy().tobytes() == want.tobytes() and t[15] == 0
    got = box.within(torch.from_numpy(pts.copy())).numpy()
    ref = CR.within_f32(want, pts)
    assert got.dtype == bool and np.array_equal(got, ref)
    assert not got[-3:].any()  # the NaN means
    kept = int(ref[:1000].sum())
    print(f"box {name}: keeps {kept} of 1000 uniform means")
    if name == "a":
        assert 400 < kept < 600
    elif name in ("b", "c"):
        assert 10 < kept < 900
    elif name == "d":
        assert ref[:-3].all()
    else:
        assert not ref.any()


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_points_on_a_face_are_outside_and_their_neighbours_decide(name):
    v = CR.crop_values(*CR.BOXES[name])
    on, inside, outside, faces = CR.face_points(name)
    h = v[12:15]
    print(f"box {name}: faces hit exactly: {sorted(set(faces))}")
    assert len(faces) == 64
    for i, (k, sign) in enumerate(faces):
        assert CR.q_f32(v, on[i:i + 1])[0, k] == np.float32(sign) * h[k]
        q_in, q_out = abs(CR.q_f32(v, inside[i:i + 1])[0, k]), abs(CR.q_f32(v, outside[i:i + 1])[0, k])
        assert h[k] - 4 * np.spacing(h[k]) <= q_in < h[k] < q_out <= h[k] + 4 * np.spacing(h[k])
    assert not CR.within_f32(v, on).any() and CR.within_f32(v, inside).all() and not CR.within_f32(v, outside).any()
    box = _box(name)
    assert not box.within(torch.from_numpy(on.copy())).any() and box.within(torch.from_numpy(inside.copy())).all()


@pytest.mark.parametrize("name", list(CR.BOXES))
def test_the_two_restatements_agree_away_from_the_faces(name):
    """What tests/test_gpu_crop.py relies on: on points 1e-3 away from every face (float64), the rule and
    `OrientedBox.within` as the reference writes it give the same mask."""
    R, T, S = CR.BOXES[name]
    pts = CR.margin_points(name, 4000, seed=11)
    q, h = CR.q_f64(R, T, S, pts)
    assert (np.abs(np.abs(q) - h) > 1e-3).all()
    from gs_fused import CropBox

    box = CropBox(R, T, S)
    a = box.within(torch.from_numpy(pts.copy())).numpy()  # the project's side, through the public class
    b = CR.within_reference(R, T, S, pts)
    c = (np.abs(q) < h).all(axis=1)
    assert np.array_equal(a, b) and np.array_equal(a, c)
    assert np.array_equal(a, CR.within_f32(box.values(), pts))
    # how far apart the two float32 evaluations are, against the margin
    gap = float(np.abs(CR.q_reference(R, T, pts) - CR.q_f32(box.values(), pts)).max())
    print(f"box {name}: the two float32 evaluations of q differ by at most {gap:.2e}")
    assert gap < 1e-4


def test_from_params_against_hand_computed_matrices():
    from gs_fused import CropBox

    h = math.pi / 2
    cases = [((h, 0, 0), [[1, 0, 0], [0, 0, -1], [0, 1, 0]]),   # roll: y -> z
             ((0, h, 0), [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]),   # pitch: z -> x
             ((0, 0, h), [[0, -1, 0], [1, 0, 0], [0, 0, 1]])]   # yaw: x -> y
    for rpy, want in cases:
        box = CropBox.from_params((1.0, 2.0, 3.0), rpy, (2.0, 4.0, 6.0))
        assert np.abs(box.R - np.array(want, np.float64)).max() < 1e-15, rpy
        assert np.array_equal(box.T, [1.0, 2.0, 3.0]) and np.array_equal(box.S, [2.0, 4.0, 6.0])
    r, p, y = 0.3, -0.7, 1.1
    Rx = np.array([[1, 0, 0], [0, math.cos(r), -math.sin(r)], [0, math.sin(r), math.cos(r)]])
    Ry = np.array([[math.cos(p), 0, math.sin(p)], [0, 1, 0], [-math.sin(p), 0, math.cos(p)]])
    Rz = np.array([[math.cos(y), -math.sin(y), 0], [math.sin(y), math.cos(y), 0], [0, 0, 1]])
    box = CropBox.from_params((0.3, -0.2, 0.4), (r, p, y), (1.5, 0.8, 2.5))
    assert np.abs(box.R - Rz @ Ry @ Rx).max() < 1e-15
    assert box.values().tobytes() == CR.crop_values(*CR.BOXES["b"]).tobytes()
    # a pure yaw by pi / 2 about T: the box's x axis is the world's y
    box = CropBox.from_params((0.0, 0.0, 0.0), (0, 0, h), (2.0, 0.2, 0.2))
    pts = torch.tensor([[0.0, 0.9, 0.0], [0.9, 0.0, 0.0]])
    assert box.within(pts).tolist() == [True, False]


def test_cropbox_refuses_what_is_not_a_box():
    from gs_fused import CropBox

    with pytest.raises(ValueError, match="R must have shape"):
        CropBox(np.eye(4), np.zeros(3), np.ones(3))
    with pytest.raises(ValueError, match="T must have shape"):
        CropBox(np.eye(3), np.zeros(4), np.ones(3))
    with pytest.raises(ValueError, match="S must be finite"):
        CropBox(np.eye(3), np.zeros(3), [1.0, np.nan, 1.0])
    with pytest.raises(ValueError, match="singular"):
        CropBox(np.diag([1.0, 0.0, 1.0]), np.zeros(3), np.ones(3))
    with pytest.raises(ValueError, match="three numbers"):
        CropBox.from_params((0, 0), (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match=r"means \[N,3\]"):
        CropBox(np.eye(3), np.zeros(3), np.ones(3)).within(torch.zeros(5))
    # torch tensors are taken as they are (float32 R as the viewer hands it over)
    box = CropBox(torch.eye(3), torch.zeros(3), torch.ones(3) * 2)
    assert box.within(torch.tensor([[0.5, 0.5, 0.5], [1.0, 0.0, 0.0]])).tolist() == [True, False]


def test_crop_gaussians_on_host_tensors():
    from gs_fused import crop_gaussians

    n = 300
    rng = np.random.default_rng(5)
    params = {"means": torch.from_numpy(CR.uniform_means(n, 5)), "scales": torch.from_numpy(rng.random((n, 3), np.float32)),
              "features_rest": torch.from_numpy(rng.random((n, 15, 3), np.float32)),
              "opacities": torch.from_numpy(rng.random((n, 1), np.float32))}
    box = _box("b")
    keep = CR.within_f32(CR.crop_values(*CR.BOXES["b"]), params["means"].numpy())
    out, mask = crop_gaussians(params, box, return_mask=True)
    assert np.array_equal(mask.numpy(), keep) and 0 < keep.sum() < n
    for k, v in params.items():
        assert torch.equal(out[k], v[torch.from_numpy(keep)]), k
    assert crop_gaussians(params, _box("e"))["features_rest"].shape == (0, 15, 3)
    with pytest.raises(ValueError, match="rows"):
        crop_gaussians(dict(params, quats=torch.zeros(n + 1, 4)), box)
    with pytest.raises(ValueError, match="means"):
        crop_gaussians({"scales": params["scales"]}, box)
    with pytest.raises(ValueError, match="CropBox"):
        crop_gaussians(params, box.tensor("cpu"))


def test_the_crop_rides_next_to_the_descriptor_not_in_it():
    """gsr_view_desc keeps its layout (tests/test_antialiased_host.py pins `opac_aa` as its last field): the box is
    an argument of gsr_view_forward_crop."""
    import re

    from gs_fused.render import _ViewDesc

    names = [f for f, _ in _ViewDesc._fields_]
    assert "crop" not in names and names[-1] == "opac_aa"
    src = open(os.path.join(ROOT, "include", "gsraster.h")).read()
    struct = src[src.index("typedef struct gsr_view_desc {"):src.index("} gsr_view_desc;")]
    assert "crop" not in re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    decl = re.search(r"int gsr_view_forward_crop\(([^;]*)\);", src).group(1)
    assert [a.strip() for a in decl.split(",")] == ["const gsr_view_desc *view", "const float *crop",
                                                    "gsr_stream_t stream"]


def test_the_entries_are_declared_and_exported():
    from rasterizer.cuda import _backend

    src = open(os.path.join(ROOT, "include", "gsraster.h")).read()
    for s in ("gsr_project_forward_crop", "gsr_crop_mask", "gsr_view_forward_crop"):
        assert s + "(" in src and s in _backend.SYMBOLS and hasattr(_backend.lib(), s)
    import gs_fused
    import rasterizer.cuda as RC

    assert callable(RC.project_gaussians_forward_crop) and callable(gs_fused.project_gaussians_cropped)
    assert callable(gs_fused.crop_gaussians)


def test_the_signatures_default_to_no_crop():
    import inspect

    from gs_fused import render_gaussians
    from gs_fused.render import ViewGraph
    from gs_fusion import fuse_views
    from harness.pipeline import render_view

    for fn, name in ((render_gaussians, "crop"), (ViewGraph.__init__, "crop"), (render_view, "crop"),
                     (fuse_views, "crop_box")):
        assert inspect.signature(fn).parameters[name].default is None, fn


def test_export_tsdf_parses_the_box():
    import export_tsdf as T

    base = ["--ply", "m.ply", "--poses", "p.json", "--out", "o"]
    assert T.parse_args(base).crop_box is None
    a = T.parse_args(base + ["--obb-pos", "0.3", "-0.2", "0.4", "--obb-rpy", "0.3", "-0.7", "1.1", "--obb-scale", "1.5",
                             "0.8", "2.5"])
    assert a.crop_box.values().tobytes() == CR.crop_values(*CR.BOXES["b"]).tobytes()
    for bad in (["--obb-pos", "0", "0", "0"], ["--obb-rpy", "0", "0", "0", "--obb-scale", "1", "1", "1"],
                ["--obb-pos", "0", "0", "0", "--obb-rpy", "0", "0", "0", "--obb-scale", "1", "-1", "1"],
                ["--obb-pos", "0", "0"]):
        with pytest.raises(SystemExit):
            T.parse_args(base + bad)


def test_export_gaussians_writes_the_kept_rows(tmp_path, capsys):
    """The tool end to end on the host (--device cpu): a checkpoint in the toolkit's layout -> a PLY of the rows
    `within` keeps, in order; without a box, all of them."""
    import export_gaussians as G
    from gs_io import read_gaussian_ply

    n = 200
    rng = np.random.default_rng(9)
    params = {"means": CR.uniform_means(n, 9), "scales": rng.standard_normal((n, 3)).astype(np.float32),
              "quats": rng.standard_normal((n, 4)).astype(np.float32),
              "features_dc": rng.standard_normal((n, 3)).astype(np.float32),
              "features_rest": rng.standard_normal((n, 15, 3)).astype(np.float32),
              "opacities": rng.standard_normal((n, 1)).astype(np.float32)}
    ckpt = tmp_path / "step-000000030.ckpt"
    torch.save({"step": 30, "pipeline": {"_model.gauss_params." + k: torch.from_numpy(v) for k, v in params.items()},
                "optimizers": {}, "schedulers": {}, "scalers": {}}, str(ckpt))
    obb = ["--obb-pos", "0.3", "-0.2", "0.4", "--obb-rpy", "0.3", "-0.7", "1.1", "--obb-scale", "1.5", "0.8", "2.5"]
    keep = CR.within_f32(CR.crop_values(*CR.BOXES["b"]), params["means"])
    assert 0 < keep.sum() < n
    for args, rows in ((obb, keep), ([], np.ones(n, bool))):
        out = tmp_path / f"g{len(args)}.ply"
        G.main([str(tmp_path), str(out), "--device", "cpu"] + args)  # (the directory: its latest step)
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert line["gaussians"] == n and line["written"] == int(rows.sum())
        back = read_gaussian_ply(str(out))
        for k, v in params.items():
            assert np.array_equal(np.asarray(back[k]).reshape(v[rows].shape), v[rows]), k
    with pytest.raises(SystemExit):
        G.parse_args([str(ckpt), "o.ply", "--obb-pos", "0", "0", "0"])
