"""GPU: mesh cleaning (gs_fusion.clean_mesh / mesh_components, csrc/mesh_clean.hip) against the NumPy oracle of
tests/mesh_clean_reference.py.  Every comparison is exact: labels, sizes and triangles with `array_equal`, vertex and
colour rows as int32 bit patterns.  The meshes are seeded; what they are assumed to hold is asserted on the oracle
alone in tests/test_mesh_clean_host.py.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_clean_reference as M
import tsdf_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)  # (a copy: the shared meshes are read-only)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _clean(v, t, c=None, min_faces=M.DEFAULT_MIN, **kw):
    from gs_fusion import clean_mesh

    out = clean_mesh(_t(v), _t(t), None if c is None else _t(c), min_faces, return_info=True, **kw)
    return [None if x is None else x.cpu().numpy() for x in out[:3]] + [out[3]]


def _components(t, V, v=None):
    from gs_fusion import mesh_components

    labels, sizes = mesh_components(_t(t), V, None if v is None else _t(v))
    assert labels.dtype == torch.int32 and sizes.dtype == torch.int32
    return labels.cpu().numpy(), sizes.cpu().numpy()


def _same_as_oracle(v, t, c, min_faces, ref=None, what=""):
    ref = ref or M.clean_reference(v, t, c, min_faces)
    gv, gc, gt, info = _clean(v, t, c, min_faces)
    assert gt.dtype == np.int32 and gt.shape == ref["triangles"].shape, what
    assert np.array_equal(gt, ref["triangles"]), what
    assert gv.shape == ref["vertices"].shape and np.array_equal(_bits(gv), _bits(ref["vertices"])), what
    if c is None:
        assert gc is None
    else:
        assert gc.shape == ref["colors"].shape and np.array_equal(_bits(gc), _bits(ref["colors"])), what
    assert info == ref["info"], what
    labels, sizes = _components(t, len(v), v)
    assert np.array_equal(labels, ref["labels"]) and np.array_equal(sizes, ref["sizes"]), what
    return ref, (gv, gc, gt)


# ---- strip -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("permute", [True, False])
def test_strip(permute):
    v, t = M.strip()
    if permute:
        v, t = M.permuted(v, t, 3)
    ref, (gv, _, gt) = _same_as_oracle(v, t, None, 4099)
    assert len(gt) == 4099 and len(gv) == 4101 and (ref["sizes"] == 4099).all() and (ref["labels"] == 0).all()
    ref, (gv, _, gt) = _same_as_oracle(v, t, None, 4100)
    assert gt.shape == (0, 3) and gv.shape == (0, 3) and ref["info"]["faces_removed_small"] == 4099


# ---- beads -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_faces", [0, 1, 6, 13])
def test_beads(min_faces):
    v, t = M.beads()
    ref, (_, _, gt) = _same_as_oracle(v, t, None, min_faces)
    assert ref["info"]["components"] == 3000
    assert len(gt) == (len(t) if min_faces <= 1 else 0 if min_faces == 13 else int((ref["sizes"] >= 6).sum()))
    assert min_faces != 6 or 0 < len(gt) < len(t)


# ---- touching --------------------------------------------------------------------------------------------------------
def test_touching():
    for make, want in ((M.two_fans_at_a_vertex, 2), (M.two_fans_at_an_edge, 1),
                       (lambda: M.two_fans_at_an_edge(True), 1), (M.three_faces_on_an_edge, 1)):
        v, t, labels = make()
        ref, _ = _same_as_oracle(v, t, None, 0)
        got, sizes = _components(t, len(v))
        assert np.array_equal(got, labels) and ref["info"]["components"] == want
        assert np.array_equal(sizes, np.bincount(labels, minlength=len(t))[labels])
    v, t, _ = M.two_fans_at_a_vertex()
    assert len(_clean(v, t, None, 3)[2]) == 6 and len(_clean(v, t, None, 4)[2]) == 0


# ---- order of the rules ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["collinear", "coincident", "repeated"])
def test_a_null_face_is_no_bridge_and_is_not_counted(kind):
    v, t, labels = M.null_bridge(kind)
    got, sizes = _components(t, len(v), v)
    assert np.array_equal(got, labels) and np.array_equal(sizes, [3, 3, 3, 0, 3, 3, 3])
    ref, (gv, _, gt) = _same_as_oracle(v, t, None, 3)
    assert len(gt) == 6 and ref["info"]["null_faces"] == 1 and ref["info"]["components"] == 2
    assert np.isfinite(gv).all() and len(gv) == 9  # the unreferenced rows of NaN are gone
    assert len(_clean(v, t, None, 4)[2]) == 0
    if kind != "repeated":
        # without coordinates it is an ordinary face, and with a NaN in one of its vertices it is not null
        got, sizes = _components(t, len(v))
        assert (got == 0).all() and (sizes == 7).all()
        v = v.copy()
        v[t[3, 0], 1] = np.nan
        ref, (gv, _, gt) = _same_as_oracle(v, t, None, 7)
        assert len(gt) == 7 and ref["info"]["null_faces"] == 0 and np.isnan(gv).sum() == 1


def test_six_orderings_count_once():
    v, t, first = M.six_orderings()
    ref, (gv, _, gt) = _same_as_oracle(v, t, None, 6)
    assert ref["info"]["duplicate_faces"] == 5
    labels, sizes = _components(t, len(v), v)
    assert [int(labels[a]) for a in M.SIX_AT] == [M.SIX_AT[0]] + [-1] * 5
    assert all(labels[a] == M.SIX_AT[0] and sizes[a] == 5 for a in M.FAN_REST_AT)
    assert not (gv[gt] == v[first]).all((1, 2)).any()  # removed: five faces, not ten
    _, (gv, _, gt) = _same_as_oracle(v, t, None, 5)
    assert (gv[gt] == v[first]).all((1, 2)).sum() == 1  # kept, as its lowest occurrence spells it


# ---- large -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("permute", [False, True], ids=["as generated", "permuted"])
def test_large_grid(permute):
    v, c, t = M.grid(permute)
    ref, (gv, gc, gt) = _same_as_oracle(v, t, c, M.DEFAULT_MIN, ref=M.grid_reference(permute))
    assert len(t) > 2048 * 256 and ref["info"]["components"] > 5000 and ref["info"]["components_kept"] == 1
    assert 0 < len(gt) < len(t) and 0 < len(gv) < len(v)


# ---- from the volume -------------------------------------------------------------------------------------------------
def test_sphere_from_the_volume_with_a_far_shell():
    from gs_fusion import TSDFVolume, clean_mesh

    class Views:
        def __init__(self, vol):
            self.vol = vol

        def integrate(self, d, c, fx, fy, cx, cy, V, valid=None, depth_trunc=10.0):
            self.vol.integrate(_t(d), _t(c), fx, fy, cx, cy, V, valid=None if valid is None else _t(valid),
                               depth_trunc=depth_trunc)

    vol = TSDFVolume(device=DEV, **R.sphere_volume_args())
    R.fuse_sphere(Views(vol))
    sv, sc, st = vol.extract_mesh()
    nv, nf = sv.shape[0], st.shape[0]
    closed, euler = M.closed_surface_report(st.cpu().numpy())
    assert nf > 30000 and closed and euler == 2
    # a small closed shell far away: a tetrahedron
    tv = torch.tensor([[9, 9, 9], [10, 9, 9], [9, 10, 9], [9, 9, 10]], dtype=torch.float32, device=DEV)
    tt = torch.tensor([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], dtype=torch.int32, device=DEV) + nv
    v = torch.cat([sv, tv]).contiguous()
    c = torch.cat([sc, torch.full((4, 3), 0.5, device=DEV)]).contiguous()
    t = torch.cat([tt[:2], st, tt[2:]]).contiguous()
    gv, gc, gt, info = clean_mesh(v, t, c, nf, return_info=True)
    assert torch.equal(gt, st) and torch.equal(gv.view(torch.int32), sv.view(torch.int32))
    assert torch.equal(gc.view(torch.int32), sc.view(torch.int32))
    assert info == {"null_faces": 0, "duplicate_faces": 0, "components": 2, "components_kept": 1,
                    "faces_removed_small": 4, "vertices_removed": 4}
    closed, euler = M.closed_surface_report(gt.cpu().numpy())
    assert closed and euler == 2
    assert clean_mesh(v, t, c, nf + 1)[2].shape == (0, 3)


# ---- plumbing --------------------------------------------------------------------------------------------------------
def test_colours_empty_meshes_repeatability_and_a_dirty_workspace():
    from gs_fusion import clean_mesh, mesh_components
    from gs_fusion.mesh import _clean_mesh
    from rasterizer.cuda._backend import lib

    v, c, t = M.grid(True, 40, 0.25, 3)
    for colours in (None, c, np.ascontiguousarray(c[:, :1]), np.concatenate([c, c[:, :2]], 1)):
        _same_as_oracle(v, t, colours, 40)
    # F = 0 (with and without vertices), V = 0
    for nv in (0, 5):
        gv, gc, gt, info = _clean(np.full((nv, 3), np.nan, np.float32), np.zeros((0, 3), np.int32),
                                  np.zeros((nv, 3), np.float32), 0)
        assert gv.shape == (0, 3) and gc.shape == (0, 3) and gt.shape == (0, 3) and gt.dtype == np.int32
        assert info == {"null_faces": 0, "duplicate_faces": 0, "components": 0, "components_kept": 0,
                        "faces_removed_small": 0, "vertices_removed": nv}
        labels, sizes = _components(np.zeros((0, 3), np.int32), nv)
        assert labels.shape == (0,) and sizes.shape == (0,)
    # two runs are bit-equal, and so is one on a workspace full of 0xFF bytes
    dv, dc, dt = _t(v), _t(c), _t(t)
    a = clean_mesh(dv, dt, dc, 40)
    b = clean_mesh(dv, dt, dc, 40)
    nbytes = lib().gsr_mesh_clean_workspace_bytes(len(v), len(t))
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    d = _clean_mesh(dv, dt, dc, 40, False, ws)
    for x, y, z in zip(a, b, d):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and torch.equal(x.view(torch.int32), z.view(torch.int32))
    la, lb = mesh_components(dt, len(v), dv), mesh_components(dt, len(v), dv)
    assert torch.equal(la[0], lb[0]) and torch.equal(la[1], lb[1])
    # the workspace query: nothing for no faces or sizes that do not fit, growing with the mesh
    q = lib().gsr_mesh_clean_workspace_bytes
    assert q(4, 0) == 0 and q(-1, 4) == 0 and q(4, (1 << 28) + 1) == 0
    sizes = [q(nv, nf) for nv, nf in ((3, 1), (100, 200), (100000, 200000), (1 << 20, 1 << 21))]
    assert sizes[0] > 0 and all(x < y for x, y in zip(sizes, sizes[1:])) and sizes[-1] >= 72 * (1 << 21)


def test_an_empty_cleaned_mesh_is_a_valid_file(tmp_path):
    """What the tool does after `mesh.ply` (tools/export_tsdf.py `write_cleaned`), with a threshold nothing reaches."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from export_tsdf import write_cleaned

    from gs_io import read_mesh_ply

    v, c, t = M.grid(True, 40, 0.25, 3)
    rows = write_cleaned(str(tmp_path), _t(v), _t(c), _t(t), len(t) + 1)
    assert rows == {"cleaned_vertices": 0, "cleaned_triangles": 0, "components": M.clean_reference(v, t)["info"]["components"]}
    path = os.path.join(str(tmp_path), "cleaned_mesh.ply")
    head = open(path, "rb").read(400)
    assert b"element vertex 0\n" in head and b"element face 0\n" in head and head.endswith(b"end_header\n")
    m = read_mesh_ply(path)
    assert m["vertices"].shape == (0, 3) and m["triangles"].shape == (0, 3) and m["vertex_colors"].shape == (0, 3)


def test_bad_arguments():
    from gs_fusion import clean_mesh, mesh_components
    from rasterizer.cuda._backend import lib

    v, c, t = M.grid(True, 40, 0.25, 3)
    dv, dc, dt = _t(v), _t(c), _t(t)
    for args in ((dv.double(), dt, dc), (dv, dt.long(), dc), (dv, dt, dc.half()), (dv.cpu(), dt, dc), (dv, dt.cpu(), dc),
                 (dv, dt, dc.cpu()), (dv[:, [2, 1, 0]].t().contiguous().t(), dt, dc), (dv, dt.t().contiguous().t(), dc),
                 (dv[:-1], dt, dc), (dv, dt, dc[:-1]), (dv, dt.reshape(-1), dc)):
        with pytest.raises(RuntimeError):
            clean_mesh(*args)
    with pytest.raises(RuntimeError):
        mesh_components(dt.long(), len(v))
    with pytest.raises(ValueError):
        clean_mesh(dv, dt, dc, -1)
    # an index outside [0, V): ValueError naming the lowest offending face, the library's message set, nothing written
    for bad in (-1, len(v)):
        t2 = t.copy()
        t2[[77, 1500], [1, 2]] = bad
        with pytest.raises(ValueError, match=r"triangle 77 has a vertex index outside \[0, %d\)" % len(v)):
            clean_mesh(dv, _t(t2), dc, 40)
        assert b"triangle 77" in lib().gsr_last_error()
        with pytest.raises(ValueError):
            mesh_components(_t(t2), len(v))
        # the C entry itself: labels and sizes handed in stay as they were
        import ctypes as C

        labels = torch.full((len(t),), -7, dtype=torch.int32, device=DEV)
        sizes = torch.full((len(t),), -7, dtype=torch.int32, device=DEV)
        state = torch.zeros(8, dtype=torch.int32, device=DEV)
        nbytes = lib().gsr_mesh_clean_workspace_bytes(len(v), len(t))
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
        d2 = _t(t2)
        torch.cuda.synchronize()
        rc = lib().gsr_mesh_label(C.c_int(len(v)), C.c_int(len(t)), C.c_void_p(dv.data_ptr()), C.c_void_p(d2.data_ptr()),
                                  C.c_int(0), C.c_void_p(state.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_size_t(nbytes),
                                  C.c_void_p(labels.data_ptr()), C.c_void_p(sizes.data_ptr()), None)
        torch.cuda.synchronize()
        assert rc == -4 and bool((labels == -7).all()) and bool((sizes == -7).all()) and bool((ws == 0).all())
    torch.cuda.synchronize()
    assert len(clean_mesh(dv, dt, dc, 40)[2]) > 0  # and the device is fine afterwards


# ---- command line ----------------------------------------------------------------------------------------------------
def test_command_line(tmp_path):
    from test_gpu_tsdf import _sphere_gaussians, _write_poses

    from gs_fusion import clean_mesh
    from gs_io import read_mesh_ply, write_gaussian_ply

    poses, model = str(tmp_path / "poses.json"), str(tmp_path / "model.ply")
    _write_poses(poses)
    write_gaussian_ply(model, _sphere_gaussians())
    args = R.sphere_volume_args()
    L, lo = args["voxel_length"], args["origin"]
    hi = [o + 8 * L * nb for o, nb in zip(lo, args["blocks"])]
    out = {}
    for name, extra in (("clean", ["--min-component-faces", "5000"]), ("raw", ["--no-clean"])):
        out[name] = str(tmp_path / name)
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tools", "export_tsdf.py"), "--ply",
               model, "--poses", poses, "--out", out[name], "--voxel-length", repr(L), "--sdf-trunc", repr(4 * L),
               "--bounds", *[repr(float(x)) for x in (*lo, *hi)], *extra]
        res = subprocess.run(cmd, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
        out[name + " summary"] = json.loads(res.stdout.strip().splitlines()[-1])
    assert not os.path.exists(os.path.join(out["raw"], "cleaned_mesh.ply"))
    assert "cleaned_triangles" not in out["raw summary"] and "components" not in out["raw summary"]
    assert sorted(os.listdir(out["raw"])) == ["mesh.ply", "point_cloud.ply"]
    mesh = read_mesh_ply(os.path.join(out["clean"], "mesh.ply"))
    cleaned = read_mesh_ply(os.path.join(out["clean"], "cleaned_mesh.ply"))
    raw = read_mesh_ply(os.path.join(out["raw"], "mesh.ply"))
    assert np.array_equal(raw["triangles"], mesh["triangles"]) and np.array_equal(raw["vertices"], mesh["vertices"])
    colours = mesh["vertex_colors"].astype(np.float32)  # (uint8 in the file: carried through as they are)
    gv, gc, gt, info = _clean(mesh["vertices"], mesh["triangles"], colours, 5000)
    s = out["clean summary"]
    assert s["cleaned_triangles"] == len(gt) > 5000 and s["cleaned_vertices"] == len(gv) and s["components"] == info["components"]
    assert s["triangles"] == len(mesh["triangles"]) and s["vertices"] == len(mesh["vertices"])
    assert np.array_equal(cleaned["triangles"], gt) and np.array_equal(_bits(cleaned["vertices"]), _bits(gv))
    assert np.array_equal(cleaned["vertex_colors"], gc.astype(np.uint8))
