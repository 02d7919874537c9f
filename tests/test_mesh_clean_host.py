"""CPU: the NumPy oracle of the mesh-cleaning rules (tests/mesh_clean_reference.py) against a plain Python union-find,
against scipy's connected components, and on hand-made meshes whose answers are written out here; the meshes the GPU
tests use are what those tests assume; the host side of `gsr_mesh_*` and of tools/export_tsdf.py.

Measured here: the oracle cleans the largest mesh of the GPU tests (561 026 triangles, 9 114 components, one of
543 721 faces) in 2.5 s unpermuted and 5 s permuted.
"""
import ctypes as C
import functools
import os
import sys
import threading

import numpy as np
import pytest

import mesh_clean_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000  # a non-null address that must never be dereferenced


def in_own_thread(fn):
    """The library keeps its last error message per thread: calls that are meant to fail run in a thread of their own,
    so that the main thread's message stays what the other test files expect to find."""
    @functools.wraps(fn)
    def wrapper(*args, **kw):
        box = []

        def body():
            try:
                fn(*args, **kw)
            except BaseException as e:  # noqa: BLE001 -- handed to the caller below
                box.append(e)

        t = threading.Thread(target=body)
        t.start()
        t.join()
        if box:
            raise box[0]

    return wrapper


def _small_meshes():
    out = {"strip": M.permuted(*M.strip(257), 1), "beads": M.beads(),
           "vertex": M.two_fans_at_a_vertex()[:2], "edge": M.two_fans_at_an_edge()[:2],
           "edge, same direction": M.two_fans_at_an_edge(True)[:2], "three": M.three_faces_on_an_edge()[:2],
           "six": M.six_orderings()[:2], "grid 40": M.grid(True, 40, 0.25, 3)[::2]}
    for kind in ("collinear", "coincident", "repeated"):
        out[kind] = M.null_bridge(kind)[:2]
    return out


@pytest.mark.parametrize("name", sorted(_small_meshes()))
def test_oracle_against_a_python_union_find(name):
    v, t = _small_meshes()[name]
    r = M.clean_reference(v, t, None, 0)
    alive = r["labels"] >= 0
    assert np.array_equal(M.union_find_labels(t, alive), r["labels"])
    # sizes are the label counts; a label is a face of its own component and its lowest
    assert (r["labels"][alive] <= np.nonzero(alive)[0]).all() and (r["labels"][r["labels"][alive]] == r["labels"][alive]).all()
    assert np.array_equal(r["sizes"][alive], np.bincount(r["labels"][alive], minlength=len(t))[r["labels"][alive]])
    assert (r["sizes"][~alive] == 0).all()


@pytest.mark.parametrize("name", ["beads", "six", "grid 40", "strip", "collinear"])
def test_oracle_against_scipy(name):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components

    v, t = _small_meshes()[name]
    r = M.clean_reference(v, t, None, 0)
    alive = np.nonzero(r["labels"] >= 0)[0]
    tt = np.asarray(t, np.int64)[alive]
    he = np.sort(np.concatenate([tt[:, [0, 1]], tt[:, [1, 2]], tt[:, [2, 0]]]), axis=1)
    key = he[:, 0] * len(v) + he[:, 1]
    face = np.tile(np.arange(len(alive)), 3)
    o = np.argsort(key, kind="stable")
    same = key[o][1:] == key[o][:-1]
    g = sp.coo_matrix((np.ones(int(same.sum())), (face[o][:-1][same], face[o][1:][same])), shape=(len(alive),) * 2)
    n, comp = connected_components(g, directed=False)
    assert n == r["info"]["components"]
    lowest = np.full(n, len(t))
    np.minimum.at(lowest, comp, alive)
    assert np.array_equal(lowest[comp], r["labels"][alive])


def test_hand_made_meshes():
    for make, want_components in ((M.two_fans_at_a_vertex, 2), (M.two_fans_at_an_edge, 1),
                                  (lambda: M.two_fans_at_an_edge(True), 1), (M.three_faces_on_an_edge, 1)):
        v, t, labels = make()
        r = M.clean_reference(v, t, None, 0)
        assert np.array_equal(r["labels"], labels) and r["info"]["components"] == want_components
        assert r["info"]["null_faces"] == 0 and r["info"]["duplicate_faces"] == 0
    # two fans of three at a vertex: min 3 keeps both, min 4 neither
    v, t, _ = M.two_fans_at_a_vertex()
    assert len(M.clean_reference(v, t, None, 3)["triangles"]) == 6
    r = M.clean_reference(v, t, None, 4)
    assert r["triangles"].shape == (0, 3) and r["vertices"].shape == (0, 3) and r["info"]["vertices_removed"] == 9


@pytest.mark.parametrize("kind", ["collinear", "coincident", "repeated"])
def test_a_null_face_is_no_bridge_and_is_not_counted(kind):
    v, t, labels = M.null_bridge(kind)
    r = M.clean_reference(v, t, None, 3)
    assert np.array_equal(r["labels"], labels) and np.array_equal(r["sizes"], [3, 3, 3, 0, 3, 3, 3])
    assert r["info"] == {"null_faces": 1, "duplicate_faces": 0, "components": 2, "components_kept": 2,
                         "faces_removed_small": 0, "vertices_removed": 14 - 9}
    assert len(M.clean_reference(v, t, None, 4)["triangles"]) == 0  # counted, the null face would make four
    if kind != "repeated":  # without coordinates the face is an ordinary one, and a bridge
        assert M.clean_reference(None, t, None, 0, num_vertices=14)["info"]["components"] == 1
    # a NaN in a referenced vertex: the product is not zero, the face stays and bridges
    v = v.copy()
    v[t[3, 0], 1] = np.nan
    r = M.clean_reference(v, t, None, 0)
    if kind != "repeated":
        assert r["info"]["null_faces"] == 0 and r["info"]["components"] == 1 and (r["sizes"] == 7).all()


def test_six_orderings_count_once():
    v, t, first = M.six_orderings()
    assert sorted(map(tuple, (t[a] for a in M.SIX_AT))) == sorted(
        (first[i], first[j], first[k]) for i, j, k in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)))
    r = M.clean_reference(v, t, None, 6)
    assert r["info"]["duplicate_faces"] == 5
    assert [int(r["labels"][a]) for a in M.SIX_AT] == [M.SIX_AT[0]] + [-1] * 5
    assert all(r["labels"][a] == M.SIX_AT[0] and r["sizes"][a] == 5 for a in M.FAN_REST_AT)
    # with min = 6 the fan is gone (counting duplicates it would have had ten faces); with min = 5 it stays, and what
    # is kept of the triple is its lowest occurrence, as spelled there
    gone = r["vertices"][r["triangles"]]
    kept = M.clean_reference(v, t, None, 5)
    stays = kept["vertices"][kept["triangles"]]
    assert not (gone == v[first]).all((1, 2)).any() and (stays == v[first]).all((1, 2)).sum() == 1


def test_the_meshes_are_what_the_gpu_tests_assume():
    v, t = M.strip()
    assert len(t) == 4099 and M.clean_reference(v, t, None, 4099)["info"]["components_kept"] == 1
    assert M.clean_reference(v, t, None, 4100)["triangles"].shape == (0, 3)
    v, t = M.beads()
    r = M.clean_reference(v, t, None, 0)
    sizes = r["sizes"][r["labels"] == np.arange(len(t))]
    assert len(sizes) == 3000 and set(sizes.tolist()) == set(range(1, 13)) and r["info"]["null_faces"] == 0
    assert not np.array_equal(np.sort(t[:, 0]), t[:, 0])  # permuted
    for permute in (False, True):
        v, c, t = M.grid(permute)
        r = M.grid_reference(permute)
        sizes = r["sizes"][r["labels"] == np.arange(len(t))]
        assert len(t) > 2048 * 256 and sizes.max() >= M.DEFAULT_MIN and r["info"]["components_kept"] == 1
        assert len(np.unique(sizes)) >= 30 and r["info"]["faces_removed_small"] > 10000
        assert r["info"]["vertices_removed"] > 1000
    a, b = M.grid_reference(False), M.grid_reference(True)
    assert a["info"] == b["info"]


def test_oracle_rejects_bad_indices():
    v, t = M.strip(5)
    for bad in (-1, len(v)):
        t2 = t.copy()
        t2[3, 1] = bad
        with pytest.raises(ValueError):
            M.clean_reference(v, t2, None, 0)


# ---- C ABI and Python wrappers, before any device use ------------------------------------------------------------------
@in_own_thread
def test_entries_reject_bad_arguments_on_the_host():
    from rasterizer.cuda._backend import lib

    L = lib()
    p, ws = C.c_void_p(FAKE), C.c_size_t(1 << 40)
    label = lambda V, F, m=0, state=p, w=p, nbytes=ws: L.gsr_mesh_label(  # noqa: E731
        C.c_int(V), C.c_int(F), p, p, C.c_int(m), state, w, nbytes, p, p, None)
    assert label(-1, 4) == -1 and b"num_vertices" in L.gsr_last_error()
    assert label(4, -1) == -1 and b"num_faces" in L.gsr_last_error()
    assert label(4, (1 << 28) + 1) == -1 and b"num_faces" in L.gsr_last_error()
    assert label(4, 4, m=-1) == -1 and b"min_component_faces" in L.gsr_last_error()
    assert label(4, 4, state=None) == -1 and b"null state" in L.gsr_last_error()
    emit = lambda V, F, nv, nf, c=3, out=p, w=p, nbytes=ws: L.gsr_mesh_emit(  # noqa: E731
        C.c_int(V), C.c_int(F), C.c_int(c), p, p, p, w, nbytes, C.c_int(nv), C.c_int(nf), out, p, p, None)
    assert emit(4, 4, 5, 1) == -1 and b"output counts" in L.gsr_last_error()
    assert emit(4, 4, 1, 5) == -1 and emit(4, 4, -1, 1) == -1 and emit(4, 4, 1, 1, c=-1) == -1
    assert emit(4, 4, 3, 1, out=None) == -1 and b"null pointer" in L.gsr_last_error()
    q = L.gsr_mesh_clean_workspace_bytes
    if q(C.c_int(4), C.c_int(4)):  # a missing or too small workspace: -3, like the other entries
        assert emit(4, 4, 3, 1, w=None) == -3 and emit(4, 4, 3, 1, nbytes=C.c_size_t(8)) == -3
        assert b"workspace" in L.gsr_last_error()
    else:  # no device: rocPRIM's size queries fail, the query says 0 and the entries say so instead of guessing
        assert emit(4, 4, 3, 1, w=None) == -1 and b"workspace size query failed" in L.gsr_last_error()
    assert emit(4, 4, 0, 0, out=None, w=None, nbytes=C.c_size_t(0)) == 0  # nothing to emit: a no-op
    assert q(C.c_int(4), C.c_int(0)) == 0 and q(C.c_int(-1), C.c_int(4)) == 0 and q(C.c_int(4), C.c_int((1 << 28) + 1)) == 0


def test_wrappers_reject_cpu_and_misshapen_tensors():
    import torch

    from gs_fusion import clean_mesh, mesh_components

    t = torch.zeros((4, 3), dtype=torch.int32)
    v = torch.zeros((5, 3))
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        clean_mesh(v, t)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        mesh_components(t, 5)
    with pytest.raises(RuntimeError, match="must be a tensor"):
        clean_mesh(np.zeros((5, 3), np.float32), t)
    with pytest.raises(RuntimeError, match=r"vertices must be \[V,3\]"):
        clean_mesh(torch.zeros(()), t)


def test_command_line_options():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from export_tsdf import parse_args

    base = ["--ply", "m.ply", "--poses", "p.json", "--out", "o"]
    a = parse_args(base)
    assert a.clean is True and a.min_component_faces == 20000 and a.voxel_length == 0.01171875
    assert parse_args(base + ["--no-clean"]).clean is False
    assert parse_args(base + ["--no-clean", "--clean"]).clean is True
    assert parse_args(base + ["--min-component-faces", "50"]).min_component_faces == 50
    for bad in (["--min-component-faces", "-1"], ["--min-component-faces", "x"], ["--clean", "yes"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
