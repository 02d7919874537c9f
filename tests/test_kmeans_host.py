"""Without a GPU: the k-means restatements' own properties, the codec of gs_io.compressed against its NumPy
restatement bit for bit and against its decode bound, the container file, the prototypes of the three native entries,
the tool's arguments, and every ValueError that needs no device."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import kmeans_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
TILE = 128


def _tool():
    spec = importlib.util.spec_from_file_location("compress_gaussians_tool",
                                                  os.path.join(ROOT, "tools", "compress_gaussians.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def as_torch(p):
    return {k: torch.from_numpy(v) for k, v in p.items()}


# ---- the restatement --------------------------------------------------------------------------------------------------
def test_tile_constant_matches_the_header():
    from gs_fused.kmeans import INERTIA_SHARE, MAX_CLUSTERS, MAX_DIM, TILE as T

    text = open(os.path.join(ROOT, "include", "gsraster.h")).read()
    for name, value in (("GSR_KMEANS_TILE", T), ("GSR_KMEANS_MAX_DIM", MAX_DIM),
                        ("GSR_KMEANS_MAX_CLUSTERS", MAX_CLUSTERS), ("GSR_KMEANS_INERTIA_SHARE", INERTIA_SHARE)):
        assert f"#define {name} {value}" in text, name
    assert T == TILE and T % 4 == 0


@pytest.mark.parametrize("n,k,d", [(65, 7, 3), (257, TILE + 1, 9), (300, 2 * TILE + 3, 45), (1, 1, 1), (64, 2, 48)])
def test_assign_restatement_is_the_sequential_rule_and_its_edges_occur(n, k, d):
    x, c = R.assign_case(n, k, d, seed=n + k + d, tile=TILE)
    labels, dist = R.assign(x, c)
    seq_labels, seq_dist = R.assign_sequential(x, c)
    assert labels.dtype == np.int32 and dist.dtype == F32
    assert np.array_equal(labels, seq_labels) and np.array_equal(dist.view(np.int32), seq_dist.view(np.int32))
    assert labels[0] == 0 and dist[0] == 0  # a point on centroid 0 (and on its duplicate 1, when there is one)
    if n > 4:
        tied = R.tied_rows(x, c)
        d_all = R.distances(x, c)
        assert tied[0] or k == 1
        assert np.isnan(x[1]).all() and labels[1] == 0 and np.isinf(dist[1])    # a row of NaN
        assert np.isinf(x[2]).all() and labels[2] == 0 and np.isinf(dist[2])    # a row of +inf
        assert dist[4] == 0 and (labels[4] == k - 1 or tied[4])                 # a point on the last centroid
        if k > 3:
            assert np.isnan(c[2]).all() and not (labels == 2).any()            # a NaN centroid never wins
        if k > TILE:
            assert labels[3] == TILE - 1 and dist[3] == 0 and d_all[3, TILE] == 0  # a tie across the tile boundary
        if k >= 7 and n >= 257:  # ties among distinct centroids too (the coarse grid), all to the lowest index
            distinct = tied & (dist > 0)
            assert distinct.any()
        finite = np.where(np.isnan(d_all), np.inf, d_all)
        for i in np.flatnonzero(tied):
            assert labels[i] == np.flatnonzero(finite[i] == finite[i].min())[0]


def test_update_and_inertia_restatements():
    x, labels, old, w = R.update_case(5, seed=1, weighted=True)
    assert sorted(np.bincount(labels, minlength=len(R.UPDATE_SIZES)).tolist()) == sorted(R.UPDATE_SIZES)
    u = R.update(x, labels, old, w)
    assert u["counts"].tolist() == list(R.UPDATE_SIZES)
    assert u["kept"].tolist() == [s == 0 or s == 7 for s in R.UPDATE_SIZES]
    assert np.array_equal(u["new"][u["kept"]].view(np.int32), old[u["kept"]].view(np.int32))
    c = 5
    idx = np.flatnonzero(labels == c)
    want = (w[idx, None].astype(F64) * x[idx].astype(F64)).sum(0) / w[idx].astype(F64).sum()
    assert np.allclose(u["mean"][c], want, rtol=1e-13, atol=0)
    plain = R.update(x, labels, old)
    assert np.allclose(plain["mean"][1], x[labels == 1][0].astype(F64), rtol=0, atol=0)  # one member: itself
    assert np.array_equal(plain["new"][1].view(np.int32), x[labels == 1][0].view(np.int32))
    # the inertia of points on their centroids is 0; moving one centroid by e adds |e|^2 per member
    cents = plain["new"]
    base = R.inertia(x, cents, labels)
    moved = cents.copy()
    moved[4, 0] += F32(0.5)
    delta = R.inertia(x, moved, labels) - base
    members = x[labels == 4, 0].astype(F64)
    want = ((members - F64(moved[4, 0])) ** 2 - (members - F64(cents[4, 0])) ** 2).sum()
    assert abs(delta - want) <= 1e-9 * abs(base)
    assert R.inertia(x, cents, labels, np.zeros(len(labels), F32)) == 0.0


# ---- the codec --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 1, 3])
def test_cpu_codec_equals_the_numpy_restatement_bit_for_bit_and_meets_the_decode_bound(degree):
    from gs_io.compressed import BITS, compress_gaussians, decompress_gaussians

    p = R.gaussian_params(257, degree, seed=degree)
    blob = compress_gaussians(as_torch(p), sh_clusters=0)
    back = decompress_gaussians(blob)
    n = 257
    columns = {"means": p["means"], "scales": p["scales"], "opacities": p["opacities"],
               "features_dc": p["features_dc"], "quats": R.normalised_quats(p["quats"])}
    if degree:
        columns["features_rest"] = p["features_rest"].reshape(n, -1)
    assert ("features_rest" in blob) == bool(degree) and "sh_labels" not in blob and "sh_codebook" not in blob
    for name, x in columns.items():
        x = np.asarray(x).astype(F64)
        lo, hi = (([-1.0] * 4, [1.0] * 4) if name == "quats" else (x.min(0).tolist(), x.max(0).tolist()))
        assert blob[name + "_lo"].tolist() == lo and blob[name + "_hi"].tolist() == hi, name
        codes = R.quantize(x, lo, hi, BITS[name])
        assert blob[name].dtype == (np.uint16 if BITS[name] == 16 else np.uint8)
        assert np.array_equal(blob[name].astype(F64), codes), name
        assert codes.min() >= 0 and codes.max() <= 2 ** BITS[name] - 1
        decoded = R.dequantize(codes, lo, hi, BITS[name])
        got = back[name].numpy().reshape(n, -1)
        assert got.dtype == F32 and np.array_equal(got.view(np.int32), decoded.view(np.int32)), name
        err = np.abs(x - got.astype(F64))
        assert (err <= R.decode_bound(x, lo, hi, BITS[name])).all(), (name, err.max())
    assert blob["features_dc_lo"][1] == blob["features_dc_hi"][1] == 0.25  # hi == lo: inv = 0, decoded exactly
    assert (back["features_dc"][:, 1] == 0.25).all() and not blob["features_dc"][:, 1].any()
    assert back["features_rest"].shape == p["features_rest"].shape and back["opacities"].shape == (n, 1)
    assert blob["meta"]["sh_degree"] == degree and blob["meta"]["sh_clusters"] == 0 and blob["kmeans"] is None


def _fake_codebook_blob(n=100, k=16, seed=0):
    """A container with a codebook, put together on the host (the clustering itself needs the GPU)."""
    from gs_io.compressed import BITS, compress_gaussians

    rng = np.random.default_rng(seed)
    p = R.gaussian_params(n, 3, seed)
    blob = compress_gaussians(as_torch(p), sh_clusters=0)
    del blob["features_rest"], blob["features_rest_lo"], blob["features_rest_hi"], blob["meta"]["bits"]["features_rest"]
    book = (0.2 * rng.standard_normal((k, 45))).astype(F32)
    lo, hi = float(book.min()), float(book.max())
    blob["sh_codebook"] = R.quantize(book, [lo] * 45, [hi] * 45, 8).astype(np.uint8)
    blob["sh_codebook_lo"], blob["sh_codebook_hi"] = np.asarray([lo]), np.asarray([hi])
    blob["sh_labels"] = rng.integers(0, k, n).astype(np.uint16)
    blob["meta"]["bits"].update(sh_codebook=BITS["sh_codebook"], sh_labels=BITS["sh_labels"])
    blob["meta"]["sh_clusters"] = k
    return blob, book


def test_container_round_trip_bytes_per_gaussian_and_version(tmp_path):
    from gs_io import decompress_gaussians, read_compressed, write_compressed
    from gs_io.compressed import bytes_per_gaussian, compress_gaussians

    blob, book = _fake_codebook_blob()
    assert bytes_per_gaussian(blob["meta"]) == 19 == 6 + 3 + 1 + 3 + 4 + 2
    path = str(tmp_path / "model.npz")
    write_compressed(path, blob)
    assert os.path.exists(path)
    back = read_compressed(path)
    assert back["meta"] == blob["meta"]
    arrays = {k for k, v in blob.items() if isinstance(v, np.ndarray)}
    assert arrays == set(back) - {"meta"}
    for k in arrays:
        assert back[k].dtype == blob[k].dtype and np.array_equal(back[k], blob[k]), k
    a, b = decompress_gaussians(blob), decompress_gaussians(back)
    for k in a:
        assert torch.equal(a[k], b[k])
    lo, hi = [float(blob["sh_codebook_lo"][0])] * 45, [float(blob["sh_codebook_hi"][0])] * 45
    decoded = R.dequantize(blob["sh_codebook"], lo, hi, 8)
    assert (np.abs(decoded.astype(F64) - book) <= R.decode_bound(book, lo, hi, 8)).all()
    want = decoded[blob["sh_labels"].astype(np.int64)].reshape(100, 15, 3)
    assert np.array_equal(a["features_rest"].numpy().view(np.int32), want.view(np.int32))
    # the widths without a codebook, and at degree 0
    assert bytes_per_gaussian(compress_gaussians(as_torch(R.gaussian_params(5, 3, 0)), sh_clusters=0)["meta"]) == 17 + 45
    assert bytes_per_gaussian(compress_gaussians(as_torch(R.gaussian_params(5, 0, 0)), sh_clusters=64)["meta"]) == 17
    # another version, another format, a label outside the codebook
    newer = dict(blob, meta=dict(blob["meta"], version=2))
    with pytest.raises(ValueError, match="write_compressed: container version 2"):
        write_compressed(path, newer)
    with open(path, "wb") as f:
        np.savez_compressed(f, meta=np.asarray(json.dumps(newer["meta"])), means=blob["means"])
    with pytest.raises(ValueError, match="read_compressed: container version 2"):
        read_compressed(path)
    with open(path, "wb") as f:
        np.savez_compressed(f, means=blob["means"])
    with pytest.raises(ValueError, match="read_compressed: not a gs-compressed container"):
        read_compressed(path)
    bad = dict(blob, sh_labels=np.full(100, 16, np.uint16))
    with pytest.raises(ValueError, match="decompress_gaussians: a label points outside the codebook"):
        decompress_gaussians(bad)


def test_an_empty_model_round_trips(tmp_path):
    from gs_io import compress_gaussians, decompress_gaussians, read_compressed, write_compressed

    p = {k: v[:0] for k, v in R.gaussian_params(4, 3, 0).items()}
    blob = compress_gaussians(as_torch(p), sh_clusters=64)  # nothing to cluster: no device needed
    write_compressed(str(tmp_path / "e.npz"), blob)
    back = decompress_gaussians(read_compressed(str(tmp_path / "e.npz")))
    assert back["features_rest"].shape == (0, 15, 3) and back["means"].shape == (0, 3)


# ---- the errors that need no device -------------------------------------------------------------------------------------
def test_compress_refuses_by_name():
    from gs_io import compress_gaussians

    p = as_torch(R.gaussian_params(20, 3, 0))
    with pytest.raises(ValueError, match="compress_gaussians: the parameters are CPU tensors.*no CPU fallback"):
        compress_gaussians(p)
    with pytest.raises(ValueError, match="compress_gaussians: the parameters are CPU tensors"):
        compress_gaussians(p, sh_clusters=8)
    for bad in (-1, 65537, 2.5):
        with pytest.raises(ValueError, match="compress_gaussians: sh_clusters"):
            compress_gaussians(p, sh_clusters=bad)
    for name in p:
        for value in (float("nan"), float("inf")):
            q = {k: v.clone() for k, v in p.items()}
            q[name].view(-1)[3] = value
            with pytest.raises(ValueError, match=f"compress_gaussians: {name} holds values that are not finite"):
                compress_gaussians(q, sh_clusters=0)
    q = dict(p)
    del q["scales"]
    with pytest.raises(ValueError, match="compress_gaussians: params has no 'scales'"):
        compress_gaussians(q, sh_clusters=0)
    with pytest.raises(ValueError, match="compress_gaussians: means must hold"):
        compress_gaussians(dict(p, means=p["means"][:, :2]), sh_clusters=0)
    with pytest.raises(ValueError, match="compress_gaussians: features_rest has 14 bands"):
        compress_gaussians(dict(p, features_rest=p["features_rest"][:, :14]), sh_clusters=0)
    with pytest.raises(ValueError, match="compress_gaussians: quats holds a zero quaternion"):
        compress_gaussians(dict(p, quats=torch.zeros(20, 4)), sh_clusters=0)


def test_kmeans_ops_refuse_cpu_tensors_and_bad_sizes_by_name():
    from gs_fused import kmeans, kmeans_assign, kmeans_inertia, kmeans_update

    x, c = torch.zeros(10, 3), torch.zeros(2, 3)
    labels = torch.zeros(10, dtype=torch.int32)
    for op, call in (("kmeans_assign", lambda: kmeans_assign(x, c)),
                     ("kmeans_update", lambda: kmeans_update(x, labels, c)),
                     ("kmeans_inertia", lambda: kmeans_inertia(x, c, labels)),
                     ("kmeans", lambda: kmeans(x, 2))):
        with pytest.raises(ValueError, match=f"{op}: points is a CPU tensor.*no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="kmeans_assign: points must be a tensor"):
        kmeans_assign(x.numpy(), c)
    with pytest.raises(ValueError, match="kmeans: K = 0; need K >= 1"):
        kmeans(x, 0)
    with pytest.raises(ValueError, match="kmeans: K = 65537; K <= 65536"):
        kmeans(x, 65537)
    with pytest.raises(ValueError, match="kmeans: iters = -1"):
        kmeans(x, 2, iters=-1)


# ---- the native entries and the tool ------------------------------------------------------------------------------------
def test_prototypes_of_the_three_entries():
    from rasterizer.cuda._prototypes import PROTOTYPES

    assert PROTOTYPES["gsr_kmeans_assign"] == ("i", "iiippppp")
    assert PROTOTYPES["gsr_kmeans_update"] == ("i", "iii" + 9 * "p")
    assert PROTOTYPES["gsr_kmeans_inertia"] == ("i", "iii" + 7 * "p")


def test_native_entries_validate_before_any_launch():
    """(entries that reject on the host before they touch a device, as test_argument_validation_needs_no_gpu)"""
    from rasterizer.cuda import _call

    for bad in ((4, 0, 2), (4, 49, 2), (4, 3, 0), (4, 3, 65537), (-1, 3, 2)):
        with pytest.raises(RuntimeError, match="kmeans_assign: need num_points >= 0, 1 <= dim <= 48"):
            _call("gsr_kmeans_assign", *bad, None, None, None, None, None)
    with pytest.raises(RuntimeError, match="kmeans_assign: null pointer"):
        _call("gsr_kmeans_assign", 4, 3, 2, None, None, None, None, None)
    with pytest.raises(RuntimeError, match="kmeans_update: null pointer"):
        _call("gsr_kmeans_update", 4, 3, 2, None, None, None, None, None, None, None, None, None)
    with pytest.raises(RuntimeError, match="kmeans_inertia: null pointer"):
        _call("gsr_kmeans_inertia", 4, 3, 2, None, None, None, None, None, None, None)
    _call("gsr_kmeans_assign", 0, 3, 2, None, None, None, None, None)  # N = 0: nothing to do


def test_tool_arguments():
    tool = _tool()
    a = tool.parse_args(["ckpts", "out.npz"])
    assert (a.source, a.out, a.sh_clusters, a.iters, a.seed, a.device) == ("ckpts", "out.npz", 16384, 10, 0, "cuda:0")
    assert not a.decompress and a.dataset is None and a.split == "val" and a.weights_from_dataset is None
    a = tool.parse_args(["g.ply", "o.npz", "--sh-clusters", "4096", "--iters", "3", "--seed", "7",
                         "--weights-from-dataset", "data", "--dataset", "data", "--split", "test", "--device", "cuda:1"])
    assert (a.sh_clusters, a.iters, a.seed, a.weights_from_dataset, a.dataset, a.split, a.device) == \
        (4096, 3, 7, "data", "data", "test", "cuda:1")
    a = tool.parse_args(["--decompress", "in.npz", "out.ply"])
    assert a.decompress and (a.source, a.out) == ("in.npz", "out.ply")
    for bad in (["ckpts", "out.ply"], ["--decompress", "in.npz", "out.npz"], ["c", "o.npz", "--sh-clusters", "65537"],
                ["c", "o.npz", "--sh-clusters", "-1"], ["c", "o.npz", "--iters", "-2"], ["c"]):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)


def test_tool_compresses_a_ply_without_a_codebook_on_the_host(tmp_path, capsys):
    from gs_io import decompress_gaussians, read_compressed, write_gaussian_ply

    p = R.gaussian_params(50, 2, seed=4)
    ply, out = str(tmp_path / "g.ply"), str(tmp_path / "g.npz")
    write_gaussian_ply(ply, p)
    summary = _tool().main([ply, out, "--sh-clusters", "0", "--device", "cpu"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == summary
    assert summary["gaussians"] == 50 and summary["sh_clusters"] == 0 and summary["inertia"] is None
    assert summary["bytes_raw"] == 50 * (14 + 24) * 4 and summary["bytes_per_gaussian"] == 17 + 24
    assert summary["bytes_on_disk"] == os.path.getsize(out) < os.path.getsize(ply)
    back = decompress_gaussians(read_compressed(out))
    assert back["features_rest"].shape == (50, 8, 3)
    assert float((back["means"] - torch.from_numpy(p["means"])).abs().max()) <= 8.0 / 65535 * 0.5001 + 1e-6


def test_tool_decompress_writes_the_ply(tmp_path, capsys):
    from gs_io import decompress_gaussians, read_gaussian_ply, write_compressed

    blob, _ = _fake_codebook_blob()
    src, out = str(tmp_path / "m.npz"), str(tmp_path / "m.ply")
    write_compressed(src, blob)
    summary = _tool().main(["--decompress", src, out])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == summary
    assert summary["gaussians"] == 100 and summary["sh_clusters"] == 16
    ply, want = read_gaussian_ply(out), decompress_gaussians(blob)
    for k, v in want.items():
        assert np.array_equal(ply[k].reshape(v.shape), v.numpy()), k
    assert os.path.getsize(src) < os.path.getsize(out)
