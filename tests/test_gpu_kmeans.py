"""GPU: k-means (csrc/kmeans.hip, gs_fused.kmeans) and the compressed container (gs_io.compressed); DESIGN.md section
4.24.  The assignment bit for bit against the float32 restatement; the update and the inertia against float64 within
the reordering bound of a float64 sum, and bit-identical from run to run; Lloyd's descent of the float64 inertia; the
codec on the device against the host; one small model end to end through the file and the renderer."""
import os

import numpy as np
import pytest
import torch

import kmeans_reference as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def dev():
    return torch.device("cuda", 0)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def same_bits(a: torch.Tensor, b) -> bool:
    b = b if isinstance(b, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(b))
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    as_int = {torch.float32: torch.int32, torch.float64: torch.int64}.get(a.dtype)
    return torch.equal(a.view(as_int), b.view(as_int)) if as_int is not None else torch.equal(a, b)


# ---- assign -----------------------------------------------------------------------------------------------------------
def _assign_cases():
    """The cross product N x K x D thinned to a Latin square: every (N, K) pair, D cycling, every value of each axis."""
    from gs_fused.kmeans import TILE as T

    ns, ks, ds = (1, 63, 64, 65, 257, 1000), (1, 2, 7, T, T + 1, 2 * T + 3), (1, 3, 9, 24, 45, 48)
    return [(n, k, ds[(i + j) % 6]) for i, n in enumerate(ns) for j, k in enumerate(ks)]


@pytest.mark.parametrize("n,k,d", _assign_cases())
def test_assign_equals_the_float32_restatement_bit_for_bit(n, k, d):
    from gs_fused import kmeans_assign
    from gs_fused.kmeans import TILE as T

    x, c = R.assign_case(n, k, d, seed=1000 * n + 10 * k + d, tile=T)
    want_labels, want_dist = R.assign(x, c)
    # by construction, and checked: the edges of the rule occur
    assert want_labels[0] == 0 and want_dist[0] == 0                               # a point on a centroid
    if n > 4:
        assert np.isnan(x[1]).all() and want_labels[1] == 0 and np.isinf(want_dist[1])  # a row of NaN
        assert np.isinf(x[2]).all() and want_labels[2] == 0 and np.isinf(want_dist[2])  # a row of +inf
        if k > 1:
            assert R.tied_rows(x, c)[0] and (c[0] == c[1]).all()                   # duplicates: the lower index
        if k > 3:
            assert np.isnan(c[2]).all() and not (want_labels == 2).any()           # a NaN centroid never wins
        if k > T:
            assert (c[T] == c[T - 1]).all() and want_labels[3] == T - 1 and want_dist[3] == 0  # across the boundary
    labels, dist = kmeans_assign(cu(x), cu(c))
    assert labels.dtype == torch.int32 and dist.dtype == torch.float32 and labels.shape == dist.shape == (n,)
    bad = np.flatnonzero(labels.cpu().numpy() != want_labels)
    assert bad.size == 0, (bad[:5], labels.cpu().numpy()[bad[:5]], want_labels[bad[:5]])
    assert same_bits(dist, want_dist), np.flatnonzero(dist.cpu().numpy().view(np.int32) != want_dist.view(np.int32))[:5]


def test_assign_through_strided_views_and_twice():
    from gs_fused import kmeans_assign

    x, c = R.assign_case(300, 40, 9, seed=5, tile=128)
    wide_x, wide_c = cu(np.concatenate([x, x], 1)), cu(np.concatenate([c, c], 1))
    a = kmeans_assign(cu(x), cu(c))
    b = kmeans_assign(wide_x[:, :9], wide_c[:, 9:])
    assert torch.equal(a[0], b[0]) and same_bits(a[1], b[1])


# ---- update -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("d", [1, 5, 45, 48])
def test_update_against_float64_counts_empty_clusters_and_reproducibility(d, weighted):
    from gs_fused import kmeans_update

    x, labels, old, w = R.update_case(d, seed=d + 7 * weighted, weighted=weighted)
    want = R.update(x, labels, old, w)
    assert want["counts"].tolist() == list(R.UPDATE_SIZES)  # clusters of 0, 1, 63, 64, 65 and 1000 members
    assert want["kept"].tolist() == [s == 0 or (weighted and s == 7) for s in R.UPDATE_SIZES]
    args = (cu(x), cu(labels), cu(old), None if w is None else cu(w))
    new, counts = kmeans_update(*args)
    assert new.dtype == torch.float32 and new.shape == old.shape and counts.dtype == torch.int32
    assert counts.cpu().tolist() == want["counts"].tolist()
    got = new.cpu().numpy()
    kept = want["kept"]
    assert np.array_equal(got[kept].view(np.int32), old[kept].view(np.int32))  # the old centroid's bits
    # float32 rounding of the quotient + the reordering of a float64 sum of n_c terms of mean magnitude `scale`
    m, n_c = want["mean"], want["counts"].astype(F64)[:, None]
    bound = 2.0 ** -24 * np.abs(m) + n_c * 2.0 ** -52 * want["scale"]
    err = np.abs(got.astype(F64) - m)
    print(f"update d={d} weighted={weighted}: max err / bound = {(err[~kept] / bound[~kept]).max():.3f}")
    assert (err[~kept] <= bound[~kept]).all(), (err[~kept] / bound[~kept]).max()
    again, counts2 = kmeans_update(*args)
    assert same_bits(again, new) and torch.equal(counts2, counts)


def test_update_ignores_labels_outside_the_clusters():
    from gs_fused import kmeans_update

    x, labels, old, _ = R.update_case(6, seed=2, weighted=False)
    k = old.shape[0]
    stray = labels.copy()
    stray[labels == 5] = k + 3
    stray[labels == 4] = -2
    new, counts = kmeans_update(cu(x), cu(stray), cu(old))
    ref, _ = kmeans_update(cu(x), cu(labels), cu(old))
    assert counts.cpu().tolist() == [0 if c in (4, 5) else s for c, s in enumerate(R.UPDATE_SIZES)]
    for c in range(k):
        assert same_bits(new[c], cu(old)[c] if c in (4, 5) else ref[c]), c


# ---- inertia ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n,d", [(1, 1), (65, 3), (1025, 45), (3000, 48)])
def test_inertia_against_float64_and_twice(n, d, weighted):
    from gs_fused import kmeans_inertia

    rng = np.random.default_rng(n + d)
    x, c = rng.standard_normal((n, d)).astype(F32), rng.standard_normal((11, d)).astype(F32)
    labels = rng.integers(0, 11, n).astype(np.int32)
    w = rng.uniform(0, 2, n).astype(F32) if weighted else None
    want = R.inertia(x, c, labels, w)
    args = (cu(x), cu(c), cu(labels), None if w is None else cu(w))
    got = kmeans_inertia(*args)
    assert got.dtype == torch.float64 and got.dim() == 0 and got.is_cuda
    print(f"inertia n={n} d={d}: relative difference {abs(float(got) - want) / want:.3e}, bound {n * 2.0 ** -52:.3e}")
    assert abs(float(got) - want) <= n * 2.0 ** -52 * want
    assert same_bits(kmeans_inertia(*args).reshape(1), got.reshape(1))


# ---- the loop -----------------------------------------------------------------------------------------------------------
def test_loop_descends_is_reproducible_and_ends_on_an_assignment():
    from gs_fused import kmeans, kmeans_assign, kmeans_inertia
    from gs_fused.kmeans import initial_centroids

    n, d, k, iters = 1000, 45, 37, 8
    x = R.loop_case(n, d)
    assert (x[-50:] == x[:50]).all()
    xs = cu(x)
    res = kmeans(xs, k, iters=iters, seed=4)
    assert res.centroids.shape == (k, d) and res.labels.shape == (n,) and res.counts.shape == (k,)
    assert res.inertia.shape == (iters + 1,) and res.inertia.dtype == torch.float64
    labels, _ = kmeans_assign(xs, res.centroids)
    assert torch.equal(res.labels, labels)
    assert res.counts.cpu().tolist() == np.bincount(labels.cpu().numpy(), minlength=k).tolist()
    assert same_bits(res.inertia[-1:], kmeans_inertia(xs, res.centroids, res.labels).reshape(1))
    inertia = res.inertia.cpu().numpy()
    print("inertia:", inertia.tolist())
    allow = 1.0 + 4.0 * (d + 2) * 2.0 ** -24  # Lloyd's descent, assigning by a float32 distance
    assert (inertia[1:] <= inertia[:-1] * allow).all() and inertia[-1] < inertia[0]
    init = initial_centroids(torch.from_numpy(x), k, 4).numpy()
    want0 = R.inertia(x, init, R.assign(x, init)[0])
    assert abs(inertia[0] - want0) <= n * 2.0 ** -52 * want0  # the CPU generator's rows, the restatement's labels
    again = kmeans(xs, k, iters=iters, seed=4)
    given = kmeans(xs, k, iters=iters, seed=99, init=initial_centroids(xs, k, 4))
    for other in (again, given):
        for a, b in zip(res, other):
            assert same_bits(a, b)
    assert not same_bits(kmeans(xs, k, iters=iters, seed=5).centroids, res.centroids)
    # weights enter the means and the inertia, not the assignment
    w = cu(np.random.default_rng(0).uniform(0, 1, n).astype(F32))
    weighted = kmeans(xs, k, iters=1, seed=4, weights=w)
    first, _ = kmeans_assign(xs, initial_centroids(xs, k, 4))
    assert same_bits(weighted.inertia[:1], kmeans_inertia(xs, initial_centroids(xs, k, 4), first, w).reshape(1))


def test_loop_with_more_clusters_than_points_and_without_iterations():
    from gs_fused import kmeans

    x = R.loop_case(100, 9)
    res = kmeans(cu(x), 500, iters=2, seed=1)
    assert res.centroids.shape == (100, 9) and res.counts.shape == (100,)
    assert float(res.inertia[-1]) == 0.0 and float(res.inertia[0]) == 0.0
    assert int(res.counts.sum()) == 100
    none = kmeans(cu(x), 7, iters=0, seed=1)
    assert none.inertia.shape == (1,) and float(none.inertia[0]) > 0


# ---- errors and empty inputs --------------------------------------------------------------------------------------------
def test_errors_by_name_and_empty_inputs():
    from gs_fused import kmeans, kmeans_assign, kmeans_inertia, kmeans_update

    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev())  # noqa: E731
    x, c, labels = z(10, 3), z(2, 3), z(10, dtype=torch.int32)
    cases = [
        ("kmeans_assign: points must be float32", lambda: kmeans_assign(z(10, 3, dtype=torch.float64), c)),
        ("kmeans_assign: points must be float32", lambda: kmeans_assign(z(10), c)),
        ("kmeans_assign: points have D = 49 columns", lambda: kmeans_assign(z(10, 49), z(2, 49))),
        ("kmeans_assign: centroids must be float32 \\[\\*,3\\]", lambda: kmeans_assign(x, z(2, 4))),
        ("kmeans_assign: centroids must be float32", lambda: kmeans_assign(x, z(2, 3, dtype=torch.float16))),
        ("kmeans_assign: K = 0; need K >= 1", lambda: kmeans_assign(x, z(0, 3))),
        ("kmeans_assign: K = 65537; K <= 65536", lambda: kmeans_assign(x, z(65537, 3))),
        ("kmeans_assign: centroids is a CPU tensor", lambda: kmeans_assign(x, c.cpu())),
        ("kmeans_update: labels must be torch.int32 \\[10\\]", lambda: kmeans_update(x, labels.long(), c)),
        ("kmeans_update: labels must be torch.int32 \\[10\\]", lambda: kmeans_update(x, labels[:9], c)),
        ("kmeans_update: labels is a CPU tensor", lambda: kmeans_update(x, labels.cpu(), c)),
        ("kmeans_update: weights must be torch.float32 \\[10\\]", lambda: kmeans_update(x, labels, c, z(9))),
        ("kmeans_update: weights must be finite and >= 0", lambda: kmeans_update(x, labels, c, z(10) - 1)),
        ("kmeans_inertia: weights must be finite and >= 0",
         lambda: kmeans_inertia(x, c, labels, z(10) + float("inf"))),
        ("kmeans: weights must be finite and >= 0", lambda: kmeans(x, 2, weights=z(10) + float("nan"))),
        ("kmeans: weights is a CPU tensor", lambda: kmeans(x, 2, weights=torch.zeros(10))),
        ("kmeans: init must be float32 \\[2,3\\]", lambda: kmeans(x, 2, init=z(3, 3))),
        ("kmeans: points have D = 49 columns", lambda: kmeans(z(10, 49), 2)),
    ]
    for match, call in cases:
        with pytest.raises(ValueError, match=match):
            call()
    labels0, dist0 = kmeans_assign(z(0, 3), c)
    assert labels0.shape == dist0.shape == (0,) and labels0.dtype == torch.int32 and dist0.is_cuda
    new, counts = kmeans_update(z(0, 3), z(0, dtype=torch.int32), c + 2)
    assert same_bits(new, c + 2) and counts.cpu().tolist() == [0, 0]
    assert float(kmeans_inertia(z(0, 3), c, z(0, dtype=torch.int32))) == 0.0
    res = kmeans(z(0, 3), 4, iters=3)
    assert res.centroids.shape == (0, 3) and res.labels.shape == (0,) and res.counts.shape == (0,)
    assert res.inertia.cpu().tolist() == [0.0] * 4


# ---- the codec on the device ----------------------------------------------------------------------------------------------
def test_codec_on_the_device_equals_the_host():
    from gs_io import compress_gaussians, decompress_gaussians

    p = R.gaussian_params(300, 3, seed=11)
    host = compress_gaussians({k: torch.from_numpy(v) for k, v in p.items()}, sh_clusters=0)
    device = compress_gaussians({k: cu(v) for k, v in p.items()}, sh_clusters=0)
    assert host["meta"] == device["meta"]
    arrays = [k for k, v in host.items() if isinstance(v, np.ndarray)]
    assert "features_rest" in arrays and len(arrays) == 18
    for k in arrays:
        assert host[k].dtype == device[k].dtype and np.array_equal(host[k], device[k]), k
    a, b = decompress_gaussians(host), decompress_gaussians(device, device=dev())
    for k in a:
        assert b[k].is_cuda and same_bits(a[k], b[k]), k


def test_codebook_labels_and_decoded_rows():
    from gs_fused import kmeans
    from gs_io import compress_gaussians, decompress_gaussians
    from gs_io.compressed import bytes_per_gaussian

    n, k = 400, 24
    p = R.gaussian_params(n, 3, seed=12)
    w = np.random.default_rng(1).uniform(0, 3, n).astype(F32)
    for weights in (None, cu(w)):
        blob = compress_gaussians({name: cu(v) for name, v in p.items()}, sh_clusters=k, iters=4, seed=2,
                                  weights=weights)
        assert blob["meta"]["sh_clusters"] == k and bytes_per_gaussian(blob["meta"]) == 19
        assert blob["sh_labels"].dtype == np.uint16 and blob["sh_codebook"].shape == (k, 45)
        assert "features_rest" not in blob and len(blob["kmeans"]["inertia"]) == 5
        rows = p["features_rest"].reshape(n, 45)
        res = kmeans(cu(rows), k, iters=4, seed=2, weights=weights)  # bit-reproducible: the centroids behind the blob
        assert blob["kmeans"]["inertia"] == res.inertia.cpu().tolist()
        cents = res.centroids.cpu().numpy()
        assert np.array_equal(blob["sh_labels"].astype(np.int32), R.assign(rows, cents)[0])
        lo, hi = [float(F64(cents.min()))] * 45, [float(F64(cents.max()))] * 45
        assert blob["sh_codebook_lo"].tolist() == lo[:1] and blob["sh_codebook_hi"].tolist() == hi[:1]
        codes = R.quantize(cents, lo, hi, 8)
        assert np.array_equal(blob["sh_codebook"].astype(F64), codes)
        decoded = R.dequantize(codes, lo, hi, 8)
        assert (np.abs(decoded.astype(F64) - cents) <= R.decode_bound(cents, lo, hi, 8)).all()
        back = decompress_gaussians(blob)["features_rest"].numpy()
        want = decoded[blob["sh_labels"].astype(np.int64)].reshape(n, 15, 3)
        assert np.array_equal(back.view(np.int32), want.view(np.int32))


# ---- the tool ---------------------------------------------------------------------------------------------------------------
def test_tool_on_a_checkpoint_with_contribution_weights_and_a_dataset(tmp_path, capsys):
    import importlib.util
    import json
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import make_synthetic_dataset as M

    import harness.train as HT
    from gs_io import read_gaussian_ply

    spec = importlib.util.spec_from_file_location("compress_gaussians_tool",
                                                  os.path.join(root, "tools", "compress_gaussians.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    directory, ckpt = str(tmp_path / "dataset"), str(tmp_path / "ckpt")
    os.makedirs(directory)
    M.make_synthetic_dataset(directory, 12, 64, 48, alpha=True, device="cuda:0")
    HT.train(HT.TrainConfig(dataset=directory, checkpoint_dir=ckpt, save_every=9, dataset_eval_split=None, iters=10,
                            num_downscales=1, resolution_schedule=20, background_color="random", sh_degree=1,
                            sh_degree_interval=2, log_every=1), dev())
    out, ply = str(tmp_path / "model.npz"), str(tmp_path / "model.ply")
    capsys.readouterr()
    summary = tool.main([ckpt, out, "--sh-clusters", "32", "--iters", "3", "--weights-from-dataset", directory,
                         "--dataset", directory, "--split", "val"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == summary
    assert summary["sh_clusters"] == 32 and summary["bytes_per_gaussian"] == 19 and len(summary["inertia"]) == 4
    assert summary["inertia"][-1] <= summary["inertia"][0] * (1 + 4 * 11 * 2.0 ** -24)
    assert summary["bytes_on_disk"] == os.path.getsize(out) < summary["bytes_raw"]
    ev = summary["evaluation"]
    print("tool:", json.dumps(ev))
    assert ev["num_images"] >= 1 and all(np.isfinite([ev["raw"]["psnr"], ev["compressed"]["psnr"], ev["psnr_between"]]))
    back = tool.main(["--decompress", out, ply])
    assert back["gaussians"] == summary["gaussians"]
    assert read_gaussian_ply(ply)["features_rest"].shape == (summary["gaussians"], 3, 3)


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_small_model_through_the_file_and_the_renderer(tmp_path):
    from gs_io import (compress_gaussians, decompress_gaussians, read_compressed, write_compressed,
                       write_gaussian_ply)
    from harness import scene as S
    from harness.pipeline import CameraTensors, render_view

    cam = S.make_camera(64, 48, yaw=0.1, pitch=-0.05)
    n = 400
    sc = S.make_scene(n, cam, sh_degree=3, seed=3, scale_lo=0.05, scale_hi=0.3)
    op = sc["opacities"].astype(F64)
    raw = {"means": sc["means3d"], "scales": np.log(sc["scales"]), "quats": sc["quats"],
           "opacities": np.log(op / (1.0 - op)), "features_dc": sc["sh_coeffs"][:, 0, :],
           "features_rest": sc["sh_coeffs"][:, 1:, :]}
    raw = {k: np.ascontiguousarray(v, dtype=F32) for k, v in raw.items()}
    blob = compress_gaussians({k: cu(v) for k, v in raw.items()}, sh_clusters=64, iters=5)
    npz, ply = str(tmp_path / "model.npz"), str(tmp_path / "model.ply")
    write_compressed(npz, blob)
    write_gaussian_ply(ply, raw)
    assert os.path.getsize(npz) < os.path.getsize(ply)
    restored = decompress_gaussians(read_compressed(npz), device=dev())
    assert restored["features_rest"].shape == (n, 15, 3)
    bg = torch.tensor(S.BACKGROUND, device=dev())
    images = []
    for p in ({k: cu(v) for k, v in raw.items()}, restored):
        q = p["quats"] / p["quats"].norm(dim=-1, keepdim=True)
        out = render_view(p["means"], torch.exp(p["scales"]), q, torch.sigmoid(p["opacities"]),
                          torch.cat([p["features_dc"][:, None, :], p["features_rest"]], dim=1).contiguous(),
                          CameraTensors.from_numpy(cam, dev()), bg, 3)
        images.append(out["rgb"])
    a, b = images
    assert a.shape == b.shape == (48, 64, 3) and bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    assert float((a - bg).abs().max()) > 0.05  # something was drawn
    mse = float(((a - b) ** 2).mean())
    print(f"{n} Gaussians, 64 clusters: {os.path.getsize(ply)} B PLY, {os.path.getsize(npz)} B compressed, "
          f"PSNR raw vs compressed {10 * np.log10(1.0 / mse):.2f} dB")
