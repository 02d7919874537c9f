"""CPU: the host side of the TSDF exporter -- argument validation of every `gsr_tsdf_*` entry before any device use,
the trajectory and PLY files, and the float32 NumPy oracle (tests/tsdf_reference.py) checked against the analytic
sphere it fuses.

Sphere scene (tsdf_reference.sphere_*): radius 0.5, 14 cameras at distance 1.5 on the cube-face and cube-corner
directions, 160x160, analytic z-depth, colour 0.5 + 0.5 n, background and grazing (cos < 0.35) pixels invalid,
L = 1/64, sdf_trunc = 4 L.  The principal point is (80.37, 79.79): with it at (80, 80) the voxel centres on the
symmetry planes of the corner cameras project exactly onto pixel borders (4.7 % of all updates flagged ambiguous).
Measured on the oracle alone: 19 472 points, worst |r - 0.5| = 0.256 L; mesh 19 474 vertices / 38 944 triangles, worst
0.243 L, closed, oriented, V - E + F = 2, volume 4.2e-5 below the sphere's; 5.5e-4 of the updates flagged ambiguous.

Noise scene (tsdf_reference.noise_*): 16 x 12 x 16 = 3072 blocks, five 317 x 203 views of per-pixel random depth, so
that the kernels that loop over blocks with 2048 workgroups go round a second time; the coverage conditions the GPU
tests rely on are asserted here, on the oracle alone.  Measured: per-view lists of 2974 / 2893 / 877 / 2925 / 2684
blocks, 3065 allocated, 2.41 M voxel updates of which 3.9e-4 flagged ambiguous; with capacity 2500 the first view
fills the pool (2974 wanted), `needed` ends at 3060.

`dense_fusion_f64` is the rule in plain float64 over every voxel, written apart from the oracle.  Measured distances
of the float32 oracle from it over stable voxels (tsdf / colour): sphere 1.6e-6 / 7.9e-8, room 1.9e-6 / 3.0e-8, noise
3.9e-6 / 1.1e-7; unstable shares 0.55 % / 0.13 % / 0.17 %; no weight differs and no in-band update lies outside the
list of its view.
"""
import ctypes as C
import functools
import json
import math
import threading
import warnings

import numpy as np
import pytest

import tsdf_reference as R


# ---- C ABI -----------------------------------------------------------------------------------------------------------
FAKE = 0x10000  # a non-null address that must never be dereferenced: every call below fails (or ends) on the host


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


def _descs(blocks=(4, 4, 4), L=0.01, trunc=0.04, capacity=8, H=8, W=8, null_pool=False, null_image=False):
    from gs_fusion.volume import _View, _Volume

    p = None if null_pool else FAKE
    vol = _Volume((C.c_float * 3)(0, 0, 0), L, trunc, (C.c_int * 3)(*blocks), capacity, p, p, p, p, p)
    eye = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
    q = None if null_image else FAKE
    view = _View(H, W, 10.0, 10.0, 4.0, 4.0, 10.0, (C.c_float * 12)(*eye), (C.c_float * 12)(*eye), q, q, None)
    return vol, view


def _entries(L, vol, view, n=4):
    p, ws = C.c_void_p(FAKE), C.c_size_t(1 << 30)
    return {
        "touch": lambda: L.gsr_tsdf_touch(C.byref(vol), C.byref(view), p, None),
        "allocate": lambda: L.gsr_tsdf_allocate(C.byref(vol), p, p, p, ws, None),
        "integrate": lambda: L.gsr_tsdf_integrate(C.byref(vol), C.byref(view), p, None),
        "points_count": lambda: L.gsr_tsdf_extract_points_count(C.byref(vol), p, ws, None),
        "points_emit": lambda: L.gsr_tsdf_extract_points_emit(C.byref(vol), p, ws, C.c_int(n), p, p, p, p, None),
        "mesh_count": lambda: L.gsr_tsdf_extract_mesh_count(C.byref(vol), p, ws, None),
        "mesh_emit": lambda: L.gsr_tsdf_extract_mesh_emit(C.byref(vol), p, ws, C.c_int(n), C.c_int(n), p, p, p, None),
    }


@pytest.mark.parametrize("bad,word", [(dict(blocks=(4, 0, 4)), b"blocks"), (dict(blocks=(-1, 4, 4)), b"blocks"),
                                       (dict(L=0.0), b"voxel length"), (dict(L=-1.0), b"voxel length"),
                                       (dict(capacity=0), b"capacity"), (dict(trunc=0.0), b"sdf_trunc"),
                                       (dict(null_pool=True), b"null volume buffer")])
@in_own_thread
def test_every_entry_rejects_a_bad_volume(bad, word):
    from rasterizer.cuda._backend import lib

    L = lib()
    vol, view = _descs(**bad)
    for name, call in _entries(L, vol, view).items():
        assert call() == -1, name
        assert word in L.gsr_last_error(), (name, L.gsr_last_error())


@in_own_thread
def test_bad_views_null_pointers_and_zero_work():
    from rasterizer.cuda._backend import lib

    L = lib()
    p, ws = C.c_void_p(FAKE), C.c_size_t(1 << 30)
    for bad, word in ((dict(H=0, W=0), b"empty image"), (dict(H=0), b"empty image"), (dict(null_image=True), b"null image")):
        vol, view = _descs(**bad)
        e = _entries(L, vol, view)
        for name in ("touch", "integrate"):
            assert e[name]() == -1 and word in L.gsr_last_error(), (name, L.gsr_last_error())
    vol, view = _descs()
    assert L.gsr_tsdf_touch(None, C.byref(view), p, None) == -1 and b"null volume" in L.gsr_last_error()
    assert L.gsr_tsdf_touch(C.byref(vol), None, p, None) == -1 and b"null view" in L.gsr_last_error()
    assert L.gsr_tsdf_touch(C.byref(vol), C.byref(view), None, None) == -1 and b"null flags" in L.gsr_last_error()
    assert L.gsr_tsdf_allocate(C.byref(vol), None, p, p, ws, None) == -1 and b"null pointer" in L.gsr_last_error()
    assert L.gsr_tsdf_allocate(C.byref(vol), p, None, p, ws, None) == -1
    assert L.gsr_tsdf_integrate(C.byref(vol), C.byref(view), None, None) == -1 and b"null list" in L.gsr_last_error()
    # outputs missing for a non-zero count
    assert L.gsr_tsdf_extract_points_emit(C.byref(vol), p, ws, C.c_int(3), None, p, p, p, None) == -1
    assert b"null output" in L.gsr_last_error()
    assert L.gsr_tsdf_extract_mesh_emit(C.byref(vol), p, ws, C.c_int(3), C.c_int(2), p, None, p, None) == -1
    assert L.gsr_tsdf_extract_mesh_emit(C.byref(vol), p, ws, C.c_int(3), C.c_int(2), p, p, None, None) == -1
    assert L.gsr_tsdf_extract_points_emit(C.byref(vol), p, ws, C.c_int(-1), p, p, p, p, None) == -1
    # workspace: missing or too small (-3, like the other entries), before anything is launched
    assert L.gsr_tsdf_allocate(C.byref(vol), p, p, None, ws, None) == -3
    assert L.gsr_tsdf_allocate(C.byref(vol), p, p, p, C.c_size_t(8), None) == -3 and b"workspace" in L.gsr_last_error()
    assert L.gsr_tsdf_extract_points_count(C.byref(vol), p, C.c_size_t(8), None) == -3
    assert L.gsr_tsdf_extract_mesh_count(C.byref(vol), None, ws, None) == -3
    # zero work: nothing to emit is a no-op, with no buffers at all
    assert L.gsr_tsdf_extract_points_emit(C.byref(vol), None, C.c_size_t(0), C.c_int(0), None, None, None, None, None) == 0
    assert L.gsr_tsdf_extract_mesh_emit(C.byref(vol), None, C.c_size_t(0), C.c_int(0), C.c_int(0), None, None, None, None) == 0
    assert L.gsr_tsdf_allocate_workspace_bytes(C.c_int(0)) == 0
    assert L.gsr_tsdf_extract_points_workspace_bytes(C.c_int(0)) == 0
    assert L.gsr_tsdf_extract_mesh_workspace_bytes(C.c_int(0), C.c_int(4)) == 0
    assert L.gsr_tsdf_extract_mesh_workspace_bytes(C.c_int(4), C.c_int(0)) == 0


def test_workspace_sizes_are_monotone():
    from rasterizer.cuda._backend import lib

    L = lib()
    sizes = [1, 2, 63, 64, 1000, 4096, 262144, 1 << 24]
    for fn in (L.gsr_tsdf_allocate_workspace_bytes, L.gsr_tsdf_extract_points_workspace_bytes,
               lambda n: L.gsr_tsdf_extract_mesh_workspace_bytes(n, C.c_int(100))):
        got = [fn(C.c_int(n)) for n in sizes]
        assert got[0] > 0 and all(a <= b for a, b in zip(got, got[1:])), got
        assert got[-1] >= 4 * sizes[-1]
    caps = [L.gsr_tsdf_extract_mesh_workspace_bytes(C.c_int(1000), C.c_int(c)) for c in (1, 10, 1000, 100000)]
    assert all(a < b for a, b in zip(caps, caps[1:])) and caps[-1] >= 100000 * 512 * 4


def test_volume_and_cpu_tensors_are_rejected_on_the_host():
    import torch

    from gs_fusion import TSDFVolume

    with pytest.raises(RuntimeError):
        TSDFVolume(0.01, 0.04, (0, 0, 0), (2, 2, 2), 8, device="cpu")
    with pytest.raises(ValueError):
        TSDFVolume(0.01, 0.04, (0, 0, 0), (2, 0, 2), 8)
    with pytest.raises(ValueError):
        TSDFVolume(0.0, 0.04, (0, 0, 0), (2, 2, 2), 8)
    # integrate checks its tensors before it touches the volume (no GPU needed to see that)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        TSDFVolume.integrate(None, torch.zeros(4, 4), torch.zeros(4, 4, 3), 1, 1, 2, 2, np.eye(4))


# ---- files -----------------------------------------------------------------------------------------------------------
def test_read_poses_json(tmp_path):
    from gs_fusion import read_poses_json

    rng = np.random.default_rng(0)
    entries, poses = [], []
    for k in range(2):
        V = R.look_at(rng.uniform(-2, 2, 3), rng.uniform(-0.2, 0.2, 3)).astype(np.float64)
        pose = np.linalg.inv(V)
        poses.append(pose)
        entries.append({"pose": pose.tolist(), "camera": {"width": 64 + 16 * k, "height": 48, "fx": 70.0 + k, "fy": 71.5,
                                                          "cx": 31.5, "cy": 24.25}})
    path = tmp_path / "poses.json"
    path.write_text(json.dumps(entries))
    cams = read_poses_json(str(path))
    assert len(cams) == 2
    for k, cam in enumerate(cams):
        assert (cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy) == (64 + 16 * k, 48, 70.0 + k, 71.5, 31.5, 24.25)
        want = np.linalg.inv(poses[k]).astype(np.float32)
        assert cam.viewmat.dtype == np.float32 and np.array_equal(cam.viewmat, want)
        assert np.allclose(cam.campos, poses[k][:3, 3], atol=1e-5)
        # the projection of the rasterizer's cameras (harness.scene.make_camera): w_clip = z_view
        p = cam.projmat @ np.array([0.1, -0.2, 0.3, 1.0], np.float32)
        z = (cam.viewmat @ np.array([0.1, -0.2, 0.3, 1.0], np.float32))[2]
        assert abs(p[3] - z) < 1e-5


def test_geometry_ply_round_trip(tmp_path):
    from gs_io import read_mesh_ply, read_point_cloud_ply, write_mesh_ply, write_point_cloud_ply
    from gs_io.ply import colors_to_uint8

    rng = np.random.default_rng(1)
    pts = rng.standard_normal((1001, 3)).astype(np.float32)
    nrm = rng.standard_normal((1001, 3)).astype(np.float32)
    col = rng.uniform(-0.1, 1.1, (1001, 3)).astype(np.float32)
    col[:4] = [[0, 0.5, 1], [0.5 / 255 - 1e-4, 0.5 / 255 + 1e-4, 254.6 / 255], [1.5, -2, 0.25], [0.999, 0.001, 0.5]]
    want8 = np.rint(np.clip(col, 0, 1) * np.float32(255)).astype(np.uint8)
    assert np.array_equal(colors_to_uint8(col), want8) and tuple(want8[1]) == (0, 1, 255) and tuple(want8[2]) == (255, 0, 64)
    f = str(tmp_path / "point_cloud.ply")
    write_point_cloud_ply(f, pts, col, nrm)
    head = open(f, "rb").read(400)
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 1001\nproperty float x\n")
    assert b"property float nx\n" in head and b"property uchar red\n" in head
    back = read_point_cloud_ply(f)
    assert np.array_equal(back["points"], pts) and np.array_equal(back["normals"], nrm)
    assert back["colors"].dtype == np.uint8 and np.array_equal(back["colors"], want8)
    write_point_cloud_ply(f, pts, col)  # without normals
    back = read_point_cloud_ply(f)
    assert back["normals"] is None and np.array_equal(back["points"], pts) and np.array_equal(back["colors"], want8)

    tri = rng.integers(0, 1001, (777, 3)).astype(np.int32)
    g = str(tmp_path / "mesh.ply")
    write_mesh_ply(g, pts, tri, col)
    assert b"element face 777\nproperty list uchar int vertex_indices\n" in open(g, "rb").read(400)
    m = read_mesh_ply(g)
    assert np.array_equal(m["vertices"], pts) and m["triangles"].dtype == np.int32 and np.array_equal(m["triangles"], tri)
    assert np.array_equal(m["vertex_colors"], want8)
    write_mesh_ply(g, pts, tri)
    m = read_mesh_ply(g)
    assert m["vertex_colors"] is None and np.array_equal(m["triangles"], tri)
    write_mesh_ply(g, pts[:0], tri[:0], col[:0])  # an empty mesh is a valid file
    m = read_mesh_ply(g)
    assert m["vertices"].shape == (0, 3) and m["triangles"].shape == (0, 3)
    with pytest.raises(ValueError):
        write_mesh_ply(g, pts[:10], tri)


# ---- the oracle against the sphere it fuses --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere():
    vol = R.RefVolume(**R.sphere_volume_args())
    infos = R.fuse_sphere(vol)
    return vol, infos


def test_sphere_scene_is_what_the_tests_assume():
    cams = R.sphere_cameras()
    assert len(cams) == 14
    for V in cams:
        assert abs(np.linalg.norm(np.linalg.inv(V.astype(np.float64))[:3, 3]) - 1.5) < 1e-6
        d, c, m = R.sphere_view(V)
        assert d.shape == (160, 160) and c.shape == (160, 160, 3) and m.dtype == np.uint8
        assert 0.2 < m.mean() < 0.6 and (d[m > 0] > 0.99).all() and (d[m > 0] < 1.5).all() and (d[d == 0].size > 0)


def test_oracle_points_and_vertices_lie_on_the_sphere(sphere):
    vol, _ = sphere
    L = R.SPHERE_L
    p, c, n, a = vol.extract_point_cloud()
    assert len(p) > 10000 and a.min() == 0 and a.max() == 2
    worst = np.abs(np.linalg.norm(p.astype(np.float64), axis=1) - R.SPHERE_RADIUS).max()
    print(f"points: {len(p)}, worst distance {worst / L:.3f} L")
    assert worst < L
    radial = p / np.linalg.norm(p, axis=1, keepdims=True)
    assert ((n * radial).sum(1) > 0.9).all()  # normals towards free space
    assert np.abs(c - (0.5 + 0.5 * radial)).max() < 0.05
    v, vc, t = vol.extract_mesh()
    worst_v = np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - R.SPHERE_RADIUS).max()
    print(f"mesh: {len(v)} vertices, {len(t)} triangles, worst distance {worst_v / L:.3f} L")
    assert worst_v < L


def test_oracle_mesh_is_a_closed_oriented_manifold(sphere):
    vol, _ = sphere
    v, vc, t = vol.extract_mesh()
    rep = R.mesh_report(v, t)
    true_volume = 4.0 / 3.0 * math.pi * R.SPHERE_RADIUS ** 3
    print(rep, "relative volume error", rep["volume"] / true_volume - 1)
    assert rep["closed"] and rep["oriented"] and rep["euler"] == 2 and rep["used_vertices"] == len(v)
    assert rep["volume"] > 0 and abs(rep["volume"] / true_volume - 1) < 0.01


def test_oracle_ambiguous_share_is_small(sphere):
    _, infos = sphere
    updated = sum(int(i["updated"].sum()) for i in infos)
    flagged = sum(int((i["ambig"] & i["updated"]).sum()) for i in infos)
    visited_flagged = sum(int(i["ambig"].sum()) for i in infos)
    print(f"updated {updated}, flagged updates {flagged} ({flagged / updated:.2e}), flagged visits {visited_flagged}")
    assert updated > 300000 and flagged <= 1e-3 * updated


def test_oracle_touch_covers_the_truncation_band():
    """Step 1 opens every block that holds a voxel within sdf_trunc of the observed surface (single view)."""
    fx, fy, cx, cy = R.sphere_intrinsics()
    V = R.sphere_cameras()[6]
    d, c, m = R.sphere_view(V)
    vol = R.RefVolume(**R.sphere_volume_args())
    info = vol.integrate(d, c, fx, fy, cx, cy, V, valid=m)
    sdf = R.dense_view_sdf(R.sphere_volume_args(), d, c, fx, fy, cx, cy, V, valid=m)
    band_blocks = np.nonzero((np.abs(sdf) < vol.trunc).any(1))[0]
    assert len(band_blocks) > 20 and np.isin(band_blocks, info["flagged"]).all()


def test_oracle_capacity_overflow(sphere):
    full, _ = sphere
    vol = R.RefVolume(**R.sphere_volume_args(capacity=200))
    R.fuse_sphere(vol)
    assert vol.overflow and vol.num_allocated == 200 and vol.needed > 200 and (vol.table < 200).all()
    with pytest.raises(RuntimeError, match="200 blocks allocated"):
        vol.extract_point_cloud()
    # the first view fits: its blocks hold the same slots in both volumes
    one = R.RefVolume(**R.sphere_volume_args())
    R.fuse_sphere(one, 1)
    assert one.num_allocated < 200
    held = one.table >= 0
    assert np.array_equal(vol.table[held], one.table[held]) and np.array_equal(full.table[held], one.table[held])


# ---- the noise scene: what the GPU tests assume of it ----------------------------------------------------------------
GRID = 2048  # workgroups of the kernels that loop over blocks (csrc/tsdf.hip)


@pytest.fixture(scope="module")
def noise():
    vol = R.RefVolume(**R.noise_volume_args())
    return vol, R.fuse_views(vol, R.noise_views())


def test_noise_scene_covers_the_second_round_of_the_block_loops(noise):
    vol, infos = noise
    lists = [len(i["blocks"]) for i in infos]
    updated = sum(int(i["updated"].sum()) for i in infos)
    flagged = sum(int((i["ambig"] & i["updated"]).sum()) for i in infos)
    print(f"noise: {int(np.prod(vol.blocks))} blocks, lists {lists}, {vol.num_allocated} allocated, {updated} updates, "
          f"ambiguous share {flagged / updated:.2e}")
    assert int(np.prod(vol.blocks)) > GRID and vol.num_allocated > GRID and not vol.overflow
    assert sum(n > GRID for n in lists) >= 3
    assert flagged <= 5e-3 * updated  # a cap on what the comparisons leave out, not a tolerance
    # the cameras: one inside the volume, one outside it, and voxels behind each of them
    lo = np.asarray(R.NOISE_ORIGIN)
    hi = lo + 8 * R.NOISE_L * np.asarray(R.NOISE_BLOCKS)
    pos = [np.linalg.inv(V.astype(np.float64))[:3, 3] for V in R.noise_cameras()]
    inside = [bool(((p > lo) & (p < hi)).all()) for p in pos]
    assert sum(inside) == 4 and not inside[4]
    corners = np.array([[x, y, z, 1.0] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    assert all(((V.astype(np.float64) @ corners.T)[2] < 0).any() for V in R.noise_cameras()[:4])
    fx, fy, _, _ = R.noise_intrinsics()
    assert abs(fy / fx - 1.07) < 1e-6


def test_noise_scene_overflows_past_slot_2048(noise):
    full, _ = noise
    cap = R.NOISE_OVERFLOW_CAPACITY
    vol = R.RefVolume(**R.noise_volume_args(cap))
    infos = R.fuse_views(vol, R.noise_views())
    first = infos[0]
    print(f"capacity {cap}: first view flags {len(first['flagged'])}, integrates {len(first['blocks'])}; "
          f"allocated {vol.num_allocated}, needed {vol.needed}")
    assert cap > GRID and vol.overflow and vol.num_allocated == cap and vol.needed > cap
    # the first view alone fills the pool: slots past 2048 are handed out and a suffix of its blocks is dropped
    assert len(first["flagged"]) > cap and len(first["blocks"]) == cap and first["slots"].max() == cap - 1
    assert np.array_equal(first["blocks"], first["flagged"][:cap])
    held = vol.table >= 0
    assert np.array_equal(vol.table[held], full.table[held])  # (ascending block order in both)
    with pytest.raises(RuntimeError, match=rf"{cap} blocks allocated, {vol.needed} needed"):
        vol.extract_mesh()


def test_poisoned_depth_is_unusable_and_raises_no_warning():
    """NaN, +inf, negative and beyond-depth_trunc pixels with `valid` set: the oracle gives what it gives with those
    pixels at depth 0, and its NumPy code stays silent with warnings turned into errors."""
    views = R.noise_views(poison=True, masked=True)[:2]
    clean = []
    for v in views:
        d = v["depth"]
        bad = ~(np.isfinite(d) & (d > 0) & (d <= np.float32(R.NOISE_DEPTH_TRUNC)))
        assert bad.mean() > 0.055 and np.isnan(d).sum() > 100 and np.isposinf(d).sum() > 100 and (d < 0).sum() > 100
        assert (d > R.NOISE_DEPTH_TRUNC).sum() > 2000 and (v["valid"][~np.isfinite(d) | (d < 0)] == 1).all()
        clean.append({**v, "depth": np.where(bad, np.float32(0), d)})
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        a = R.RefVolume(**R.noise_volume_args())
        R.fuse_views(a, views)
        R.fuse_views(a, [{**views[0], "valid": None}])
        R.dense_fusion_f64(R.noise_volume_args(), views[:1])
    b = R.RefVolume(**R.noise_volume_args())
    R.fuse_views(b, clean)
    R.fuse_views(b, [{**clean[0], "valid": None}])
    assert a.num_allocated == b.num_allocated > GRID and np.array_equal(a.table, b.table)
    for k in ("tsdf", "weight", "color"):
        assert np.isfinite(getattr(a, k)).all() and np.array_equal(getattr(a, k), getattr(b, k)), k


# ---- the rule in float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["sphere", "room", "noise"])
def test_oracle_against_the_float64_rule(scene, sphere, noise):
    """The float32 oracle against `dense_fusion_f64` (which knows no blocks): equal weights on every stable voxel,
    and every in-band update of every view inside a block that view lists."""
    args, views, lists = R.f64_case(scene)
    vol, infos = {"sphere": sphere, "noise": noise}.get(scene) or R.fused_oracle(scene)
    dense = R.dense_fusion_f64(args, views, lists(infos))
    rep = R.f64_distance(vol.table, vol.tsdf, vol.weight, vol.color, dense, f"{scene}: oracle")
    assert rep["unstable_share"] <= 0.01
    assert (dense["weight"] > 0)[rep["stable"]].sum() > 100000
    assert rep["weight_mismatches"] == 0 and rep["uncovered"] == 0
    assert R.band_uncovered(dense, [i["blocks"] for i in infos]) == [0] * len(views)
    # the sdf carries a few roundings of numbers up to the depth range (ulp(3.2) = 2.4e-7, times the ray factor <= 2)
    # and is divided by sdf_trunc = 1/16 or 1/8: some 1e-5 at worst.  1e-4 separates that from a wrong rule.
    assert rep["d_tsdf"] < 1e-4 and rep["d_color"] < 1e-4


# ---- random volumes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.RANDOM_KINDS)
@pytest.mark.parametrize("blocks", R.RANDOM_SHAPES, ids=lambda b: "x".join(map(str, b)))
def test_oracle_extraction_of_random_volumes(blocks, kind):
    sd = R.random_state(blocks, kind)
    nb = int(np.prod(blocks))
    table = sd["table"].reshape(-1)
    held = np.nonzero(table >= 0)[0]
    n = sd["num_allocated"]
    assert len(held) == n == max(1, round(R.random_fill(blocks) * nb)) and sd["capacity"] > n
    assert np.array_equal(np.sort(table[held]), np.arange(n))
    if n > 1:
        assert not np.array_equal(table[held], np.arange(n))  # slot order is not block order
    f, w = sd["tsdf"][:n], sd["weight"][:n]
    assert 0.08 < (w == 0).mean() < 0.12
    if nb > 1:
        for value in R.PLANTED:
            same = (f == value) & (np.signbit(f) == np.signbit(value))
            assert same.sum() > 200, value
        for a, B in enumerate(blocks):  # blocks on both faces of the volume along every axis
            idx = (held // int(np.prod(blocks[:a]))) % B
            assert idx.min() == 0 and idx.max() == B - 1
    vol = R.ref_from_state(sd)
    p, c, nrm, axis = vol.extract_point_cloud()
    v, vc, t = vol.extract_mesh()
    rep = R.mesh_report(v, t)
    print(f"{blocks} {kind}: {n} blocks, {len(p)} points, {len(v)} vertices, {len(t)} triangles, "
          f"oriented {rep['oriented']}")
    few = nb == 1
    assert len(p) > (20 if few else 10000) and len(v) > (20 if few else 10000) and len(t) > (10 if few else 5000)
    assert t.min() >= 0 and t.max() < len(v) and np.isfinite(p).all() and np.isfinite(v).all()
    assert np.isfinite(nrm).all() and np.isfinite(c).all() and np.isfinite(vc).all()
    if kind == "smooth":
        assert rep["oriented"]
