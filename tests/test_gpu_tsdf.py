"""GPU: TSDF fusion (gs_fusion, csrc/tsdf.hip) against the float32 NumPy oracle of tests/tsdf_reference.py.

The oracle performs the kernels' operations in the kernels' order, so integration is compared exactly (weights) and to
1e-6 (tsdf in [-1, 1], colours in [0, 1]: a few fp32 roundings with a 10x margin) on every voxel the oracle does not
flag ambiguous; the tests print how many values were bit-equal.  Extraction is compared on the ORACLE's volume (loaded
with `load_state_dict`), so no decision depends on the last bit of integration.

The noise scene (3072 blocks, per-view lists of up to 2974 blocks, 3065 allocated) sends every kernel that loops over
blocks with 2048 workgroups round a second time; `dense_fusion_f64` checks the kernel against the rule in plain float64,
within twice the float32 oracle's own distance from it; the random volumes of `tsdf_reference.random_volume_state`
(slot order unrelated to block order, weight holes, exact 0.0 / -0.0 / +-0.98, blocks on every face of the volume,
one-block-thick volumes) are extracted exactly as the oracle extracts them.

End-to-end scene: 20 000 flat (0.02 x 0.02 x 0.002), opaque Gaussians on the radius-0.5 sphere, 14 cameras.  Extracted
points must lie within sdf_trunc + 3 * max scale = 0.1225 of the sphere (the TSDF has crossings only within the
truncation band of observed depths, and observed depths are alpha-weighted means of splat depths);
`test_end_to_end_render_and_fuse` prints the measured worst distance (0.0219 on the first hardware run).
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tsdf_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _NumpyViews:
    """`integrate` of a gs_fusion.TSDFVolume taking the oracle's numpy arrays."""

    def __init__(self, vol):
        self.vol = vol

    def integrate(self, d, c, fx, fy, cx, cy, V, valid=None, depth_trunc=10.0):
        self.vol.integrate(_t(d), _t(c), fx, fy, cx, cy, V, valid=None if valid is None else _t(valid),
                           depth_trunc=depth_trunc)


def _gpu_volume(args):
    from gs_fusion import TSDFVolume

    return TSDFVolume(device=DEV, **args)


def _compare_volumes(gv, ref, infos, what):
    sd = gv.state_dict()
    n = ref.num_allocated
    assert sd["num_allocated"] == n and sd["overflow"] == ref.overflow and sd["needed"] == ref.needed
    assert np.array_equal(sd["table"].cpu().numpy(), ref.table), f"{what}: slot assignment differs"
    ambig = np.zeros((ref.capacity, 512), bool)
    for i in infos:
        ambig[i["slots"]] |= i["ambig"]
    ok = ~ambig[:n]
    w, t, c = (sd[k].cpu().numpy()[:n] for k in ("weight", "tsdf", "color"))
    rw, rt, rc = ref.weight[:n], ref.tsdf[:n], ref.color[:n]
    dt, dc = np.abs(t - rt)[ok], np.abs(c - rc)[ok]
    print(f"{what}: {n} blocks, {int(ok.sum())} voxels compared ({int((~ok).sum())} ambiguous); bit-equal weight "
          f"{int((w == rw)[ok].sum())}, tsdf {int((t == rt)[ok].sum())}, colour values {int((c == rc)[ok].sum())} of "
          f"{3 * int(ok.sum())}; max |d tsdf| {dt.max():.2e}, max |d colour| {dc.max():.2e}")
    assert np.array_equal(w[ok], rw[ok]), f"{what}: weights differ"
    assert dt.max() <= 1e-6 and dc.max() <= 1e-6
    assert (rw > 0).sum() > 1000
    return sd


@pytest.fixture(scope="module")
def sphere_ref():
    ref = R.RefVolume(**R.sphere_volume_args())
    return ref, R.fuse_sphere(ref)


@pytest.fixture(scope="module")
def sphere_gpu():
    gv = _gpu_volume(R.sphere_volume_args())
    R.fuse_sphere(_NumpyViews(gv))
    return gv


# ---- integration -----------------------------------------------------------------------------------------------------
def test_integration_parity_sphere(sphere_ref, sphere_gpu):
    ref, infos = sphere_ref
    _compare_volumes(sphere_gpu, ref, infos, "sphere")
    assert sphere_gpu.num_allocated_blocks == ref.num_allocated


def test_integration_parity_room():
    ref = R.RefVolume(**R.room_volume_args())
    infos = R.fuse_room(ref)
    gv = _gpu_volume(R.room_volume_args())
    R.fuse_room(_NumpyViews(gv))
    _compare_volumes(gv, ref, infos, "room")


def test_single_view_detail():
    fx, fy, cx, cy = R.sphere_intrinsics()
    V = R.sphere_cameras()[6]
    d, c, m = R.sphere_view(V)
    ref = R.RefVolume(**R.sphere_volume_args())
    info = ref.integrate(d, c, fx, fy, cx, cy, V, valid=m)
    gv = _gpu_volume(R.sphere_volume_args())
    _NumpyViews(gv).integrate(d, c, fx, fy, cx, cy, V, valid=m)
    sd = gv.state_dict()
    table = sd["table"].cpu().numpy().reshape(-1)
    weight = sd["weight"].cpu().numpy()
    # only flagged blocks hold anything
    assert np.array_equal(np.nonzero(table >= 0)[0], info["flagged"])
    assert sd["num_allocated"] == len(info["flagged"]) and (weight[sd["num_allocated"]:] == 0).all()
    assert np.isin(weight, (0.0, 1.0)).all()
    # every voxel of the WHOLE volume within the truncation band of this view was observed once
    sdf = R.dense_view_sdf(R.sphere_volume_args(), d, c, fx, fy, cx, cy, V, valid=m)
    bb, vv = np.nonzero(np.abs(sdf) < ref.trunc)
    assert len(bb) > 5000 and (table[bb] >= 0).all()
    assert (weight[table[bb], vv] == 1.0).all()


def test_valid_none_all_invalid_and_streams():
    fx, fy, cx, cy = R.sphere_intrinsics()
    cams = R.sphere_cameras()
    args = R.sphere_volume_args()
    # all-invalid view: a no-op that allocates nothing
    gv = _gpu_volume(args)
    d, c, m = R.sphere_view(cams[0])
    _NumpyViews(gv).integrate(d, c, fx, fy, cx, cy, cams[0], valid=np.zeros_like(m))
    assert gv.num_allocated_blocks == 0 and bool((gv.table == -1).all())
    p, _, _ = gv.extract_point_cloud()
    v, _, t = gv.extract_mesh()
    assert p.shape == (0, 3) and v.shape == (0, 3) and t.shape == (0, 3)
    # valid=None: the depth alone decides (background depth is 0, grazing pixels now count)
    ref = R.RefVolume(**args)
    infos = [ref.integrate(*R.sphere_view(V)[:2], fx, fy, cx, cy, V, valid=None) for V in cams[:3]]
    for V in cams[:3]:
        d, c, _ = R.sphere_view(V)
        _NumpyViews(gv).integrate(d, c, fx, fy, cx, cy, V, valid=None)
    want = _compare_volumes(gv, ref, infos, "valid=None")
    # the same on a non-default stream
    gs = _gpu_volume(args)
    views = [tuple(_t(a) for a in R.sphere_view(V)[:2]) for V in cams[:3]]
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        for V, (d, c) in zip(cams[:3], views):
            gs.integrate(d, c, fx, fy, cx, cy, V)
    s.synchronize()
    got = gs.state_dict()
    for k in ("table", "tsdf", "weight", "color"):
        assert torch.equal(got[k], want[k]), k


def test_nan_prefilled_pool(sphere_gpu):
    """Blocks are initialised when their slot is handed out, not at construction."""
    gv = _gpu_volume(R.sphere_volume_args())
    for t in (gv.tsdf, gv.weight, gv.color):
        t.fill_(float("nan"))
    R.fuse_sphere(_NumpyViews(gv))
    got, want = gv.state_dict(), sphere_gpu.state_dict()
    assert got["num_allocated"] == want["num_allocated"] > 0
    for k in ("table", "tsdf", "weight", "color"):
        assert torch.equal(got[k], want[k]), k


def test_capacity_overflow():
    args = R.sphere_volume_args(capacity=200)
    ref = R.RefVolume(**args)
    infos = R.fuse_sphere(ref)
    assert ref.overflow
    gv = _gpu_volume(args)
    R.fuse_sphere(_NumpyViews(gv))  # integrate itself does not raise
    _compare_volumes(gv, ref, infos, "capacity 200")
    for fn in (gv.extract_point_cloud, gv.extract_mesh):
        with pytest.raises(RuntimeError, match=rf"200 blocks allocated, {ref.needed} needed"):
            fn()


# ---- more than 2048 blocks: the noise scene --------------------------------------------------------------------------
def _fused_gpu(args, views):
    gv = _gpu_volume(args)
    R.fuse_views(_NumpyViews(gv), views)
    return gv


@pytest.fixture(scope="module")
def noise_gpu():
    return _fused_gpu(R.noise_volume_args(), R.noise_views())


def test_noise_scene_parity(noise_gpu):
    ref, infos = R.fused_oracle("noise")
    assert min(ref.num_allocated, int(np.prod(ref.blocks))) > 2048 and sum(len(i["blocks"]) > 2048 for i in infos) >= 3
    _compare_volumes(noise_gpu, ref, infos, "noise")


def test_noise_scene_overflow():
    cap = R.NOISE_OVERFLOW_CAPACITY
    ref, infos = R.fused_oracle("noise", capacity=cap)
    assert ref.overflow and len(infos[0]["flagged"]) > cap > 2048  # the dropped suffix lies past slot 2048
    gv = _fused_gpu(R.noise_volume_args(cap), R.noise_views())
    sd = _compare_volumes(gv, ref, infos, f"noise, capacity {cap}")
    assert sd["overflow"] and sd["needed"] == ref.needed and sd["num_allocated"] == cap
    for fn in (gv.extract_point_cloud, gv.extract_mesh):
        with pytest.raises(RuntimeError, match=rf"{cap} blocks allocated, {ref.needed} needed"):
            fn()


@pytest.mark.parametrize("masked", [False, True], ids=["valid=None", "valid=mask"])
def test_poisoned_depth(masked):
    """NaN, +inf, negative and beyond-depth_trunc depths (with `valid` set) are unusable pixels, nothing more."""
    ref, infos = R.fused_oracle("noise", poison=True, masked=masked)
    gv = _fused_gpu(R.noise_volume_args(), R.noise_views(poison=True, masked=masked))
    sd = _compare_volumes(gv, ref, infos, f"poisoned depth, masked={masked}")
    n = sd["num_allocated"]
    for k in ("tsdf", "weight", "color"):
        assert bool(torch.isfinite(sd[k][:n]).all()), k


@pytest.mark.parametrize("scene", ["sphere", "room", "noise"])
def test_kernel_against_the_float64_rule(scene, sphere_gpu, noise_gpu):
    """The fused volume against the rule in plain float64 over every voxel (`dense_fusion_f64`, which shares no code
    with the oracle's integrate): equal weights on stable voxels; tsdf and colour within twice the float32 oracle's own
    largest distance from float64 on the same scene, recomputed here (the factor 2 allows the kernel a different
    rounding on the worst element)."""
    args, views, lists = R.f64_case(scene)
    ref, infos = R.fused_oracle(scene)
    dense = R.dense_fusion_f64(args, views, lists(infos))
    own = R.f64_distance(ref.table, ref.tsdf, ref.weight, ref.color, dense, f"{scene}: oracle")
    gv = {"sphere": sphere_gpu, "noise": noise_gpu}.get(scene) or _fused_gpu(args, views)
    sd = gv.state_dict()
    got = R.f64_distance(sd["table"].cpu().numpy(), *(sd[k].cpu().numpy() for k in ("tsdf", "weight", "color")), dense,
                         f"{scene}: kernel")
    assert own["weight_mismatches"] == 0 and 0 < own["d_tsdf"] < 1e-4 and 0 < own["d_color"] < 1e-4
    assert got["weight_mismatches"] == 0 and got["uncovered"] == 0
    assert got["d_tsdf"] <= 2 * own["d_tsdf"] and got["d_color"] <= 2 * own["d_color"]


def test_resume_from_a_state_dict(noise_gpu):
    """`state_dict` holds enough to resume: two views, a round trip into a fresh volume whose pool holds NaN, three
    more views -- the same bits as the uninterrupted fusion."""
    views = R.noise_views()
    first = _fused_gpu(R.noise_volume_args(), views[:2])
    sd = first.state_dict()
    assert 2048 < sd["num_allocated"] < noise_gpu.num_allocated_blocks  # the later views still open blocks
    gv = _gpu_volume(R.noise_volume_args())
    for t in (gv.tsdf, gv.weight, gv.color):
        t.fill_(float("nan"))
    gv.load_state_dict(sd)
    del first
    R.fuse_views(_NumpyViews(gv), views[2:])
    got, want = gv.state_dict(), noise_gpu.state_dict()
    assert (got["num_allocated"], got["overflow"], got["needed"]) == (want["num_allocated"], False, want["needed"])
    for k in ("table", "tsdf", "weight", "color"):
        assert torch.equal(got[k], want[k]), k


def test_forms_of_the_arguments():
    """[3,4] and CUDA view matrices, [H,W,1] depth, bool and 0 / 255 uint8 masks: the same bits as the plain call."""
    views = R.sphere_views(2)
    args = R.sphere_volume_args()

    def fuse(change):
        gv = _gpu_volume(args)
        for v in views:
            kw = dict(depth=_t(v["depth"]), color=_t(v["color"]), viewmat=v["viewmat"], valid=_t(v["valid"]))
            change(kw)
            gv.integrate(kw["depth"], kw["color"], v["fx"], v["fy"], v["cx"], v["cy"], kw["viewmat"],
                         valid=kw["valid"], depth_trunc=v["depth_trunc"])
        return gv.state_dict()

    want = fuse(lambda kw: None)
    assert want["num_allocated"] > 100 and views[0]["valid"].dtype == np.uint8
    forms = {"viewmat [3,4]": lambda kw: kw.update(viewmat=kw["viewmat"][:3]),
             "viewmat on the device": lambda kw: kw.update(viewmat=_t(kw["viewmat"])),
             "viewmat [3,4] on the device": lambda kw: kw.update(viewmat=_t(kw["viewmat"][:3])),
             "depth [H,W,1]": lambda kw: kw.update(depth=kw["depth"][..., None].contiguous()),
             "valid bool": lambda kw: kw.update(valid=kw["valid"].bool()),
             "valid 0 / 255": lambda kw: kw.update(valid=kw["valid"] * 255)}
    for name, change in forms.items():
        got = fuse(change)
        assert got["num_allocated"] == want["num_allocated"], name
        for k in ("table", "tsdf", "weight", "color"):
            assert torch.equal(got[k], want[k]), (name, k)


# ---- extraction ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.RANDOM_KINDS)
@pytest.mark.parametrize("blocks", R.RANDOM_SHAPES, ids=lambda b: "x".join(map(str, b)))
def test_extraction_of_random_volumes(blocks, kind):
    """Extraction makes discrete decisions on given floats: on a loaded volume every count, axis and triangle is the
    oracle's, whatever the field."""
    sd = R.random_state(blocks, kind)
    ref = R.ref_from_state(sd)
    gv = _gpu_volume(dict(voxel_length=sd["voxel_length"], sdf_trunc=sd["sdf_trunc"], origin=sd["origin"],
                          blocks=sd["blocks"], capacity=sd["capacity"]))
    gv.load_state_dict(sd)
    what = f"{'x'.join(map(str, blocks))} {kind}"
    p, c, n, a = (x.cpu().numpy() for x in gv.extract_point_cloud(return_axis=True))
    rp, rc, rn, ra = ref.extract_point_cloud()
    assert p.shape == rp.shape and len(rp) > 20
    assert np.array_equal(a, ra)
    print(f"{what}: {len(p)} points, max |d| position {np.abs(p - rp).max():.2e}, colour {np.abs(c - rc).max():.2e}, "
          f"normal {np.abs(n - rn).max():.2e}; bit-equal positions {int((p == rp).sum())} of {p.size}, normals "
          f"{int((n == rn).sum())} of {n.size}")
    assert np.abs(p - rp).max() <= 1e-5 and np.abs(c - rc).max() <= 1e-5 and np.abs(n - rn).max() <= 1e-4
    v, vc, t = (x.cpu().numpy() for x in gv.extract_mesh())
    rv, rvc, rt = ref.extract_mesh()
    assert v.shape == rv.shape and t.shape == rt.shape and t.dtype == np.int32 and len(rt) > 10
    assert np.array_equal(t, rt)
    print(f"{what}: {len(v)} vertices, {len(t)} triangles, max |d| position {np.abs(v - rv).max():.2e}, "
          f"colour {np.abs(vc - rvc).max():.2e}; bit-equal positions {int((v == rv).sum())} of {v.size}")
    assert np.abs(v - rv).max() <= 1e-5 and np.abs(vc - rvc).max() <= 1e-5
    p2, c2, n2, a2 = gv.extract_point_cloud(return_axis=True)
    v2, vc2, t2 = gv.extract_mesh()
    for x, y in ((p2, p), (c2, c), (n2, n), (a2, a), (v2, v), (vc2, vc), (t2, t)):
        assert np.array_equal(x.cpu().numpy(), y)
    if kind == "smooth":
        assert R.mesh_report(v, t)["oriented"]


@pytest.mark.parametrize("scene", ["sphere", "room"])
def test_extraction_parity(scene, sphere_ref):
    if scene == "sphere":
        ref, _ = sphere_ref
        args = R.sphere_volume_args()
    else:
        args = R.room_volume_args()
        ref = R.RefVolume(**args)
        R.fuse_room(ref)
    gv = _gpu_volume(args)
    gv.load_state_dict(ref.state_dict())
    p, c, n, a = (x.cpu().numpy() for x in gv.extract_point_cloud(return_axis=True))
    rp, rc, rn, ra = ref.extract_point_cloud()
    assert p.shape == rp.shape and len(rp) > 10000
    assert np.array_equal(a, ra)
    print(f"{scene}: {len(p)} points, max |d| position {np.abs(p - rp).max():.2e}, colour {np.abs(c - rc).max():.2e}, "
          f"normal {np.abs(n - rn).max():.2e}")
    assert np.abs(p - rp).max() <= 1e-5 and np.abs(c - rc).max() <= 1e-5 and np.abs(n - rn).max() <= 1e-4
    v, vc, t = (x.cpu().numpy() for x in gv.extract_mesh())
    rv, rvc, rt = ref.extract_mesh()
    assert v.shape == rv.shape and t.shape == rt.shape and t.dtype == np.int32 and len(rt) > 10000
    assert np.array_equal(t, rt)
    print(f"{scene}: {len(v)} vertices, {len(t)} triangles, max |d| position {np.abs(v - rv).max():.2e}, "
          f"colour {np.abs(vc - rvc).max():.2e}")
    assert np.abs(v - rv).max() <= 1e-5 and np.abs(vc - rvc).max() <= 1e-5
    # extraction reads the volume only: a second call gives the same arrays
    v2, _, t2 = gv.extract_mesh()
    assert np.array_equal(v2.cpu().numpy(), v) and np.array_equal(t2.cpu().numpy(), t)


def test_mesh_quality_of_the_fused_sphere(sphere_gpu):
    L = R.SPHERE_L
    p, c, n = (x.cpu().numpy() for x in sphere_gpu.extract_point_cloud())
    v, vc, t = (x.cpu().numpy() for x in sphere_gpu.extract_mesh())
    wp = np.abs(np.linalg.norm(p.astype(np.float64), axis=1) - R.SPHERE_RADIUS).max()
    wv = np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - R.SPHERE_RADIUS).max()
    rep = R.mesh_report(v, t)
    print(f"{len(p)} points worst {wp / L:.3f} L; {len(v)} vertices worst {wv / L:.3f} L; {rep}")
    assert len(p) > 10000 and wp < L and wv < L
    assert rep["closed"] and rep["oriented"] and rep["euler"] == 2 and rep["used_vertices"] == len(v)
    assert rep["volume"] > 0 and abs(rep["volume"] / (4.0 / 3.0 * math.pi * R.SPHERE_RADIUS ** 3) - 1) < 0.01
    radial = p / np.linalg.norm(p, axis=1, keepdims=True)
    assert ((n * radial).sum(1) > 0.9).all()


# ---- end to end ------------------------------------------------------------------------------------------------------
MAX_SCALE = 0.02


def _sphere_gaussians(n=20000, seed=11):
    """Raw (pre-activation) parameters, as a Gaussian PLY holds them: flat opaque discs tangent to the sphere."""
    from harness.scene import SH_C0

    rng = np.random.default_rng(seed)
    nrm = rng.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = nrm[nrm[:, 2] > -0.999]
    n = len(nrm)
    q = np.concatenate([1.0 + nrm[:, 2:3], -nrm[:, 1:2], nrm[:, 0:1], np.zeros((n, 1))], 1)  # z axis -> normal
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    f32 = np.float32
    return {"means": (R.SPHERE_RADIUS * nrm).astype(f32),
            "scales": np.log(np.tile([MAX_SCALE, MAX_SCALE, 0.002], (n, 1))).astype(f32),
            "quats": (q * 1.7).astype(f32), "opacities": np.full((n, 1), 6.0, f32),  # sigmoid(6) = 0.9975
            "features_dc": ((0.5 + 0.5 * nrm - 0.5) / SH_C0).astype(f32),
            "features_rest": np.zeros((n, 0, 3), f32)}


def _write_poses(path):
    fx, fy, cx, cy = R.sphere_intrinsics()
    cam = {"width": R.SPHERE_SIZE, "height": R.SPHERE_SIZE, "fx": fx, "fy": fy, "cx": cx, "cy": cy}
    entries = [{"pose": np.linalg.inv(V.astype(np.float64)).tolist(), "camera": cam} for V in R.sphere_cameras()]
    with open(path, "w") as f:
        json.dump(entries, f)


def test_end_to_end_render_and_fuse(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from export_tsdf import activated

    from gs_fusion import fuse_views, read_poses_json, view_depth
    from gs_io import read_mesh_ply, read_point_cloud_ply, write_gaussian_ply
    from harness.pipeline import CameraTensors, render_view

    raw = _sphere_gaussians()
    poses = str(tmp_path / "poses.json")
    _write_poses(poses)
    cams = read_poses_json(poses)
    assert len(cams) == 14
    params = activated(raw, torch.device(DEV))
    bg = torch.zeros(3, device=DEV)
    args = R.sphere_volume_args()
    va = _gpu_volume(args)
    fuse_views(va, params, cams, bg, 0, alpha_min=0.5, depth_trunc=10.0)
    # the same by hand
    vb = _gpu_volume(args)
    with torch.no_grad():
        for cam in cams:
            out = render_view(params["means3d"], params["scales"], params["quats"], params["opacities"],
                              params["sh_coeffs"], CameraTensors.from_numpy(cam, DEV), bg, 0, render_depth=True,
                              fused_depth=True, normalise_depth=False)
            alpha = out["alpha"][..., 0]
            valid = alpha >= 0.5
            depth = torch.where(valid, out["depth_acc"][..., 0] / alpha, torch.zeros_like(alpha))
            d2, v2 = view_depth(out["depth_acc"], out["alpha"], 0.5)
            assert torch.equal(d2, depth) and torch.equal(v2.bool(), valid) and int(valid.sum()) > 3000
            vb.integrate(depth.contiguous(), out["rgb"].contiguous(), cam.fx, cam.fy, cam.cx, cam.cy, cam.viewmat,
                         valid=valid, depth_trunc=10.0)
    a, b = va.state_dict(), vb.state_dict()
    assert a["num_allocated"] == b["num_allocated"] > 100
    for k in ("table", "tsdf", "weight", "color"):
        assert torch.equal(a[k], b[k]), k
    p, c, n = (x.cpu().numpy() for x in va.extract_point_cloud())
    assert len(p) > 5000
    worst = np.abs(np.linalg.norm(p.astype(np.float64), axis=1) - R.SPHERE_RADIUS).max()
    print(f"end to end: {len(p)} points, worst distance from the sphere {worst:.4f} "
          f"(bound {float(va.sdf_trunc) + 3 * MAX_SCALE:.4f})")
    assert worst <= va.sdf_trunc + 3 * MAX_SCALE

    # the command-line tool on the same model, in one child process under its own time limit
    model = str(tmp_path / "model.ply")
    write_gaussian_ply(model, raw)
    out_dir = str(tmp_path / "export")
    L = args["voxel_length"]
    lo = args["origin"]
    hi = [o + 8 * L * nb for o, nb in zip(lo, args["blocks"])]
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tools", "export_tsdf.py"), "--ply", model,
           "--poses", poses, "--out", out_dir, "--voxel-length", repr(L), "--sdf-trunc", repr(4 * L), "--bounds",
           *[repr(float(x)) for x in (*lo, *hi)]]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    summary = json.loads(res.stdout.strip().splitlines()[-1])
    pc = read_point_cloud_ply(os.path.join(out_dir, "point_cloud.ply"))
    mesh = read_mesh_ply(os.path.join(out_dir, "mesh.ply"))
    assert summary["points"] == len(pc["points"]) == len(p) and np.array_equal(pc["points"], p)
    assert pc["colors"].dtype == np.uint8 and pc["normals"].shape == pc["points"].shape
    assert summary["triangles"] == len(mesh["triangles"]) > 5000 and mesh["triangles"].max() < len(mesh["vertices"])
    assert mesh["vertex_colors"].shape == mesh["vertices"].shape
