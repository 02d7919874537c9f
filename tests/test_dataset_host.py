"""Host: gs_io.dataset.load_dataset on a directory written by tools/make_synthetic_dataset.py (12 views of 48x32,
rendered through the CPU stand-ins of tests/cpu_standins.py): file order, the splits of all four eval modes and of
`*_filenames`, poses / scale / transform, global and per-frame intrinsics, the seed cloud, dtypes and values of images,
masks and depth, monocular scale and shift, every refusal -- and the pose and split arithmetic against what the
reference's own functions produced (tests/golden/dataset_poses.npz, tests/golden/make_golden_dataset.py)."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gs_io import dataset as D  # noqa: E402
from gs_io.dataset import load_dataset  # noqa: E402

VIEWS, W, H = 12, 48, 32


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """(directory, transforms.json dict, the cameras the images were rendered from) -- built once."""
    import make_synthetic_dataset as M

    import harness.train as HT

    out = str(tmp_path_factory.mktemp("dataset"))
    restore = M.use_cpu_standins()
    try:
        meta = M.make_synthetic_dataset(out, VIEWS, W, H, alpha=True, device="cpu")
    finally:
        restore()
    return out, meta, HT.orbit_cameras(VIEWS, W, H)


def _variant(made, name, edit):
    """Another transforms file next to the first (load_dataset takes the json itself), edited by `edit(meta)`."""
    out, meta, _ = made
    meta = copy.deepcopy(meta)
    edit(meta)
    path = os.path.join(out, f"{name}.json")
    with open(path, "w") as f:
        json.dump(meta, f)
    return path


def test_files_dtypes_and_values(made):
    from PIL import Image

    out, meta, _ = made
    ds = load_dataset(out, "train", eval_mode="all")
    assert len(ds) == VIEWS and (ds.width, ds.height) == (W, H)
    assert [os.path.basename(f) for f in ds.image_filenames] == [f"frame_{i:05d}.png" for i in range(VIEWS)]
    for i in (0, 5, VIEWS - 1):
        img, m, z = ds.image(i), ds.mask(i), ds.depth(i)
        assert img.dtype == np.uint8 and img.shape == (H, W, 4) and img.flags.c_contiguous
        assert np.array_equal(img, np.array(Image.open(ds.image_filenames[i])))
        assert m.dtype == np.uint8 and m.shape == (H, W) and set(np.unique(m)) <= {0, 1} and m.any() and not m.all()
        assert np.array_equal(m, (np.array(Image.open(ds.mask_filenames[i])) > 0).astype(np.uint8))
        assert z.dtype == np.uint16 and z.shape == (H, W) and z.max() > 1000  # millimetres, cameras 6 units away
        assert np.array_equal(z, np.array(Image.open(ds.depth_filenames[i])))
        assert np.array_equal(img[..., 3] > 127, m.astype(bool))  # the mask is the silhouette alpha > 0.5
    assert ds.depth_unit == 1e-3 and not ds.mono_depth
    assert ds.mono_depth_scales == [] and ds.mono_depth_shifts == []


def test_grey_image_is_replicated_and_rgb_mask_is_converted(made, tmp_path):
    from PIL import Image

    g = (np.arange(H * W) % 251).astype(np.uint8).reshape(H, W)
    Image.fromarray(g, "L").save(tmp_path / "g.png")
    img = D.read_image_u8(str(tmp_path / "g.png"))
    assert img.shape == (H, W, 3) and all(np.array_equal(img[..., c], g) for c in range(3))
    rgb = np.zeros((H, W, 3), np.uint8)
    rgb[3, 4] = (0, 9, 0)
    Image.fromarray(rgb, "RGB").save(tmp_path / "m.png")
    m = D.read_mask_u8(str(tmp_path / "m.png"))
    assert m.dtype == np.uint8 and m.sum() == 1 and m[3, 4] == 1


def test_file_order_is_by_name_whatever_the_json_order(made):
    def shuffle(meta):
        rng = np.random.default_rng(3)
        meta["frames"] = [meta["frames"][i] for i in rng.permutation(VIEWS)]

    a = load_dataset(made[0], "train", eval_mode="all", orientation_method="none", center_method="none")
    b = load_dataset(_variant(made, "shuffled", shuffle), "train", eval_mode="all", orientation_method="none",
                     center_method="none")
    assert a.image_filenames == b.image_filenames and a.depth_filenames == b.depth_filenames
    assert np.array_equal(a.camera_to_worlds, b.camera_to_worlds)


def test_splits(made):
    out = made[0]
    kw = dict(orientation_method="none", center_method="none")
    tr, ev = load_dataset(out, "train", **kw), load_dataset(out, "val", **kw)  # fraction 0.9
    assert list(tr.indices) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11] and list(ev.indices) == [10]
    assert list(load_dataset(out, "test", **kw).indices) == [10]
    tr, ev = (load_dataset(out, s, eval_mode="interval", **kw) for s in ("train", "val"))  # interval 8
    assert list(ev.indices) == [0, 8] and list(tr.indices) == [1, 2, 3, 4, 5, 6, 7, 9, 10, 11]
    tr, ev = (load_dataset(out, s, eval_mode="interval", eval_interval=3, **kw) for s in ("train", "val"))
    assert list(ev.indices) == [0, 3, 6, 9]
    tr, ev = (load_dataset(out, s, eval_mode="all", **kw) for s in ("train", "val"))
    assert list(tr.indices) == list(ev.indices) == list(range(VIEWS))
    with pytest.raises(ValueError, match="train"):  # eval_mode filename: these names hold neither word
        load_dataset(out, "train", eval_mode="filename", **kw)
    with pytest.raises(ValueError, match="eval mode"):
        load_dataset(out, "train", eval_mode="nonsense", **kw)
    with pytest.raises(ValueError, match="split"):
        load_dataset(out, "holdout", **kw)
    # every per-view list follows the split
    assert [os.path.basename(f) for f in ev.mask_filenames] == [os.path.basename(f) for f in ev.image_filenames]
    assert ev.camera_to_worlds.shape == (VIEWS, 3, 4) and len(ev.cameras) == VIEWS


def test_split_filename_mode_and_filename_lists(made, tmp_path):
    i_train, i_eval = D.split_filename(["a/train_0.png", "a/eval_0.png", "b/train_1.png"])
    assert list(i_train) == [0, 2] and list(i_eval) == [1]

    def lists(meta):
        meta["train_filenames"] = [f"images/frame_{i:05d}.png" for i in (7, 1, 4)]
        meta["val_filenames"] = ["images/frame_00002.png"]
        meta["test_filenames"] = ["images/frame_00003.png", "images/frame_00011.png"]

    p = _variant(made, "lists", lists)
    assert list(load_dataset(p, "train", eval_mode="interval").indices) == [1, 4, 7]  # the lists take precedence
    assert list(load_dataset(p, "val").indices) == [2] and list(load_dataset(p, "test").indices) == [3, 11]
    p = _variant(made, "lists_missing", lambda m: m.update(train_filenames=["images/frame_00001.png"]))
    with pytest.raises(RuntimeError, match="val"):
        load_dataset(p, "val")
    p = _variant(made, "lists_unknown", lambda m: m.update(train_filenames=["images/nope.png"]))
    with pytest.raises(RuntimeError, match="nope"):
        load_dataset(p, "train")


def test_poses_scale_transform_and_cameras(made):
    out, meta, cams = made
    written = np.array([fr["transform_matrix"] for fr in meta["frames"]], np.float32)
    raw = load_dataset(out, "train", eval_mode="all", orientation_method="none", center_method="none")
    assert raw.camera_to_worlds.dtype == np.float32 and np.array_equal(raw.camera_to_worlds, written[:, :3])
    assert raw.scale == 1.0 and np.array_equal(raw.transform, np.eye(4, dtype=np.float32)[:3])
    # the cameras are the ones the images were rendered from: viewmat, projmat and intrinsics
    for c, o in zip(raw.cameras, cams):
        assert (c.width, c.height) == (W, H)
        assert abs(c.fx - o.fx) < 1e-4 and abs(c.fy - o.fy) < 1e-4 and c.cx == o.cx and c.cy == o.cy
        assert np.abs(c.viewmat - o.viewmat).max() < 2e-6 and c.viewmat.dtype == np.float32
        assert np.abs(c.projmat - o.projmat).max() < 1e-5 and c.projmat.dtype == np.float32
    # defaults: orientation "up", centring "poses", computed over ALL frames before the split
    want, transform = D.auto_orient_and_center_poses(written, "up", "poses")
    tr = load_dataset(out, "train")
    assert np.array_equal(tr.camera_to_worlds, want.numpy()[tr.indices])
    assert np.array_equal(tr.transform, transform.numpy())
    assert float(want[:, :3, 3].mean(0).abs().max()) < 1e-5  # centred
    up = want[:, :3, 1].mean(0)
    assert float(up[2] / up.norm()) > 1 - 1e-5  # the mean up vector is +z
    # auto_scale_poses then scale_factor
    sc = load_dataset(out, "train", auto_scale_poses=True, scale_factor=0.5)
    s = 0.5 / float(want[:, :3, 3].abs().max())
    assert abs(sc.scale - s) < 1e-7
    assert np.allclose(sc.camera_to_worlds[:, :, 3], want.numpy()[sc.indices][:, :, 3] * np.float32(s), atol=1e-7)
    assert np.array_equal(sc.camera_to_worlds[:, :, :3], want.numpy()[sc.indices][:, :, :3])
    # applied_scale replaces scale_factor; orientation_override replaces the method
    ap = load_dataset(_variant(made, "applied_scale", lambda m: m.update(applied_scale=0.25)), "train", scale_factor=3.0)
    assert ap.scale == 0.25
    ov = load_dataset(_variant(made, "override", lambda m: m.update(orientation_override="none")), "train",
                      center_method="none")
    assert np.array_equal(ov.camera_to_worlds, written[ov.indices][:, :3])


def test_intrinsics_global_and_per_frame(made):
    def per_frame(meta):
        for k in ("fl_x", "fl_y", "cx", "cy", "w", "h"):
            v = meta.pop(k)
            for i, fr in enumerate(meta["frames"]):
                fr[k] = v + (0.5 * i if k in ("fl_x", "cx") else 0)

    g = load_dataset(made[0], "train", eval_mode="all")
    p = load_dataset(_variant(made, "per_frame", per_frame), "train", eval_mode="all")
    assert g.fx.dtype == np.float32 and g.fx.shape == (VIEWS,) and len(set(g.fx.tolist())) == 1
    assert np.allclose(p.fx, g.fx + 0.5 * np.arange(VIEWS)) and np.allclose(p.cx, g.cx + 0.5 * np.arange(VIEWS))
    assert np.array_equal(p.fy, g.fy) and (p.width, p.height) == (W, H)
    assert p.cameras[3].fx == float(p.fx[3]) and p.cameras[3].cx == float(p.cx[3])
    val = load_dataset(_variant(made, "per_frame", per_frame), "val")  # fraction: frame 10
    assert np.allclose(val.fx, g.fx[:1] + 5.0)

    def drop(meta):
        meta.pop("cx")

    with pytest.raises(ValueError, match="cx"):
        load_dataset(_variant(made, "no_cx", drop), "train")


def test_seed_cloud(made):
    from gs_io import read_point_cloud_ply

    out, meta, _ = made
    cloud = read_point_cloud_ply(os.path.join(out, "sparse_pc.ply"))
    raw = load_dataset(out, "train", orientation_method="none", center_method="none")
    assert raw.points3D_xyz.dtype == np.float32 and raw.points3D_rgb.dtype == np.uint8
    assert np.array_equal(raw.points3D_xyz, cloud["points"]) and np.array_equal(raw.points3D_rgb, cloud["colors"])
    ds = load_dataset(out, "val", auto_scale_poses=True)  # the same cloud for every split
    pts = torch.from_numpy(cloud["points"])
    want = (torch.cat((pts, torch.ones_like(pts[:, :1])), -1) @ torch.from_numpy(ds.transform).T) * ds.scale
    assert np.array_equal(ds.points3D_xyz, want.numpy())
    # applied_transform is folded into the dataparser transform the points go through
    applied = [[0, 1, 0, 0.5], [-1, 0, 0, 0], [0, 0, 1, -2.0]]
    at = load_dataset(_variant(made, "applied_transform", lambda m: m.update(applied_transform=applied)), "train",
                      orientation_method="none", center_method="none")
    A = np.array(applied, np.float32)
    assert np.allclose(at.points3D_xyz, cloud["points"] @ A[:, :3].T + A[:, 3], atol=1e-6)
    assert np.array_equal(at.camera_to_worlds, raw.camera_to_worlds)  # (the poses are not touched by it)
    none = load_dataset(_variant(made, "no_ply", lambda m: m.pop("ply_file_path")), "train")
    assert none.points3D_xyz is None and none.points3D_rgb is None


def test_mono_depth_scale_and_shift(made):
    from PIL import Image

    out, meta, _ = made
    os.makedirs(os.path.join(out, "mono"), exist_ok=True)
    rng = np.random.default_rng(0)
    planes = []
    for i in range(VIEWS):
        planes.append(rng.integers(0, 256, (H, W), dtype=np.uint8))
        Image.fromarray(planes[-1], "L").save(os.path.join(out, "mono", f"frame_{i:05d}.png"))

    def mono(meta):
        for i, fr in enumerate(meta["frames"]):
            fr.update(depth_path=f"mono/frame_{i:05d}.png", scale=1.5 + i, shift=-0.25 * i)

    ds = load_dataset(_variant(made, "mono", mono), "val")  # frame 10
    assert ds.mono_depth and ds.depth_unit == 1.0 / 255.0
    assert ds.mono_depth_scales == [11.5] and ds.mono_depth_shifts == [-2.5]
    z = ds.depth(0)
    assert z.dtype == np.uint8 and np.array_equal(z, planes[10])

    def partial(meta):
        meta["frames"][0]["scale"] = 2.0

    with pytest.raises(ValueError, match="scale"):
        load_dataset(_variant(made, "mono_partial", partial), "train")


REFUSALS = {
    "k1": lambda m: m.update(k1=0.01),
    "p2": lambda m: m["frames"][2].update(p2=-1e-3),
    "distortion_params": lambda m: m.update(distortion_params=[0, 0, 0.1, 0, 0, 0]),
    "camera_model": lambda m: m.update(camera_model="OPENCV_FISHEYE"),
    "differing size": lambda m: [m.pop("w"), [fr.update(w=W + (i == 5)) for i, fr in enumerate(m["frames"])]],
    "orientation_method": lambda m: m.update(orientation_override="pca"),
    r"\.npy": lambda m: m["frames"][1].update(depth_path="depths/frame_00001.npy"),
    r"\.exr": lambda m: [fr.update(depth_path=fr["depth_path"].replace(".png", ".exr")) for fr in m["frames"]],
    "mask_path": lambda m: m["frames"][4].pop("mask_path"),
}


@pytest.mark.parametrize("word", list(REFUSALS))
def test_refusals_name_the_key(made, word):
    p = _variant(made, "refused", REFUSALS[word])
    with pytest.raises(ValueError, match=word):
        load_dataset(p, "train")


def test_refused_config_values(made):
    out = made[0]
    for kw, word in ((dict(orientation_method="pca"), "orientation_method"),
                     (dict(orientation_method="vertical"), "orientation_method"),
                     (dict(center_method="focus"), "center_method"),
                     (dict(downscale_factor=2), "downscale_factor")):
        with pytest.raises(ValueError, match=word):
            load_dataset(out, "train", **kw)
    load_dataset(out, "train", downscale_factor=1)
    zero = _variant(made, "zero_distortion", lambda m: m.update(k1=0.0, p1=0.0, camera_model="OPENCV"))
    assert len(load_dataset(zero, "train")) == 11  # zero distortion is no distortion
    with pytest.raises(FileNotFoundError):
        load_dataset(os.path.join(out, "nowhere"), "train")


def test_against_the_reference_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "dataset_poses.npz"))
    # float32 torch on both sides and the same operations: held to 4 ulp of the largest pose entry (the golden was
    # recorded on another build of torch; matmul may order its sums differently)
    for name in ("orbit", "tilted", "single"):
        poses = g[f"poses_{name}"]
        tol = 4 * 2.0 ** -23 * float(np.abs(poses).max()) * 4  # four-term dot products
        for method in ("up", "none"):
            for centre in ("poses", "none"):
                oriented, transform = D.auto_orient_and_center_poses(poses, method, centre)
                assert oriented.shape == (len(poses), 3, 4)
                assert np.abs(oriented.numpy() - g[f"oriented_{name}_{method}_{centre}"]).max() <= tol
                assert np.abs(transform.numpy() - g[f"transform_{name}_{method}_{centre}"]).max() <= tol
    up = torch.from_numpy(g["poses_tilted"])[:, :3, 1].mean(0)
    assert float(up[2] / up.norm()) < 0.0  # the tilted set's mean up vector is far from +z ...
    up = torch.from_numpy(g["oriented_tilted_up_poses"])[:, :3, 1].mean(0)
    assert float(up[2] / up.norm()) > 1 - 1e-5  # ... and the reference turned it there
    assert np.abs(g["oriented_single_up_poses"][0, :, 3]).max() < 1e-6  # one frame: centred on itself
    for n in (1, 2, 9, 10, 12, 31, 100):
        for frac in (0.9, 0.5):
            tr, ev = D.split_fraction(n, frac)
            assert np.array_equal(tr, g[f"fraction_{n}_{frac}_train"]) and np.array_equal(ev, g[f"fraction_{n}_{frac}_eval"])
        for k in (8, 3):
            tr, ev = D.split_interval(n, k)
            assert np.array_equal(tr, g[f"interval_{n}_{k}_train"]) and np.array_equal(ev, g[f"interval_{n}_{k}_eval"])
        tr, ev = D.split_all(n)
        assert np.array_equal(tr, g[f"all_{n}_train"]) and np.array_equal(ev, g[f"all_{n}_eval"])
    tr, ev = D.split_filename([str(s) for s in g["filename_names"]])
    assert np.array_equal(tr, g["filename_train"]) and np.array_equal(ev, g["filename_eval"])
