"""A dataset directory as the toolkit's own dataparser reads it (`GSToolkit._generate_dataparser_outputs`,
gs_toolkit/data/dataparsers/gs_toolkit_dataparser.py:77-432), restated for what this trainer can use: a
`transforms.json` with perspective, undistorted frames of one size, images / masks / depth read with Pillow into the
integer dtypes of data/datasets/base_dataset.py, the SfM seed cloud, and the cameras as `get_outputs` builds them
(vanilla_gs.py:722-742).  Host code: NumPy, torch on the CPU for the float32 pose arithmetic the reference does in
torch, Pillow for the files.  What is refused is refused by name (ValueError), never silently read differently.
"""
import json
import math
import os
from dataclasses import dataclass, field
from pathlib import PurePath
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .ply import read_point_cloud_ply

PERSPECTIVE_MODELS = ("SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV")
FISHEYE_MODELS = ("OPENCV_FISHEYE",)  # read with `allow_fisheye` and zero distortion: the ideal equidistant lens
DISTORTION_KEYS = ("k1", "k2", "k3", "k4", "p1", "p2")
IMAGE_DEPTH_SUFFIXES = (".png", ".jpg", ".jpeg")


# ---- splits (data/utils/dataparsers_utils.py) -------------------------------------------------------------------
def split_fraction(num_images: int, train_split_fraction: float) -> Tuple[np.ndarray, np.ndarray]:
    """Equally spaced training images from the first to the last; the rest evaluate."""
    num_train = math.ceil(num_images * train_split_fraction)
    i_train = np.linspace(0, num_images - 1, num_train, dtype=int)
    i_eval = np.setdiff1d(np.arange(num_images), i_train)
    if len(i_eval) != num_images - num_train:
        raise ValueError(f"train_split_fraction {train_split_fraction} picks a frame of {num_images} twice")
    return i_train, i_eval


def split_filename(image_filenames: List[str]) -> Tuple[np.ndarray, np.ndarray]:
    i_train, i_eval = [], []
    for i, name in enumerate(os.path.basename(f) for f in image_filenames):
        if "train" in name:
            i_train.append(i)
        elif "eval" in name:
            i_eval.append(i)
        else:
            raise ValueError(f"eval_mode 'filename': {name!r} holds neither 'train' nor 'eval'")
    return np.array(i_train, dtype=int), np.array(i_eval, dtype=int)


def split_interval(num_images: int, eval_interval: int) -> Tuple[np.ndarray, np.ndarray]:
    i_all = np.arange(num_images)
    return i_all[i_all % eval_interval != 0], i_all[i_all % eval_interval == 0]


def split_all(num_images: int) -> Tuple[np.ndarray, np.ndarray]:
    i_all = np.arange(num_images)
    return i_all, i_all


# ---- orientation and centring (cameras/camera_utils.py:462-493, 552-660), float32 torch as there ----------------
def rotation_between(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """The rotation that turns `a` into `b` (Rodrigues); exactly opposite vectors get a little noise, as there."""
    a = a / torch.linalg.norm(a)
    b = b / torch.linalg.norm(b)
    v = torch.linalg.cross(a, b)
    c = torch.dot(a, b)
    if c < -1 + 1e-8:
        return rotation_between(a + (torch.rand(3) - 0.5) * 0.01, b)
    s = torch.linalg.norm(v)
    k = torch.tensor([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype=torch.float32)
    return torch.eye(3) + k + k @ k * ((1 - c) / (s ** 2 + 1e-8))


def auto_orient_and_center_poses(poses, method: str = "up", center_method: str = "poses"):
    """poses [n,4,4] (or [n,3,4]) float32 -> (oriented [n,3,4], transform [3,4]).  `method`: "up" (the mean up vector
    becomes +z) or "none"; `center_method`: "poses" (the mean origin becomes 0) or "none"."""
    poses = torch.as_tensor(np.asarray(poses), dtype=torch.float32)
    if center_method not in ("poses", "none"):
        raise ValueError(f"center_method {center_method!r} is not supported (only 'poses' and 'none')")
    if method not in ("up", "none"):
        raise ValueError(f"orientation_method {method!r} is not supported (only 'up' and 'none')")
    mean_origin = torch.mean(poses[..., :3, 3], dim=0)
    translation = mean_origin if center_method == "poses" else torch.zeros_like(mean_origin)
    if method == "up":
        up = torch.mean(poses[:, :3, 1], dim=0)
        up = up / torch.linalg.norm(up)
        rotation = rotation_between(up, torch.tensor([0.0, 0.0, 1.0]))
        transform = torch.cat([rotation, rotation @ -translation[..., None]], dim=-1)
    else:
        transform = torch.eye(4)
        transform[:3, 3] = -translation
        transform = transform[:3, :]
    if poses.shape[-2] == 3:
        poses = torch.cat([poses, torch.tensor([[[0.0, 0.0, 0.0, 1.0]]]).expand(poses.shape[0], 1, 4)], dim=1)
    return transform @ poses, transform


# ---- cameras (vanilla_gs.py:722-742, 770-771) -------------------------------------------------------------------
def camera_from_pose(c2w: np.ndarray, fx: float, fy: float, cx: float, cy: float, width: int, height: int,
                     model: str = "pinhole"):
    """`harness.scene.Camera` of a camera-to-world [3,4]: the y/z flip into the rasterizer's convention, the analytic
    inverse, the fields of view from width / fx, `projection_matrix(0.001, 1000, fovx, fovy) @ viewmat` -- float32.
    `model`: "pinhole" or "fisheye" (the projection matrix is formed alike; the fisheye projection does not read it)."""
    from harness import scene as S

    c2w = torch.as_tensor(np.asarray(c2w, np.float32))
    R = c2w[:3, :3] @ torch.diag(torch.tensor([1.0, -1.0, -1.0]))
    T = c2w[:3, 3:4]
    R_inv = R.T
    viewmat = torch.eye(4)
    viewmat[:3, :3] = R_inv
    viewmat[:3, 3:4] = -R_inv @ T
    fx, fy, cx, cy = (float(np.float32(v)) for v in (fx, fy, cx, cy))
    fovx, fovy = 2 * math.atan(width / (2 * fx)), 2 * math.atan(height / (2 * fy))
    V = viewmat.numpy().copy()
    P = S.projection_matrix(0.001, 1000.0, fovx, fovy) @ V
    return S.Camera(int(width), int(height), fx, fy, cx, cy, V, P.astype(np.float32), model)


# ---- files (data/datasets/base_dataset.py:52-128, data/utils/data_utils.py:13-30) --------------------------------
def read_image_u8(path: str) -> np.ndarray:
    """uint8 [H,W,3|4]; a grey image is replicated to three channels."""
    from PIL import Image

    image = np.array(Image.open(path), dtype="uint8")
    if image.ndim == 2:
        image = image[:, :, None].repeat(3, axis=2)
    if image.ndim != 3 or image.shape[2] not in (3, 4):
        raise ValueError(f"{path}: image of shape {image.shape}")
    return np.ascontiguousarray(image)


def read_mask_u8(path: str) -> np.ndarray:
    """uint8 [H,W], 1 where the file is non-zero."""
    from PIL import Image

    m = Image.open(path)
    if np.array(m).ndim == 3:
        m = m.convert("L")
    return np.ascontiguousarray((np.array(m) != 0).astype(np.uint8))


def read_depth_int(path: str, mono: bool) -> np.ndarray:
    """The PNG's integer values: uint16 [H,W] (unit 1e-3), or -- monocular depth -- uint8 (unit 1 / 255)."""
    from PIL import Image

    suffix = os.path.splitext(path)[1].lower()
    if suffix not in IMAGE_DEPTH_SUFFIXES:
        raise ValueError(f"depth_path {path!r}: only integer image files are read ({suffix or 'no suffix'} is not)")
    d = np.array(Image.open(path))
    if d.ndim != 2 or d.dtype.kind not in "ui" or d.min() < 0 or d.max() > (255 if mono else 65535):
        raise ValueError(f"depth_path {path!r}: expected one integer channel, got {d.dtype} {d.shape}")
    return np.ascontiguousarray(d.astype(np.uint8 if mono else np.uint16))


@dataclass
class Dataset:
    """One split of a dataset directory.  Poses, intrinsics and file names per view of THIS split, in file-name order;
    `scale` and `transform` are the dataparser's (`dataparser_scale`, `dataparser_transform`)."""
    root: str
    split: str
    indices: np.ndarray                      # this split's frames among all frames (sorted by file name)
    image_filenames: List[str]
    mask_filenames: Optional[List[str]]
    depth_filenames: Optional[List[str]]
    camera_to_worlds: np.ndarray             # float32 [n,3,4], oriented, centred and scaled
    fx: np.ndarray                           # float32 [n]
    fy: np.ndarray
    cx: np.ndarray
    cy: np.ndarray
    width: int
    height: int
    scale: float
    transform: np.ndarray                    # float32 [3,4], `applied_transform` folded in
    points3D_xyz: Optional[np.ndarray]       # float32 [m,3] in the oriented, scaled frame
    points3D_rgb: Optional[np.ndarray]       # uint8 [m,3]
    mono_depth_scales: List[float] = field(default_factory=list)
    mono_depth_shifts: List[float] = field(default_factory=list)
    depth_unit_scale_factor: float = 1e-3
    cameras: list = field(default_factory=list)  # harness.scene.Camera per view
    camera_model: str = "pinhole"            # or "fisheye": OPENCV_FISHEYE with every distortion coefficient zero

    def __len__(self) -> int:
        return len(self.image_filenames)

    @property
    def mono_depth(self) -> bool:
        return bool(self.mono_depth_scales or self.mono_depth_shifts)

    @property
    def depth_unit(self) -> float:
        """What one count of the depth files is worth: 1 / 255 for monocular depth (base_dataset.py:118-121), else
        `depth_unit_scale_factor`.  The pose scale is NOT applied to depth, as in the reference's dataset."""
        return 1.0 / 255.0 if self.mono_depth else self.depth_unit_scale_factor

    def image(self, i: int) -> np.ndarray:
        img = read_image_u8(self.image_filenames[i])
        if img.shape[:2] != (self.height, self.width):
            raise ValueError(f"{self.image_filenames[i]}: {img.shape[1]}x{img.shape[0]} pixels, transforms.json says "
                             f"{self.width}x{self.height}")
        return img

    def mask(self, i: int) -> Optional[np.ndarray]:
        if self.mask_filenames is None:
            return None
        m = read_mask_u8(self.mask_filenames[i])
        if m.shape != (self.height, self.width):
            raise ValueError(f"{self.mask_filenames[i]}: mask and image have different shapes")
        return m

    def depth(self, i: int) -> Optional[np.ndarray]:
        if self.depth_filenames is None:
            return None
        d = read_depth_int(self.depth_filenames[i], self.mono_depth)
        if d.shape != (self.height, self.width):
            raise ValueError(f"{self.depth_filenames[i]}: depth and image have different shapes")
        return d


def _distortion(where: str, holder: Dict) -> None:
    for k in DISTORTION_KEYS:
        if k in holder and float(holder[k]) != 0.0:
            raise ValueError(f"{where}: distortion parameter {k} = {holder[k]} -- undistortion is not part of this loader")
    if "distortion_params" in holder and any(float(v) != 0.0 for v in holder["distortion_params"]):
        raise ValueError(f"{where}: non-zero distortion_params -- undistortion is not part of this loader")


def _split_indices(meta: Dict, split: str, names: List[str], rel: List[str], data_dir: str, eval_mode: str,
                   train_split_fraction: float, eval_interval: int) -> np.ndarray:
    if split not in ("train", "val", "test"):
        raise ValueError(f"Unknown dataparser split {split}")
    if f"{split}_filenames" in meta:
        wanted = {os.path.join(data_dir, x) for x in meta[f"{split}_filenames"]}
        missing = wanted.difference(names)
        if missing:
            raise RuntimeError(f"Some filenames for split {split} were not found: {sorted(missing)}.")
        return np.array([i for i, p in enumerate(names) if p in wanted], dtype=np.int32)
    if any(f"{s}_filenames" in meta for s in ("train", "val", "test")):
        raise RuntimeError(f"The dataset's list of filenames for split {split} is missing.")
    n = len(names)
    if eval_mode == "fraction":
        i_train, i_eval = split_fraction(n, train_split_fraction)
    elif eval_mode == "filename":
        i_train, i_eval = split_filename(rel)
    elif eval_mode == "interval":
        i_train, i_eval = split_interval(n, eval_interval)
    elif eval_mode == "all":
        i_train, i_eval = split_all(n)
    else:
        raise ValueError(f"Unknown eval mode {eval_mode}")
    return i_train if split == "train" else i_eval


def load_dataset(path: str, split: str = "train", *, scale_factor: float = 1.0, downscale_factor: Optional[int] = None,
                 orientation_method: str = "up", center_method: str = "poses", auto_scale_poses: bool = False,
                 eval_mode: str = "fraction", train_split_fraction: float = 0.9, eval_interval: int = 8,
                 depth_unit_scale_factor: float = 1e-3, allow_fisheye: bool = False) -> Dataset:
    """`path`: a directory holding `transforms.json`, or the json itself.  The keyword arguments are the fields of
    `GSToolkitDataParserConfig` with its defaults.  `allow_fisheye`: also read `camera_model: OPENCV_FISHEYE` where
    every distortion coefficient is zero (the ideal equidistant lens, `Dataset.camera_model == "fisheye"`): the caller
    renders such cameras through gs_fused.project_gaussians_fisheye, nothing is undistorted."""
    path = os.fspath(path)
    if not os.path.exists(path):
        raise FileNotFoundError(f"Data directory {path} does not exist.")
    json_path = path if path.endswith(".json") else os.path.join(path, "transforms.json")
    data_dir = os.path.dirname(json_path)
    with open(json_path, "r", encoding="utf-8") as f:
        meta = json.load(f)
    if downscale_factor not in (None, 1):
        raise ValueError(f"downscale_factor {downscale_factor}: downscaled image folders (images_{downscale_factor}/) "
                         f"are not read; the trainer's resolution schedule resizes on the GPU")
    model = meta.get("camera_model", "PINHOLE")
    fisheye = allow_fisheye and model in FISHEYE_MODELS
    if model not in PERSPECTIVE_MODELS and not fisheye:
        raise ValueError(f"camera_model {model!r} is not a perspective camera"
                         + (" (allow_fisheye=True reads it where every distortion coefficient is zero)"
                            if model in FISHEYE_MODELS else ""))
    if meta.get("fisheye_crop_radius") is not None:
        raise ValueError("fisheye_crop_radius: fisheye images are not supported"
                         + (" with a crop radius (pass the image circle as mask_path)" if fisheye else ""))
    _distortion("transforms.json", meta)
    if "applied_scale" in meta:
        scale_factor = float(meta["applied_scale"])
    method = meta.get("orientation_override", orientation_method)
    if method not in ("up", "none"):
        raise ValueError(f"orientation_method {method!r} is not supported (only 'up' and 'none')")
    if center_method not in ("poses", "none"):
        raise ValueError(f"center_method {center_method!r} is not supported (only 'poses' and 'none')")

    frames = meta["frames"]
    if not frames:
        raise ValueError("transforms.json: no frames")
    # (the reference argsorts pathlib.Path objects: by path components, not by the joined string)
    frames = sorted(frames, key=lambda fr: PurePath(os.path.join(data_dir, fr["file_path"])).parts)

    def intrinsic(key: str, kind):
        if key in meta:
            return [kind(meta[key])] * len(frames)
        for fr in frames:
            if key not in fr:
                raise ValueError(f"{key} is neither global nor given for frame {fr['file_path']!r}")
        return [kind(fr[key]) for fr in frames]

    fx, fy, cx, cy = (intrinsic(k, float) for k in ("fl_x", "fl_y", "cx", "cy"))
    hs, ws = intrinsic("h", int), intrinsic("w", int)
    if len(set(hs)) != 1 or len(set(ws)) != 1:
        raise ValueError(f"frames of differing size (h in {sorted(set(hs))}, w in {sorted(set(ws))}): one size per "
                         f"dataset is supported")
    rel, names, masks, depths, scales, shifts, poses = [], [], [], [], [], [], []
    for fr in frames:
        _distortion(f"frame {fr['file_path']!r}", fr)
        rel.append(fr["file_path"])
        names.append(os.path.join(data_dir, fr["file_path"]))
        poses.append(np.array(fr["transform_matrix"]))
        if "scale" in fr:
            scales.append(float(fr["scale"]))
        if "shift" in fr:
            shifts.append(float(fr["shift"]))
        if "mask_path" in fr:
            masks.append(os.path.join(data_dir, fr["mask_path"]))
        if "depth_path" in fr:
            suffix = os.path.splitext(fr["depth_path"])[1].lower()
            if suffix not in IMAGE_DEPTH_SUFFIXES:
                raise ValueError(f"depth_path {fr['depth_path']!r}: {suffix} depth is not read (integer PNG only)")
            depths.append(os.path.join(data_dir, fr["depth_path"]))
    n = len(frames)
    for what, lst in (("mask_path", masks), ("depth_path", depths), ("scale", scales), ("shift", shifts)):
        if len(lst) not in (0, n):
            raise ValueError(f"{what} is given for {len(lst)} of {n} frames: every frame or none")

    indices = _split_indices(meta, split, names, rel, data_dir, eval_mode, train_split_fraction, eval_interval)

    # orientation, centring and scale over ALL frames, before the split (gs_toolkit_dataparser.py:268-305)
    all_poses, transform = auto_orient_and_center_poses(np.array(poses).astype(np.float32), method, center_method)
    scale = 1.0
    if auto_scale_poses:
        scale /= float(torch.max(torch.abs(all_poses[:, :3, 3])))
    scale *= scale_factor
    all_poses[:, :3, 3] *= scale
    sel = torch.as_tensor(np.asarray(indices), dtype=torch.long)
    c2w = all_poses[sel].numpy().astype(np.float32)

    if "applied_transform" in meta:
        applied = torch.tensor(meta["applied_transform"], dtype=transform.dtype)
        transform = transform @ torch.cat([applied, torch.tensor([[0, 0, 0, 1]], dtype=transform.dtype)], 0)

    xyz = rgb = None
    if "ply_file_path" in meta:  # `_load_3D_points` (:434-457)
        cloud = read_point_cloud_ply(os.path.join(data_dir, meta["ply_file_path"]))
        pts = torch.from_numpy(np.asarray(cloud["points"], dtype=np.float32))
        pts = torch.cat((pts, torch.ones_like(pts[..., :1])), -1) @ transform.T
        pts *= scale
        xyz = pts.numpy()
        rgb = cloud["colors"] if cloud["colors"] is not None else np.full((len(xyz), 3), 128, np.uint8)

    pick = lambda lst: [lst[i] for i in indices]  # noqa: E731
    arr = lambda lst: np.array(pick(lst), dtype=np.float32)  # noqa: E731
    ds = Dataset(root=data_dir, split=split, indices=np.asarray(indices), image_filenames=pick(names),
                 mask_filenames=pick(masks) if masks else None, depth_filenames=pick(depths) if depths else None,
                 camera_to_worlds=c2w, fx=arr(fx), fy=arr(fy), cx=arr(cx), cy=arr(cy), width=ws[0], height=hs[0],
                 scale=float(scale), transform=transform.numpy().astype(np.float32), points3D_xyz=xyz,
                 points3D_rgb=rgb, mono_depth_scales=pick(scales) if scales else [],
                 mono_depth_shifts=pick(shifts) if shifts else [], depth_unit_scale_factor=depth_unit_scale_factor)
    ds.camera_model = "fisheye" if fisheye else "pinhole"
    ds.cameras = [camera_from_pose(c2w[i], ds.fx[i], ds.fy[i], ds.cx[i], ds.cy[i], ds.width, ds.height, ds.camera_model)
                  for i in range(len(ds))]
    return ds
