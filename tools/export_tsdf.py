"""Point cloud and mesh from a trained Gaussian model: the toolkit's `ExportTSDF` on the GPU, without Open3D.

    python tools/export_tsdf.py --ply MODEL.ply --poses poses.json --out DIR
        [--voxel-length 0.01171875] [--sdf-trunc 0.06] [--depth-trunc 10] [--bounds x0 y0 z0 x1 y1 z1]
        [--capacity BLOCKS] [--alpha-min 0.5] [--background r g b] [--no-clean] [--min-component-faces 20000]
        [--gt GT.{stl,ply}] [--gt-threshold T] [--masks MASKS.npy [--bounding-box]]
        [--obb-pos X Y Z --obb-rpy R P Y --obb-scale SX SY SZ]

Renders RGB + depth from every camera of `poses.json` (the trajectory file `TSDFFusion.read_trajectory` reads), fuses
the views into a block-sparse TSDF volume (gs_fusion) and writes `point_cloud.ply` and `mesh.ply` to DIR.  File names
and defaults are `ExportTSDF`'s (gs_toolkit/scripts/exporter.py:233-237).  Without --bounds the volume is the box of
the Gaussians' 1st-99th percentiles per axis, padded by the truncation distance.  With cleaning on (the default, as
`ExportTSDF.clean`), `cleaned_mesh.ply` is written as well: `mesh.ply` without null faces, duplicate faces, connected
components of fewer than --min-component-faces faces and unreferenced vertices (gs_fusion.clean_mesh).  With --gt the
JSON line also carries the surface distance of `mesh.ply` (fields `mesh_average_error`, `mesh_rms`, ...) and, when it
was written, of `cleaned_mesh.ply` (`cleaned_average_error`, ...) against that ground truth: what tools/eval_surface.py
prints for each file.

--masks MASKS.npy restricts the fusion to an object, as `ExportTSDF`'s `using_mask` / `mask_path` do: a uint8 array
[V,H,W] or [V,H,W,3], one mask per camera of `poses.json` in its order; a view's depth is fused only where its mask is
non-zero (for three channels: where 0.21 R + 0.72 G + 0.07 B, truncated to 8 bits, is non-zero -- gs_fusion.export_mask).
--bounding-box fuses inside the rectangle around each mask's non-zero pixels, grown by 5 pixels, instead (`bounding_box`).
The toolkit reads the masks as PNG files (`Annotations/frame_%05d.png`); this project depends on no image library, so
decoding them into the .npy array stays with the caller.

--obb-pos / --obb-rpy / --obb-scale (all three, or none) cut the object out in 3-D instead: the oriented crop box of
the toolkit's viewer (`OrientedBox.from_params`: position, roll-pitch-yaw in radians, extents).  Every view is rendered
with the Gaussians whose centre lies inside it (gs_fused.CropBox, a test inside the projection kernel), and without
--bounds the volume is sized by those Gaussians alone.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-splatting-toolkit_amd")]
import numpy as np
import torch

from gs_fused.crop import CropBox
from gs_fusion import TSDFVolume, clean_mesh, fuse_views, read_poses_json
from gs_io import read_gaussian_ply, write_mesh_ply, write_point_cloud_ply

DEFAULT_CAPACITY = 200_000  # blocks of 10 KiB: 2 GB


def default_bounds(means: np.ndarray, pad: float):
    lo, hi = np.percentile(means.astype(np.float64), [1.0, 99.0], axis=0)
    return lo - pad, hi + pad


def activated(raw, device):
    """Raw values of a Gaussian PLY -> what `render_view` takes."""
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in raw.items()}
    return {"means3d": t["means"], "scales": torch.exp(t["scales"]),
            "quats": t["quats"] / t["quats"].norm(dim=-1, keepdim=True), "opacities": torch.sigmoid(t["opacities"]),
            "sh_coeffs": torch.cat([t["features_dc"][:, None, :], t["features_rest"]], 1).contiguous()}


def load_masks(path, num_views):
    """--masks: [V,H,W] or [V,H,W,3] uint8, one mask per camera."""
    masks = np.load(path)
    if masks.dtype != np.uint8 or masks.ndim not in (3, 4) or (masks.ndim == 4 and masks.shape[-1] != 3):
        raise SystemExit(f"export_tsdf: --masks must be a uint8 array [V,H,W] or [V,H,W,3], got {masks.dtype} "
                         f"{masks.shape}")
    if masks.shape[0] != num_views:
        raise SystemExit(f"export_tsdf: {masks.shape[0]} masks for {num_views} cameras")
    return masks


def add_obb_arguments(ap):
    """--obb-pos / --obb-rpy / --obb-scale, shared with tools/export_gaussians.py."""
    ap.add_argument("--obb-pos", type=float, nargs=3, metavar=("X", "Y", "Z"), help="crop box: centre")
    ap.add_argument("--obb-rpy", type=float, nargs=3, metavar=("R", "P", "Y"),
                    help="crop box: roll, pitch, yaw in radians (R = Rz(yaw) Ry(pitch) Rx(roll))")
    ap.add_argument("--obb-scale", type=float, nargs=3, metavar=("SX", "SY", "SZ"), help="crop box: extents")


def obb_from_args(ap, a):
    """-> CropBox or None; the three options come together, extents must not be negative."""
    given = [v is not None for v in (a.obb_pos, a.obb_rpy, a.obb_scale)]
    if not any(given):
        return None
    if not all(given):
        ap.error("--obb-pos, --obb-rpy and --obb-scale go together")
    if min(a.obb_scale) < 0:
        ap.error("--obb-scale must not be negative")
    try:
        return CropBox.from_params(a.obb_pos, a.obb_rpy, a.obb_scale)
    except ValueError as e:
        ap.error(str(e))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ply", required=True)
    ap.add_argument("--poses", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--voxel-length", type=float, default=0.01171875)  # 6 / 512
    ap.add_argument("--sdf-trunc", type=float, default=0.06)
    ap.add_argument("--depth-trunc", type=float, default=10.0)
    ap.add_argument("--bounds", type=float, nargs=6, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--capacity", type=int, default=None, help="pool size in blocks of 8x8x8 voxels")
    ap.add_argument("--alpha-min", type=float, default=0.5)
    ap.add_argument("--background", type=float, nargs=3, default=(0.0, 0.0, 0.0))
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--clean", dest="clean", action="store_true", default=True,
                    help="also write cleaned_mesh.ply (default)")
    ap.add_argument("--no-clean", dest="clean", action="store_false")
    ap.add_argument("--min-component-faces", type=int, default=20000,
                    help="components of fewer faces are removed from cleaned_mesh.ply")
    ap.add_argument("--gt", default=None, help="ground-truth mesh (.stl or .ply): append surface-distance fields")
    ap.add_argument("--gt-threshold", type=float, default=None)
    ap.add_argument("--masks", default=None,
                    help="uint8 .npy [V,H,W] or [V,H,W,3], one object mask per camera: fuse depth only where it is "
                         "non-zero (PNG masks must be decoded by the caller: no image library here)")
    ap.add_argument("--bounding-box", action="store_true",
                    help="with --masks: fuse inside each mask's bounding rectangle grown by 5 pixels")
    ap.add_argument("--rasterize-mode", default="classic", choices=["classic", "antialiased"],
                    help="the mode the model was trained in: antialiased composites opacities * compensation "
                         "(a model trained that way gives wrong depth and alpha in classic mode)")
    ap.add_argument("--depth-mode", default="expected", choices=["expected", "median"],
                    help="the depth of a view that is fused: the alpha-blended depth, or the depth of the Gaussian at "
                         "which the transmittance crosses 0.5 (no blend of foreground and background at a silhouette)")
    add_obb_arguments(ap)
    a = ap.parse_args(argv)
    a.crop_box = obb_from_args(ap, a)
    if a.min_component_faces < 0:
        ap.error("--min-component-faces must not be negative")
    if a.gt_threshold is not None and not a.gt_threshold >= 0:
        ap.error("--gt-threshold must not be negative")
    if a.bounding_box and not a.masks:
        ap.error("--bounding-box needs --masks")
    return a


def write_cleaned(out_dir, vertices, vcolors, triangles, min_component_faces):
    """`cleaned_mesh.ply` from the device tensors of `mesh.ply` -> the rows it adds to the JSON line.  A mesh of which
    nothing is left is written as a file with zero vertices and zero faces."""
    cv, cc, ct, info = clean_mesh(vertices, triangles, vcolors, min_component_faces, return_info=True)
    write_mesh_ply(os.path.join(out_dir, "cleaned_mesh.ply"), cv.cpu().numpy(), ct.cpu().numpy(), cc.cpu().numpy())
    return {"cleaned_vertices": int(cv.shape[0]), "cleaned_triangles": int(ct.shape[0]),
            "components": info["components"]}


def main(argv=None):
    a = parse_args(argv)

    raw = read_gaussian_ply(a.ply)
    try:
        cams = read_poses_json(a.poses)  # (refuses a fisheye camera by name: fusion is pinhole only)
    except ValueError as e:
        raise SystemExit(f"export_tsdf: {e}") from None
    masks = load_masks(a.masks, len(cams)) if a.masks else None
    if a.bounds:
        lo, hi = np.asarray(a.bounds[:3]), np.asarray(a.bounds[3:])
    else:
        means = raw["means"]
        if a.crop_box is not None:
            inside = a.crop_box.within(torch.from_numpy(np.ascontiguousarray(means, np.float32))).numpy()
            if not inside.any():
                raise SystemExit("export_tsdf: the crop box keeps no Gaussian")
            means = means[inside]
        lo, hi = default_bounds(means, a.sdf_trunc)
    if not (hi > lo).all():
        raise SystemExit("export_tsdf: empty bounds")
    blocks = np.maximum(1, np.ceil((hi - lo) / (8.0 * a.voxel_length) - 1e-9)).astype(int)
    capacity = a.capacity if a.capacity else min(int(np.prod(blocks)), DEFAULT_CAPACITY)
    vol = TSDFVolume.from_bounds(lo, hi, a.voxel_length, a.sdf_trunc, capacity, a.device)
    params = activated(raw, vol.device)
    K = params["sh_coeffs"].shape[1]
    bg = torch.tensor(a.background, dtype=torch.float32, device=vol.device)
    fuse_views(vol, params, cams, bg, {1: 0, 4: 1, 9: 2, 16: 3}.get(K, 4), alpha_min=a.alpha_min,
               depth_trunc=a.depth_trunc, masks=masks, bounding_box=a.bounding_box, rasterize_mode=a.rasterize_mode,
               crop_box=a.crop_box, depth_mode=a.depth_mode)
    points, colors, normals = vol.extract_point_cloud()
    vertices, vcolors, triangles = vol.extract_mesh()
    os.makedirs(a.out, exist_ok=True)
    cpu = lambda t: t.cpu().numpy()  # noqa: E731
    write_point_cloud_ply(os.path.join(a.out, "point_cloud.ply"), cpu(points), cpu(colors), cpu(normals))
    write_mesh_ply(os.path.join(a.out, "mesh.ply"), cpu(vertices), cpu(triangles), cpu(vcolors))
    summary = {"views": len(cams), "blocks": [int(b) for b in vol.blocks], "capacity": vol.capacity,
               "allocated_blocks": vol.num_allocated_blocks, "points": int(points.shape[0]),
               "vertices": int(vertices.shape[0]), "triangles": int(triangles.shape[0]), "out": a.out}
    if masks is not None:
        summary["masks"] = "bounding box" if a.bounding_box else "mask"
    if a.crop_box is not None:
        summary["crop_box"] = {"pos": list(a.obb_pos), "rpy": list(a.obb_rpy), "scale": list(a.obb_scale)}
    if a.clean:
        summary.update(write_cleaned(a.out, vertices, vcolors, triangles, a.min_component_faces))
    if a.gt:
        from eval_surface import evaluate, load_mesh

        gt = load_mesh(a.gt)
        for name, prefix in (("mesh.ply", "mesh_"), ("cleaned_mesh.ply", "cleaned_")):
            path = os.path.join(a.out, name)
            if os.path.exists(path) and (name == "mesh.ply" or a.clean):
                summary.update(evaluate(gt, load_mesh(path), vol.device, threshold=a.gt_threshold, prefix=prefix))
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
