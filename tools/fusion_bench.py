"""TSDF fusion on the bench scene: render and fuse K views, per-view medians by device events.

    python tools/fusion_bench.py [--views 100] [--gaussians 1000000] [--width 1920] [--height 1080]
                                 [--no-torch] [--out profiles/fusion_bench.json]

Volume: 512^3 voxel positions of L = 6/512 (a 6 m box over the scene), sdf_trunc = 0.06, every block in the pool.
Reported per view (median over the views after the warm-up ones): render ms, touch + allocate ms, integrate ms,
integrate bytes (40 B per updated voxel + 8 B per visited, not updated voxel) over time as a fraction of the 8 TB/s
HBM peak, and the same integration written in plain torch ops over the same listed blocks (what a user could write
without this package); then point-cloud and mesh extraction (host clock around a call that ends in its read-back);
then `clean`: gs_fusion.clean_mesh (label + emit, min_component_faces = 20000) on the mesh just extracted, host clock
around the synchronised call, and next to it the same mesh's face components through
`scipy.sparse.csgraph.connected_components` on the host (the labelling alone, the mesh already in host memory), when
scipy imports; then `eval`: gs_fusion.MeshDistance on the mesh just extracted (BVH build, host clock around the
synchronised call) and the query of its own vertices moved by half a voxel along x (device events), the size of job
tools/eval_surface.py does for an exported mesh.
Kernel names and times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/fusion_bench.py
--no-torch` run (tools/summarize_prof.py).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-splatting-toolkit_amd")]
import numpy as np
import torch

from gs_fusion import MeshDistance, TSDFVolume, clean_mesh, view_depth
from gs_fusion.volume import ST_LIST
from harness import scene as S
from harness.pipeline import CameraTensors, render_view
from rasterizer.cuda import _stream

HBM_PEAK = 8.0e12


def torch_integrate(vol, pool, blocks, depth, color, valid, cam, depth_trunc):
    """The integration rule in plain torch ops over the listed blocks; `pool` = (tsdf, weight, color) to update."""
    dev = depth.device
    Bx, By, _ = vol.blocks
    slots = vol.table.reshape(-1)[blocks].long()
    v = torch.arange(512, device=dev)
    g = [((blocks % Bx) * 8)[:, None] + (v & 7), (((blocks // Bx) % By) * 8)[:, None] + ((v >> 3) & 7),
         ((blocks // (Bx * By)) * 8)[:, None] + (v >> 6)]
    p = [vol.origin[a] + (g[a].float() + 0.5) * vol.voxel_length for a in range(3)]
    V = torch.from_numpy(cam.viewmat).to(dev)
    pc = [((V[r, 0] * p[0] + V[r, 1] * p[1]) + V[r, 2] * p[2]) + V[r, 3] for r in range(3)]
    H, W = depth.shape
    z = torch.where(pc[2] > 0, pc[2], torch.ones_like(pc[2]))
    ju, iv = torch.floor(cam.fx * (pc[0] / z) + cam.cx), torch.floor(cam.fy * (pc[1] / z) + cam.cy)
    live = (pc[2] > 0) & (ju >= 0) & (ju < W) & (iv >= 0) & (iv < H)
    j, i = ju.clamp(0, W - 1).long(), iv.clamp(0, H - 1).long()
    d = depth[i, j]
    live &= (d > 0) & (d <= depth_trunc) & (valid[i, j] != 0)
    xn, yn = ((j.float() + 0.5) - cam.cx) / cam.fx, ((i.float() + 0.5) - cam.cy) / cam.fy
    sdf = (d - pc[2]) * torch.sqrt((1 + xn * xn) + yn * yn)
    upd = live & (sdf > -vol.sdf_trunc)
    f = torch.clamp(sdf / vol.sdf_trunc, max=1.0)
    tsdf, weight, col = pool
    w = weight[slots]
    w1 = w + 1
    tsdf[slots] = torch.where(upd, (tsdf[slots] * w + f) / w1, tsdf[slots])
    col[slots] = torch.where(upd[..., None], (col[slots] * w[..., None] + color[i, j]) / w1[..., None], col[slots])
    weight[slots] = torch.where(upd, w1, w)


def scipy_components_ms(triangles, num_vertices):
    """Face components of a host mesh with scipy (faces that share an edge linked in a sparse graph), or None."""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        return None
    t0 = time.perf_counter()
    tri = triangles.astype(np.int64)
    he = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]), axis=1)
    key = he[:, 0] * num_vertices + he[:, 1]
    order = np.argsort(key, kind="stable")
    face = np.tile(np.arange(len(tri)), 3)[order]
    same = key[order][1:] == key[order][:-1]
    g = coo_matrix((np.ones(int(same.sum()), np.int8), (face[:-1][same], face[1:][same])), shape=(len(tri),) * 2)
    n, _ = connected_components(g, directed=False)
    return round((time.perf_counter() - t0) * 1e3, 3), int(n)


def clean_stage(vertices, vcolors, triangles, min_faces=20000):
    """-> the `clean_*` rows of the result: label + emit on the extracted mesh, and scipy on the host next to it."""
    if triangles.shape[0] == 0:
        return {"clean_ms": None}
    clean_mesh(vertices, triangles, vcolors, min_faces)  # warm-up of the shape
    torch.cuda.synchronize()
    t = time.perf_counter()
    cv, _, ct, info = clean_mesh(vertices, triangles, vcolors, min_faces, return_info=True)
    torch.cuda.synchronize()
    row = {"clean_ms": round((time.perf_counter() - t) * 1e3, 3), "clean_min_component_faces": min_faces,
           "clean_rows": [int(cv.shape[0]), int(ct.shape[0])], "clean_info": info}
    host = scipy_components_ms(triangles.cpu().numpy(), int(vertices.shape[0]))
    if host is not None:
        # (scipy sees every face: null and duplicate faces are not removed first, so its count can differ)
        row["clean_scipy_components_ms"], row["clean_scipy_components"] = host
    return row


def eval_stage(vertices, triangles, shift):
    """-> the `eval_*` rows of the result: BVH build and one query of the surface-distance evaluation."""
    if triangles.shape[0] == 0:
        return {"eval_build_ms": None}
    points = (vertices + torch.tensor([shift, 0.0, 0.0], device=vertices.device)).contiguous()
    MeshDistance(vertices, triangles).query(points)  # warm-up of the shapes
    torch.cuda.synchronize()
    t = time.perf_counter()
    mesh = MeshDistance(vertices, triangles)
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t) * 1e3
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    dist, _ = mesh.query(points)
    e1.record()
    torch.cuda.synchronize()
    s = mesh.stats(dist)
    return {"eval_build_ms": round(build_ms, 3), "eval_query_ms": round(e0.elapsed_time(e1), 3),
            "eval_rows": [int(triangles.shape[0]), int(points.shape[0])], "eval_mean": s["mean"], "eval_max": s["max"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-ops integration (profiling runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fusion_bench: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    cams = [S.make_camera(a.width, a.height, yaw=0.004 * k - 0.2, pitch=0.05 * np.sin(0.3 * k),
                          trans=(0.3 * np.sin(0.2 * k), 0.0, 0.0)) for k in range(a.views)]
    sc = S.make_scene(a.gaussians, S.make_camera(a.width, a.height), sh_degree=3, seed=42, scale_lo=0.0025,
                      scale_hi=0.025)
    p = {k: torch.from_numpy(v).to(dev) for k, v in sc.items()}
    # (the cloud is translucent, opacities U(0.1, 0.9): depth is the alpha-weighted mean of what a pixel composites)
    bg = torch.tensor(S.BACKGROUND, device=dev)
    L, trunc = 6.0 / 512, 0.06
    vol = TSDFVolume(L, trunc, (-3.0, -3.0, 3.0), (64, 64, 64), 64 ** 3, dev)
    pool2 = None if a.no_torch else (torch.zeros_like(vol.tsdf), torch.zeros_like(vol.weight), torch.zeros_like(vol.color))
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    rows = []
    s = _stream(dev)
    for k, cam in enumerate(cams):
        e = [ev() for _ in range(6)]
        with torch.no_grad():
            e[0].record()
            out = render_view(p["means3d"], p["scales"], p["quats"], p["opacities"], p["sh_coeffs"],
                              CameraTensors.from_numpy(cam, dev), bg, 3, render_depth=True, fused_depth=True,
                              normalise_depth=False)
            depth, valid = view_depth(out["depth_acc"], out["alpha"], 0.5)
            rgb = out["rgb"].contiguous()
            e[1].record()
        w_before = float(vol.weight[:vol.num_allocated_blocks].sum(dtype=torch.float64))
        desc = vol._desc()
        view = vol._view_desc(depth, rgb, cam.fx, cam.fy, cam.cx, cam.cy, cam.viewmat, valid.data_ptr(), 10.0)
        e[2].record()
        vol._touch_allocate(desc, view, s)
        e[3].record()
        vol._integrate_listed(desc, view, s)
        e[4].record()
        torch.cuda.synchronize()
        n_list = int(vol._state[ST_LIST].item())
        updated = float(vol.weight[:vol.num_allocated_blocks].sum(dtype=torch.float64)) - w_before
        row = {"render_ms": e[0].elapsed_time(e[1]), "touch_allocate_ms": e[2].elapsed_time(e[3]),
               "integrate_ms": e[3].elapsed_time(e[4]), "blocks": n_list, "updated_voxels": updated}
        row["integrate_bytes"] = 40.0 * updated + 8.0 * (512.0 * n_list - updated)
        if pool2 is not None:
            blocks = (vol._list[:n_list] & ((1 << 30) - 1)).long()
            t0, t1 = ev(), ev()
            t0.record()
            torch_integrate(vol, pool2, blocks, depth, rgb, valid, cam, 10.0)
            t1.record()
            torch.cuda.synchronize()
            row["torch_integrate_ms"] = t0.elapsed_time(t1)
        rows.append(row)
    timed = rows[a.warmup:]
    med = lambda key: statistics.median(r[key] for r in timed)  # noqa: E731
    res = {"metric": "TSDF fusion, per-view medians (device events)", "views": a.views, "warmup_views": a.warmup,
           "gaussians": a.gaussians, "resolution": f"{a.width}x{a.height}", "voxel_length": L, "sdf_trunc": trunc,
           "volume_blocks": list(vol.blocks), "allocated_blocks": vol.num_allocated_blocks,
           "render_ms": round(med("render_ms"), 4), "touch_allocate_ms": round(med("touch_allocate_ms"), 4),
           "integrate_ms": round(med("integrate_ms"), 4), "blocks_per_view": med("blocks"),
           "updated_voxels_per_view": med("updated_voxels"), "integrate_bytes_per_view": med("integrate_bytes")}
    rate = statistics.median(r["integrate_bytes"] / (r["integrate_ms"] * 1e-3) for r in timed)
    res["integrate_bytes_per_s"] = rate
    res["integrate_fraction_of_hbm_peak"] = round(rate / HBM_PEAK, 4)
    if pool2 is not None:
        res["torch_integrate_ms"] = round(med("torch_integrate_ms"), 4)
        res["torch_over_hip"] = round(res["torch_integrate_ms"] / res["integrate_ms"], 2)
        n = vol.num_allocated_blocks
        res["torch_matches_hip"] = bool(torch.equal(pool2[1][:n], vol.weight[:n]) and
                                        float((pool2[0][:n] - vol.tsdf[:n]).abs().max()) < 1e-5)
    for name, fn in (("extract_points_ms", vol.extract_point_cloud), ("extract_mesh_ms", vol.extract_mesh)):
        fn()  # warm-up of the shape
        torch.cuda.synchronize()
        t = time.perf_counter()
        got = fn()
        torch.cuda.synchronize()
        res[name] = round((time.perf_counter() - t) * 1e3, 3)
        res[name.replace("_ms", "_rows")] = [int(x.shape[0]) for x in got]
    res.update(clean_stage(*got))
    res.update(eval_stage(got[0], got[2], 0.5 * L))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
