"""Device time of the projection's pose pass (camera gradients) next to `project_bwd_kernel`.

    python tools/pose_grad_bench.py [--sizes 200000 1000000 3000000] [--repeats 20] [--launches 20]

For every size: a seeded cloud in front of a 1920x1080 camera is projected once; then `gsr_project_backward` (the
per-Gaussian backward, one launch) and `gsr_project_backward_pose` (two launches: per-workgroup float64 partials, then
the one-workgroup final sum) are timed alternately -- `--repeats` windows of `--launches` back-to-back calls each,
device events around a window, after a warm-up of both; outputs and the workspace are allocated outside the windows.
Reported per call: the median window / launches, and the spread (min, max) over the windows.  Bytes per Gaussian are
what the algorithm needs, from the shapes: the pose pass reads means3d 12, radii 4, conics 12, compensation 4, cov3d
24 and the cotangents 8 + 4 + 12 + 4 = 84 B (visible or not: a culled Gaussian costs its radius alone, counted in
full), and writes 192 B per 1024 Gaussians; the backward reads the same plus scales 12 and quats 16 and writes
19 floats = 188 B.  The fraction of the 8 TB/s HBM peak is those bytes over the measured time.  One JSON line per
size; needs a GPU."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gaussian-splatting-toolkit_amd")]
import numpy as np

HBM_PEAK = 8.0e12  # bytes / s
POSE_BYTES = 84.0 + 192.0 / 1024.0
BWD_BYTES = 84.0 + 28.0 + 76.0


def bench(n, repeats, launches, device):
    import torch

    import rasterizer.cuda as RC
    from harness import scene as S
    from rasterizer.cuda._backend import lib

    if not torch.cuda.is_available():
        raise SystemExit("pose_grad_bench: no GPU")
    cam = S.make_camera(1920, 1080)
    sc = S.make_scene(n, cam, sh_degree=0, seed=7)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    means, scales, quats = t(sc["means3d"]), t(sc["scales"]), t(sc["quats"])
    viewmat, projmat = t(cam.viewmat[:3]), t(cam.projmat)
    cov3d, xys, depths, radii, conics, comp, tiles = RC.project_gaussians_forward(
        n, means, scales, 1.0, quats, viewmat, projmat, cam.fx, cam.fy, cam.cx, cam.cy, cam.height, cam.width, 16, 0.01)
    g = torch.Generator(device=device).manual_seed(5)
    cot = [torch.randn(s, device=device, generator=g) for s in ((n, 2), (n,), (n, 3), (n,))]
    L = lib()
    ws_bytes = int(L.gsr_project_backward_pose_workspace(C.c_int(n)))
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=device)
    vv, vp = torch.empty(12, device=device), torch.empty(16, device=device)
    outs = [torch.empty((n, k), device=device) for k in (3, 6, 3, 3, 4)]
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    f = C.c_float
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def pose():
        rc = L.gsr_project_backward_pose(C.c_int(n), p(means), p(viewmat), p(projmat), f(cam.fx), f(cam.fy),
                                         C.c_uint(cam.height), C.c_uint(cam.width), p(cov3d), p(radii), p(conics),
                                         p(comp), *(p(c) for c in cot), p(ws), C.c_size_t(ws_bytes), p(vv), p(vp), stream)
        assert rc == 0, L.gsr_last_error()

    def backward():
        rc = L.gsr_project_backward(C.c_int(n), p(means), p(scales), f(1.0), p(quats), p(viewmat), p(projmat), f(cam.fx),
                                    f(cam.fy), f(cam.cx), f(cam.cy), C.c_uint(cam.height), C.c_uint(cam.width), p(cov3d),
                                    p(radii), p(conics), p(comp), *(p(c) for c in cot), *(p(o) for o in outs), stream)
        assert rc == 0, L.gsr_last_error()

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / launches  # us per call

    for fn in (pose, backward):  # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {"pose": [], "backward": []}
    for _ in range(repeats):  # alternating: both see the same machine
        times["pose"].append(window(pose))
        times["backward"].append(window(backward))
    row = {"n": n, "visible": float((radii > 0).float().mean()), "launches_per_window": launches, "windows": repeats}
    for k, nbytes in (("pose", POSE_BYTES), ("backward", BWD_BYTES)):
        med = float(np.median(times[k]))
        row[k] = {"us_median": round(med, 2), "us_min": round(min(times[k]), 2), "us_max": round(max(times[k]), 2),
                  "bytes_per_gaussian": round(nbytes, 2), "gb_per_s": round(nbytes * n / med / 1e3, 1),
                  "fraction_of_hbm_peak": round(nbytes * n / (med * 1e-6) / HBM_PEAK, 4)}
    row["pose_over_backward"] = round(row["pose"]["us_median"] / row["backward"]["us_median"], 3)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[200_000, 1_000_000, 3_000_000])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    for n in a.sizes:
        print(json.dumps(bench(n, a.repeats, a.launches, a.device)), flush=True)


if __name__ == "__main__":
    main()
