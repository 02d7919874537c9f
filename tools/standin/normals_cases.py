"""Case files for tools/standin/normals_main.cpp: the shapes of tests/test_gpu_normals.py that a host run can afford,
with what the float64 restatement (tests/_normals_ref.py) returns for them and the error of the same restatement in
float32 (the tolerance's baseline).
    python tools/standin/normals_cases.py DIR"""
import os
import sys

import numpy as np
import torch

OUT = sys.argv[1]
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import _normals_ref as R

f32 = lambda a: a.numpy().astype(np.float32).tobytes()  # noqa: E731
f64 = lambda a: a.numpy().astype(np.float64).tobytes()  # noqa: E731
u8 = lambda a: a.numpy().astype(np.uint8).tobytes()  # noqa: E731


def put_image(name, H, W, seed, masked):
    """header int32 [4]: 0, H, W, masked; float64 [4]: fx, fy, cx, cy; float32: depth, alpha, normals_img, (mask);
    float64: normals, loss, v_normals_img, v_depth (upstream 1); float64 [4]: their e of the float32 restatement;
    uint8: valid, near_valid."""
    case = R.image_case(H, W, seed, masked)
    want = R.image_reference(case)
    with open(os.path.join(OUT, f"{name}.bin"), "wb") as f:
        f.write(np.array([0, H, W, int(masked)], np.int32).tobytes())
        f.write(np.array(case["K"], np.float64).tobytes())
        for a in (case["depth"], case["alpha"], case["nimg"]) + ((case["mask"],) if masked else ()):
            f.write(f32(a))
        keys = ("normals", "loss", "v_nimg", "v_depth")
        for k in keys:
            f.write(f64(want[k]))
        f.write(np.array([want["e32"][k] for k in keys], np.float64).tobytes())
        f.write(u8(want["valid"]) + u8(want["near_valid"]))


def put_gaussians(name, n, seed):
    """header int32 [4]: 1, N, 0, 0; float32: quats, scales, means, viewmat [12], v_normals; int32: axis; float64:
    normals, v_quats; float64 [2]: their e of the float32 restatement."""
    case, _ = R.gaussian_case(n, seed)
    want = R.gaussian_reference(case, seed + 1)
    with open(os.path.join(OUT, f"{name}.bin"), "wb") as f:
        f.write(np.array([1, n, 0, 0], np.int32).tobytes())
        for a in (case["quats"], case["scales"], case["means"], case["viewmat"], want["v_normals"]):
            f.write(f32(a))
        f.write(want["axis"].numpy().astype(np.int32).tobytes())
        f.write(f64(want["normals"]) + f64(want["v_quats"]))
        f.write(np.array([want["e32"]["normals"], want["e32"]["v_quats"]], np.float64).tobytes())


for i, (H, W) in enumerate(((1, 1), (2, 2), (3, 3), (5, 7), (17, 33), (64, 64))):
    put_image(f"img{i}_{H}x{W}", H, W, 100 + i, False)
    put_image(f"img{i}_{H}x{W}_masked", H, W, 100 + i, True)
for n in (1, 63, 64, 65, 1000):
    put_gaussians(f"gauss_{n}", n, 200 + n)
print(len(os.listdir(OUT)), "case files")
