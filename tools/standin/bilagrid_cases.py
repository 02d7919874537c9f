"""Case files for tools/standin/bilagrid_main.cpp: the shapes of tests/test_gpu_bilagrid.py that a host run can afford,
with what the float64 restatement (tests/_bilagrid_ref.py) returns for them and the error of the same restatement in
float32 (the tolerance's baseline).
    python tools/standin/bilagrid_cases.py DIR"""
import os
import sys

import numpy as np
import torch

OUT = sys.argv[1]
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import _bilagrid_ref as B


def put(name, H, W, gw, gh, gl, view, V=3):
    """header int32 [7]: H, W, V, view, Gw, Gh, L; float32: grids, rgb, v_out; float64: out, v_rgb, v_grids, tv,
    v_tv (upstream 1); float64 [5]: e(out), e(v_rgb), e(v_grids), e(tv), e(v_tv) of the float32 restatement."""
    (grids, rgb, v_out), want, base = B.slice_case(H, W, gw, gh, gl, view, V)
    tv = []
    for dt in (torch.float64, torch.float32):
        a = grids.to(dt).clone().requires_grad_(True)
        t = B.tv_ref(a)
        t.backward()
        tv.append((t.detach().reshape(1), a.grad))
    e32 = [B.rel_err(b, w) for b, w in zip(base + tv[1], want + tv[0])]
    with open(os.path.join(OUT, f"{name}.bin"), "wb") as f:
        f.write(np.array([H, W, V, view, gw, gh, gl], np.int32).tobytes())
        for a in (grids, rgb, v_out):
            f.write(a.numpy().astype(np.float32).tobytes())
        for a in want + tv[0]:
            f.write(a.numpy().astype(np.float64).tobytes())
        f.write(np.array(e32, np.float64).tobytes())


put("0_1x1_g2", 1, 1, 2, 2, 2, 0)
put("0_1x1_g16", 1, 1, 16, 16, 8, 2)
put("1_5x7_g2", 5, 7, 2, 2, 2, 1)
put("1_5x7_g325", 5, 7, 3, 2, 5, 2)
put("1_5x7_g16", 5, 7, 16, 16, 8, 0)
put("2_37x53_g325", 37, 53, 3, 2, 5, 0)
put("2_37x53_g16", 37, 53, 16, 16, 8, 1)
put("3_64x64_g2", 64, 64, 2, 2, 2, 2)
put("3_20x33_g64", 20, 33, 64, 64, 16, 1)
print(len(os.listdir(OUT)), "case files")
