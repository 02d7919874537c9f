"""CPU: bench.py's option surface and the rule by which --dump-outputs samples what a step computed."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_full_and_dump_outputs_are_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in out.stdout, opt


def _step(n, h, w, depth=False):
    g = torch.Generator().manual_seed(0)
    params = {k: torch.zeros(n, *s, requires_grad=True)
              for k, s in (("means3d", (3,)), ("scales", (3,)), ("quats", (4,)), ("opacities", (1,)), ("sh_coeffs", (16, 3)))}
    for p in params.values():
        p.grad = torch.randn(p.shape, generator=g)
    out = {"rgb": torch.rand(h, w, 3, generator=g), "alpha": torch.rand(h, w, 1, generator=g),
           "depth": torch.rand(h, w, 1, generator=g) if depth else None, "xys": torch.rand(n, 2, generator=g),
           "radii": torch.randint(0, 9, (n,), dtype=torch.int32, generator=g), "depths": torch.rand(n, generator=g),
           "conics": torch.rand(n, 3, generator=g), "num_tiles_hit": torch.randint(0, 9, (n,), dtype=torch.int32, generator=g),
           "rgbs": torch.rand(n, 3, generator=g)}
    return out, params


def test_dump_keeps_small_outputs_whole():
    import bench

    out, params = _step(5000, 36, 64)
    r = bench.outputs_of_step(out, params, 36 * 64)
    assert np.array_equal(r["rgb"], out["rgb"].numpy()) and r["alpha"].shape == (36, 64, 1) and "depth" not in r
    assert np.array_equal(r["grad_sh_coeffs"], params["sh_coeffs"].grad.numpy())
    assert np.array_equal(r["radii"], out["radii"].numpy().astype(np.float32))
    assert all(a.dtype == np.float32 for a in r.values())


def test_dump_samples_large_outputs_the_same_way_every_time(tmp_path):
    import bench

    n, h, w = 1_000_000, 2160, 3840
    out, params = _step(n, h, w, depth=True)
    a = bench.outputs_of_step(out, params, h * w)
    b = bench.outputs_of_step(out, params, h * w)
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert a["grad_means3d"].shape == (bench.DUMP_GAUSSIANS, 3) and a["rgb"].shape == (bench.DUMP_PIXELS, 3)
    assert a["depth"].shape == (bench.DUMP_PIXELS, 1)
    assert sum(x.nbytes for x in a.values()) <= 64_000_000
    bench.write_outputs(str(tmp_path), a)
    assert sorted(f[:-4] for f in os.listdir(tmp_path)) == sorted(a)
    assert np.array_equal(np.load(tmp_path / "rgb.npy"), a["rgb"])
