"""CPU: the host side of the antialiased rasterize mode -- the descriptor's two new fields, the defaults of every
switch, and the trainer on the oracle-backed stand-ins (tests/cpu_standins.py, wired as tools/train_trajectory.py
wires them)."""
import json
import os
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_view_descriptor_mirror_matches_the_header(tmp_path):
    """`antialiased` and `opac_aa` are the LAST two fields of gsr_view_desc; every older field keeps its offset (the
    C compiler's, as tests/test_capi_and_host.py compares them)."""
    import ctypes as C

    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    from gs_fused.render import _ViewDesc

    names = [f for f, _ in _ViewDesc._fields_]
    assert names[-2:] == ["antialiased", "opac_aa"] and names[-3] == "seg_ws_bytes"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gsraster.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(gsr_view_desc));']
    lines += [f'  printf("{f} %zu\\n", offsetof(gsr_view_desc, {f}));' for f in names]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    want = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(want["size"]) == C.sizeof(_ViewDesc)
    for f in names:
        assert int(want[f]) == getattr(_ViewDesc, f).offset, f
    assert _ViewDesc.antialiased.offset == _ViewDesc.seg_ws_bytes.offset + C.sizeof(C.c_size_t)


def test_the_two_entries_are_declared_and_exported():
    from rasterizer.cuda import _backend

    src = open(os.path.join(ROOT, "include", "gsraster.h")).read()
    for s in ("gsr_project_forward_aa", "gsr_project_backward_aa"):
        assert s + "(" in src and s in _backend.SYMBOLS and hasattr(_backend.lib(), s)
    assert _backend.lib().gsr_version() == 200


def test_every_switch_defaults_to_classic():
    import inspect

    from gs_fused import ViewSpec
    from gs_fusion import fuse_views
    from harness.train import TrainConfig
    from rasterizer.inria import GaussianRasterizationSettings

    spec = ViewSpec(48, 64, 50.0, 50.0, 32.0, 24.0, 1)
    assert spec.rasterize_mode == "classic" and not spec.antialiased
    assert ViewSpec(48, 64, 50.0, 50.0, 32.0, 24.0, 1, rasterize_mode="antialiased").antialiased
    assert spec != ViewSpec(48, 64, 50.0, 50.0, 32.0, 24.0, 1, rasterize_mode="antialiased")  # (a graph's key)
    with pytest.raises(ValueError, match="Unknown rasterize_mode: smooth"):
        ViewSpec(48, 64, 50.0, 50.0, 32.0, 24.0, 1, rasterize_mode="smooth")
    assert TrainConfig().rasterize_mode == "classic"
    assert inspect.signature(fuse_views).parameters["rasterize_mode"].default == "classic"
    # the older tuple, positionally: twelve fields, then the new one with its default
    eye = torch.eye(4)
    old = GaussianRasterizationSettings(48, 64, 0.5, 0.4, torch.zeros(3), 1.0, eye, eye, 3, torch.zeros(3), False, False)
    assert old.antialiasing is False and old.debug is False and old._fields[-1] == "antialiasing"
    short = GaussianRasterizationSettings(48, 64, 0.5, 0.4, torch.zeros(3), 1.0, eye, eye, 3, torch.zeros(3))
    assert len(short) == len(old) == 13 and short[10:] == (False, False, False)
    assert GaussianRasterizationSettings(*old[:12], True).antialiasing is True


def test_an_unknown_mode_is_refused_by_the_trainer():
    from harness.train import TrainConfig, train

    with pytest.raises(ValueError, match="Unknown rasterize_mode"):
        train(TrainConfig(rasterize_mode="smooth", num_gaussians=100, iters=1), torch.device("cpu"))


BASE = dict(num_gaussians=600, init_gaussians=200, width=64, height=48, num_views=4, eval_views=2, sh_degree=1,
            sh_degree_interval=10, scene_scale=(0.03, 0.15), log_every=1, iters=10)  # tools/train_trajectory.py's BASE


@pytest.fixture(scope="module")
def cpu_runs():
    """Three 10-step runs on the stand-ins: the default, "classic" spelled out, "antialiased"."""
    import sys

    sys.path[:0] = [p for p in (os.path.join(ROOT, "tools"),) if p not in sys.path]
    import cpu_standins as SI
    import harness.pipeline as HP
    import harness.train as HT
    from oracle import oracle as O
    from train_trajectory import TIMING, _hex

    torch.set_num_threads(2)
    O.set_threads(2)
    saved = HP.project_gaussians, HP.spherical_harmonics, HP.rasterize_gaussians
    HP.project_gaussians, HP.spherical_harmonics, HP.rasterize_gaussians = (
        SI.project_gaussians, SI.spherical_harmonics, SI.rasterize_gaussians)
    try:
        res = {k: HT.train(HT.TrainConfig(**BASE, **kw), torch.device("cpu"))
               for k, kw in (("default", {}), ("classic", dict(rasterize_mode="classic")),
                             ("antialiased", dict(rasterize_mode="antialiased")))}
    finally:
        HP.project_gaussians, HP.spherical_harmonics, HP.rasterize_gaussians = saved
    line = lambda r: json.dumps({k: _hex(v) for k, v in r.items()  # noqa: E731  (what the tool prints for a case)
                                 if k not in TIMING and not k.startswith("phase_")})
    return res, {k: line(r) for k, r in res.items()}


def test_classic_spelled_out_prints_the_defaults_bytes(cpu_runs):
    res, lines = cpu_runs
    assert lines["classic"] == lines["default"] and "rasterize_mode" not in res["default"]


def test_antialiased_training_differs_from_the_first_loss_on(cpu_runs):
    res, lines = cpu_runs
    a, c = res["antialiased"], res["classic"]
    assert a["rasterize_mode"] == "antialiased" and len(a["losses"]) == len(c["losses"]) == 10
    assert all(x != y for x, y in zip(a["losses"], c["losses"]))
    assert a["psnr_start"] != c["psnr_start"] and a["param_checksum"] != c["param_checksum"]
    assert all(torch.isfinite(torch.tensor(a["losses"])))
