"""Tile lists built ahead for a caller that never blocks but runs this package's SH forward between
`project_gaussians` and `rasterize_gaussians` (rasterizer/ahead.py, "WHEN"): the lists are built on the side stream
beside the SH kernel, and nothing the caller sees changes -- lists, image, alpha to the last bit, gradients within
the spread of float atomics -- against the same views in a process of its own with GSR_SPECULATE=0.

Run as a script (`python tests/test_gpu_lists_beside_sh.py OUT.npz`) this file is that process."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    for _p in (ROOT, os.path.join(ROOT, "gaussian-splatting-toolkit_amd")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import pytest  # noqa: E402
import torch  # noqa: E402

from harness import scene as S  # noqa: E402
from harness.pipeline import CameraTensors  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, WIDTH, HEIGHT = 20_000, 320, 180
YAWS = (0.0, 0.05, -0.05, 0.1, -0.1, 0.02)
# the three parts, one view per entry: (colours, opacity)
PLAN = [("sh", "sigmoid")] * 6 + [("torch", "sigmoid")] * 4 + [("sh", "sigmoid")] * 3 + [("sh", "other")] \
    + [("sh", "sigmoid")] * 3
PART_A, PART_B, PART_C = range(0, 6), range(6, 10), range(10, 17)
OTHER_VIEW = 13


def run_views():
    """Every view of PLAN -> per view: lists, image, alpha, gradients (numpy) and the counters after it."""
    from rasterizer import ahead as A
    from rasterizer import project_gaussians, rasterize_gaussians, spherical_harmonics
    from rasterizer import rasterize as R
    from rasterizer.cuda import _tuning

    saved_rows = _tuning.overrides()
    _tuning.set_overrides(dict(saved_rows, speculate_min=1000))
    dev = torch.device(DEV)
    cams = [S.make_camera(WIDTH, HEIGHT, yaw=y) for y in YAWS]
    sc = S.make_scene(N, cams[0], sh_degree=3, seed=31, scale_lo=0.004, scale_hi=0.04)
    t = lambda a, g=False: torch.from_numpy(a).to(dev).requires_grad_(g)  # noqa: E731
    means, scales, quats, coeffs = t(sc["means3d"], True), t(sc["scales"]), t(sc["quats"]), t(sc["sh_coeffs"], True)
    logits = torch.logit(t(sc["opacities"]).clamp(1e-3, 1 - 1e-3)).requires_grad_(True)
    plain = torch.rand(N, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(3)).requires_grad_(True)
    bg = torch.tensor(S.BACKGROUND, device=dev)
    # a caller that never blocks keeps its stream busy: this one queues ~1 ms of its own work in front of each view, so
    # that the stream is not idle when `rasterize_gaussians` is entered (the OTHER signal of "auto")
    filler = torch.rand(4096, 4096, device=dev)
    st = A._spec.setdefault(dev, {"stream": None, "recipe": None, "entry": None})
    st["idle"] = 0.0
    # (a test before this one may have handed in opacities no recipe explains until the detection switched itself off)
    st["recipes_off"], st["unknown_run"] = False, 0
    views = []
    try:
        for i, (colours, opacity) in enumerate(PLAN):
            cam = cams[i % len(cams)]
            ct = CameraTensors.from_numpy(cam, DEV)
            (filler @ filler) @ filler
            xys, depths, radii, conics, _comp, num_tiles_hit, _cov = project_gaussians(
                means, scales, 1.0, quats, ct.viewmat[:3], ct.projmat, cam.fx, cam.fy, cam.cx, cam.cy, HEIGHT, WIDTH, 16)
            if colours == "sh":
                dirs = means.detach() - ct.campos
                dirs = dirs / dirs.norm(dim=-1, keepdim=True)
                rgbs = torch.clamp(spherical_harmonics(3, dirs, coeffs) + 0.5, min=0.0)
                colour_leaf = coeffs
            else:
                rgbs = torch.clamp(plain + 0.0, min=0.0)
                colour_leaf = plain
            op = torch.sigmoid(logits) if opacity == "sigmoid" else (torch.sigmoid(logits) * 0.5).detach()
            img, alpha = rasterize_gaussians(xys, depths, radii, conics, num_tiles_hit, rgbs, op, HEIGHT, WIDTH, 16,
                                             background=bg, return_alpha=True)
            del op
            loss = (img * img).sum() + alpha.sum()
            g_means, g_colour = torch.autograd.grad(loss, (means, colour_leaf))
            torch.cuda.synchronize()
            lists = R._cache_snapshot()["value"]
            count = int(lists.num_intersects)
            views.append({"ids": lists.ids[:count].cpu().numpy(), "bins": lists.bins.cpu().numpy(),
                          "img": img.detach().cpu().numpy(), "alpha": alpha.detach().cpu().numpy(),
                          "g_means": g_means.cpu().numpy(), "g_colour": g_colour.cpu().numpy(),
                          "counters": dict(R.counters), "idle": st.get("idle")})
    finally:
        _tuning.set_overrides(saved_rows)
    return views


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """-> (the views in this process under "auto", the same views of a fresh process under GSR_SPECULATE=0)"""
    import subprocess

    from rasterizer import rasterize as R

    out = str(tmp_path_factory.mktemp("beside_sh") / "off.npz")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), out], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, GSR_SPECULATE="0"), cwd=ROOT)
    assert child.returncode == 0, child.stdout[-2000:] + child.stderr[-2000:]
    off = np.load(out)
    R._speculation_mode()
    saved = R._spec_knobs["mode"]
    R._spec_knobs["mode"] = "auto"
    try:
        start = dict(R.counters)
        views = run_views()
    finally:
        R._spec_knobs["mode"] = saved
    return start, views, off


def _delta(views, start, i, name):
    before = start if i == 0 else views[i - 1]["counters"]
    return views[i]["counters"][name] - before[name]


def _same_results(views, off, i):
    v = views[i]
    for name in ("ids", "bins", "img", "alpha"):
        assert np.array_equal(v[name], off[f"{name}_{i}"]), (i, name)
    for name in ("g_means", "g_colour"):
        ref = off[f"{name}_{i}"]
        diff, top = np.abs(v[name] - ref).max(), np.abs(ref).max()
        print(f"view {i} {name}: largest difference {diff:.3e}, largest value {top:.3e}")
        assert diff <= 1e-5 * top, (i, name, diff, top)


def test_child_built_nothing_ahead(both):
    _, _, off = both
    assert int(off["list_builds_ahead"]) == 0 and int(off["ahead_hits"]) == 0


def test_lists_are_built_beside_our_sh_for_a_caller_that_never_blocks(both):
    start, views, off = both
    for i in PART_A:
        print(f"view {i}: idle average {views[i]['idle']:.3f}")
        moved = {k: _delta(views, start, i, k) for k in views[i]["counters"] if _delta(views, start, i, k)}
        print(f"view {i}: counters moved {moved}")
        if i >= 1:
            assert _delta(views, start, i, "list_builds_ahead") == 1 and _delta(views, start, i, "ahead_hits") == 1, (i, moved)
        assert _delta(views, start, i, "ahead_misses") == 0, (i, moved)
        _same_results(views, off, i)
    # it was the SH signal, not an idle stream, that switched the lists on
    assert views[PART_A[-1]]["idle"] <= 0.5, [v["idle"] for v in views]


def test_torch_colours_build_nothing_ahead(both):
    """The signal is the PREVIOUS view's: the first view behind part (a) still has its lists built; no later one."""
    start, views, off = both
    for i in PART_B:
        if i > PART_B[0]:
            assert _delta(views, start, i, "list_builds_ahead") == 0 and _delta(views, start, i, "ahead_hits") == 0, i
        _same_results(views, off, i)
    assert views[PART_B[-1]]["idle"] <= 0.5


def test_another_opacity_is_a_miss_and_the_views_behind_it_recover(both):
    """View OTHER_VIEW receives a tensor nobody announced: its lists were built for `sigmoid(logits)` and are dropped.
    The next view's recipe is "the tensor handed in last time", which predicts nothing of use (a depth order alone, or
    lists that are dropped again: whichever, its results are right); the views behind it have their lists built ahead
    and use them."""
    start, views, off = both
    for i in PART_C:
        _same_results(views, off, i)
    assert _delta(views, start, OTHER_VIEW - 1, "ahead_hits") == 1
    assert _delta(views, start, OTHER_VIEW, "ahead_misses") == 1 and _delta(views, start, OTHER_VIEW, "ahead_hits") == 0
    for i in (OTHER_VIEW + 2, OTHER_VIEW + 3):
        assert _delta(views, start, i, "ahead_hits") == 1 and _delta(views, start, i, "ahead_misses") == 0, i


if __name__ == "__main__":
    from rasterizer import rasterize as _R

    _views = run_views()
    _arrays = {f"{k}_{i}": v[k] for i, v in enumerate(_views) for k in ("ids", "bins", "img", "alpha", "g_means", "g_colour")}
    np.savez(sys.argv[1], list_builds_ahead=_R.counters["list_builds_ahead"], ahead_hits=_R.counters["ahead_hits"],
             **_arrays)
