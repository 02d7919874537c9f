"""Host: the float32 restatement of the target kernels (tests/target_reference.py) against the torch CPU path the
trainer has used so far -- `downscale_image` / `downscale_depth` / `composite_with_background` of harness.train fed
`u8.float() / 255` -- on the shapes of tests/test_gpu_target.py.

Tolerance.  The restatement and torch may order the three lerps and the composite differently: at most 8 roundings on
values in [0,1], 8 * 2^-24.  Their float32 source coordinates may differ by one rounding of `scale * (dst + 0.5)`: at
most max(H,W) * 2^-22, times a tap difference of at most 1.  So tol = 2^-21 + max(H,W) * 2^-22, for planes relative to
the largest tap.  Without a resize (d = 1) and without alpha both sides are `u8 / 255` and are held equal.

Also: the float32 restatement against the same rule in float64 (the restatement's own error), and `print_largest`
(python tests/test_target_host.py) prints the largest difference per case for DESIGN.md section 4.15."""
import numpy as np
import pytest
import torch

import target_reference as R
from harness.train import composite_with_background, downscale_depth, downscale_image

BG = np.array([0.0, 1.0, 0.3], np.float32)
SHAPES = [((37, 23), d) for d in (1, 2, 3, 4)] + [((23, 37), d) for d in (1, 2, 3, 4)] \
    + [((64, 48), d) for d in (2, 4, 8)] + [((48, 64), d) for d in (2, 4, 8)] \
    + [((1, 7), 1), ((7, 1), 1), ((2, 2), 2), ((3, 257), 2), ((257, 3), 2)]
IDS = [f"{hw[0]}x{hw[1]}-d{d}" for hw, d in SHAPES]


def tolerance(H: int, W: int) -> float:
    return 2.0 ** -21 + max(H, W) * 2.0 ** -22


def _images(H, W, C, rng):
    ramp = (np.arange(H * W * C) % 256).astype(np.uint8).reshape(H, W, C)
    rnd = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    out = {"ramp": ramp, "random": rnd}
    if C == 4:
        binary = rnd.copy()
        binary[..., 3] = rng.integers(0, 2, (H, W), dtype=np.uint8) * 255
        out["alpha_binary"] = binary
    return out


def _planes(H, W, rng):
    depth = rng.integers(0, 65536, (H, W)).astype(np.uint16)
    depth.reshape(-1)[:3] = (0, 1, 65535)
    return {"depth_u16": (depth, 1e-3), "mask_u8": (rng.integers(0, 2, (H, W)).astype(np.uint8), 1.0),
            "mono_u8": (rng.integers(0, 256, (H, W)).astype(np.uint8), 1.0 / 255.0)}


def torch_target(img: np.ndarray, d: int) -> np.ndarray:
    v = torch.from_numpy(img).float() / 255.0
    return composite_with_background(downscale_image(v, d), torch.from_numpy(BG)).numpy()


def torch_plane(p: np.ndarray, unit: float, d: int) -> np.ndarray:
    v = torch.from_numpy(p.astype(np.float32)) * torch.tensor(unit, dtype=torch.float32)
    return downscale_depth(v, d).numpy()


def differences():
    """(what, H, W, d, largest |restatement - torch|, tolerance in the same units) for every case."""
    rows = []
    for (H, W), d in SHAPES:
        rng = np.random.default_rng(1000 * H + W)
        hw = (H // d, W // d)
        for C in (3, 4):
            for name, img in _images(H, W, C, rng).items():
                diff = np.abs(R.target_from_u8(img, BG, hw).astype(np.float64) - torch_target(img, d)).max()
                rows.append((f"rgb{'a' if C == 4 else ''}:{name}", H, W, d, float(diff), tolerance(H, W)))
        for name, (p, unit) in _planes(H, W, rng).items():
            diff = np.abs(R.plane_from_int(p, unit, hw).astype(np.float64) - torch_plane(p, unit, d)).max()
            top = float(np.float32(p.max()) * np.float32(unit))
            rows.append((f"plane:{name}", H, W, d, float(diff), tolerance(H, W) * max(top, 2.0 ** -126)))
    return rows


_ROWS = None


def _rows():
    global _ROWS
    if _ROWS is None:
        _ROWS = differences()  # computed once, shared
    return _ROWS


def test_restatement_matches_torch_path():
    worst = 0.0
    for what, H, W, d, diff, tol in _rows():
        assert diff <= tol, f"{what} {H}x{W} d={d}: {diff} > {tol}"
        worst = max(worst, diff / tol)
    print(f"largest difference / tolerance: {worst:.3f}")


def test_no_resize_no_alpha_is_exact():
    for what, H, W, d, diff, _ in _rows():
        if d == 1 and (what.startswith("rgb:") or what.startswith("plane:")):
            assert diff == 0.0, f"{what} {H}x{W}"


@pytest.mark.parametrize("hw,d", SHAPES, ids=IDS)
def test_float32_restatement_against_float64(hw, d):
    """The restatement's own error: conversion 1 rounding, the weights 2, the lerps 7, the composite 4 -- 14 * 2^-24
    on values in [0,1] -- plus the two source coordinates, each off by at most max(H,W) * 2^-23 (the scale's rounding
    and the product's) times a tap difference of at most 1."""
    H, W = hw
    out_hw = (H // d, W // d)
    rng = np.random.default_rng(31 * H + W)
    tol = 14 * 2.0 ** -24 + 2 * max(H, W) * 2.0 ** -23
    for C in (3, 4):
        for name, img in _images(H, W, C, rng).items():
            a = R.target_from_u8(img, BG, out_hw)
            b = R.target_from_u8(img, BG.astype(np.float64), out_hw, np.float64)
            assert a.dtype == np.float32 and b.dtype == np.float64
            assert np.abs(a - b).max() <= tol, name
    for name, (p, unit) in _planes(H, W, rng).items():
        a, b = R.plane_from_int(p, unit, out_hw), R.plane_from_int(p, unit, out_hw, np.float64)
        top = float(np.float32(p.max()) * np.float32(unit))
        assert np.abs(a - b).max() <= tol * top, name


def test_restatement_edges():
    """2x2 -> 1x1 is the mean of the four taps; 0/255 alpha composites to the colour or the background exactly."""
    img = np.array([[[0, 10, 20], [40, 50, 60]], [[80, 90, 100], [120, 130, 255]]], np.uint8)
    got = R.target_from_u8(img, None, (1, 1))
    want = (img.astype(np.float64) / 255).mean(axis=(0, 1))
    assert np.abs(got[0, 0] - want).max() <= 4 * 2.0 ** -24
    rgba = np.zeros((3, 3, 4), np.uint8)
    rgba[..., :3] = 77
    rgba[1, 1, 3] = 255
    out = R.target_from_u8(rgba, BG, (3, 3))
    assert np.array_equal(out[1, 1], np.full(3, np.float32(77) / np.float32(255)))
    assert np.array_equal(out[0, 0], BG)


def print_largest():
    by = {}
    for what, H, W, d, diff, tol in differences():
        k = what.split(":")[0]
        by[k] = max(by.get(k, (0.0, 0.0)), (diff / tol, diff))
    for k, (rel, diff) in by.items():
        print(f"{k}: largest difference {diff:.3e} ({rel:.3f} of the tolerance)")


if __name__ == "__main__":
    print_largest()
