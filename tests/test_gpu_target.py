"""GPU: gs_fused.target_from_u8 / plane_from_int (csrc/target.hip) equal the float32 NumPy restatement of
tests/target_reference.py BIT FOR BIT on every case: sizes that divide and that do not, one-pixel-wide sources, a 2x2
source shrunk to one pixel, a row wider than a workgroup's; a ramp of all 256 byte values, random bytes, alpha 0/255 and
random; a background with 0.0, 1.0 and a value that is no dyadic rational; planes of uint16 (0, 1, 65535, random;
unit 1e-3), uint8 masks and uint8 with unit 1/255.  `out=`: a slice is refused, a matching tensor is written in place
with the guard band around it untouched.  A non-default stream; two calls give the same bytes; the argument checks."""
import numpy as np
import pytest
import torch

import target_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BG = np.array([0.0, 1.0, 0.3], np.float32)  # 0.3 is not a dyadic rational

# (H, W, factors or explicit out sizes)
CASES = {
    "A": [((37, 23), d) for d in (1, 2, 3, 4)] + [((23, 37), d) for d in (1, 2, 3, 4)],
    "B": [((64, 48), d) for d in (2, 4, 8)] + [((48, 64), d) for d in (2, 4, 8)],
    "C": [((1, 7), 1), ((7, 1), 1)],
    "D": [((2, 2), (1, 1))],
    "E": [((3, 257), 2), ((257, 3), 2)],
}
ALL = [(k, hw, d) for k, v in CASES.items() for hw, d in v]
IDS = [f"{k}-{hw[0]}x{hw[1]}-{d}" for k, hw, d in ALL]


def _out_hw(hw, d):
    return d if isinstance(d, tuple) else (max(hw[0] // d, 1), max(hw[1] // d, 1))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _images(H, W, C, rng):
    """name -> uint8 [H,W,C]: the ramp (every byte value, in every channel, as far as the size allows), random bytes,
    and for C = 4 alpha 0/255 only and random alpha."""
    n = H * W * C
    ramp = (np.arange(n) % 256).astype(np.uint8).reshape(H, W, C)
    rnd = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    out = {"ramp": ramp, "random": rnd}
    if C == 4:
        binary = rnd.copy()
        binary[..., 3] = rng.integers(0, 2, (H, W), dtype=np.uint8) * 255
        out["alpha_binary"] = binary
        ramp_a = ramp.copy()
        ramp_a[..., 3] = rng.integers(0, 256, (H, W), dtype=np.uint8)
        out["ramp_alpha_random"] = ramp_a
    return out


def test_ramp_is_u8_over_255_for_every_byte():
    """C = 3 without a resize is exactly u8 / 255: all 256 inputs."""
    from gs_fused import target_from_u8

    img = np.arange(256 * 3, dtype=np.int64).reshape(16, 16, 3) // 3
    img = img.astype(np.uint8)
    got = target_from_u8(torch.from_numpy(img).to(DEV), None, (16, 16)).cpu().numpy()
    want = img.astype(np.float32) / np.float32(255)
    assert np.array_equal(_bits(got), _bits(want))
    assert set(np.unique(img)) == set(range(256))


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("case,hw,d", ALL, ids=IDS)
def test_target_bit_equal(case, hw, d, C):
    from gs_fused import target_from_u8

    H, W = hw
    out_hw = _out_hw(hw, d)
    rng = np.random.default_rng(1000 * H + W + C)
    bg = torch.from_numpy(BG).to(DEV)
    for name, img in _images(H, W, C, rng).items():
        got = target_from_u8(torch.from_numpy(img).to(DEV), bg, out_hw)
        assert got.shape == (*out_hw, 3) and got.dtype == torch.float32
        want = R.target_from_u8(img, BG, out_hw)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), f"{case} {name} C={C} -> {out_hw}"


@pytest.mark.parametrize("case,hw,d", ALL, ids=IDS)
def test_plane_bit_equal(case, hw, d):
    from gs_fused import plane_from_int

    H, W = hw
    out_hw = _out_hw(hw, d)
    rng = np.random.default_rng(77 * H + W)
    depth = rng.integers(0, 65536, (H, W)).astype(np.uint16)
    depth.reshape(-1)[:3] = (0, 1, 65535)
    depth.reshape(-1)[-1] = 65535
    planes = {
        "depth_u16": (depth, 1e-3),
        "mask_u8": (rng.integers(0, 2, (H, W)).astype(np.uint8), 1.0),
        "mono_u8": (rng.integers(0, 256, (H, W)).astype(np.uint8), 1.0 / 255.0),
    }
    for name, (p, unit) in planes.items():
        got = plane_from_int(torch.from_numpy(p).to(DEV), unit, out_hw)
        assert got.shape == out_hw and got.dtype == torch.float32
        want = R.plane_from_int(p, unit, out_hw)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), f"{case} {name} -> {out_hw}"
    if out_hw == (H, W):  # a mask stays 0/1 without a resize
        m = plane_from_int(torch.from_numpy(planes["mask_u8"][0]).to(DEV), 1.0, out_hw).cpu().numpy()
        assert np.array_equal(m, planes["mask_u8"][0].astype(np.float32))


def test_out_in_place_guard_band_and_slice_refused():
    from gs_fused import plane_from_int, target_from_u8

    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (37, 23, 4), dtype=np.uint8)
    t, bg = torch.from_numpy(img).to(DEV), torch.from_numpy(BG).to(DEV)
    h, w = 18, 11
    guard = -7.0
    big = torch.full((3, h, w, 3), guard, device=DEV)
    ret = target_from_u8(t, bg, (h, w), out=big[1])
    assert ret.data_ptr() == big[1].data_ptr()
    assert np.array_equal(_bits(big[1].cpu().numpy()), _bits(R.target_from_u8(img, BG, (h, w))))
    assert bool((big[0] == guard).all()) and bool((big[2] == guard).all())
    wide = torch.full((h, w + 2, 3), guard, device=DEV)
    with pytest.raises(ValueError, match="out"):
        target_from_u8(t, bg, (h, w), out=wide[:, 1:-1])
    assert bool((wide == guard).all())
    with pytest.raises(ValueError, match="out"):
        target_from_u8(t, bg, (h, w), out=torch.empty((h, w, 4), device=DEV))
    with pytest.raises(ValueError, match="out"):
        target_from_u8(t, bg, (h, w), out=torch.empty((h, w, 3), device=DEV, dtype=torch.float64))
    # planes
    p = rng.integers(0, 65536, (37, 23)).astype(np.uint16)
    bigp = torch.full((3, h, w), guard, device=DEV)
    plane_from_int(torch.from_numpy(p).to(DEV), 1e-3, (h, w), out=bigp[1])
    assert np.array_equal(_bits(bigp[1].cpu().numpy()), _bits(R.plane_from_int(p, 1e-3, (h, w))))
    assert bool((bigp[0] == guard).all()) and bool((bigp[2] == guard).all())
    widep = torch.full((h, w + 2), guard, device=DEV)
    with pytest.raises(ValueError, match="out"):
        plane_from_int(torch.from_numpy(p).to(DEV), 1e-3, (h, w), out=widep[:, 1:-1])
    assert bool((widep == guard).all())


def test_non_default_stream_and_repeat():
    from gs_fused import plane_from_int, target_from_u8

    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (64, 48, 4), dtype=np.uint8)
    p = rng.integers(0, 65536, (64, 48)).astype(np.uint16)
    t, tp, bg = torch.from_numpy(img).to(DEV), torch.from_numpy(p).to(DEV), torch.from_numpy(BG).to(DEV)
    first, firstp = target_from_u8(t, bg, (32, 24)), plane_from_int(tp, 1e-3, (32, 24))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        second, secondp = target_from_u8(t, bg, (32, 24)), plane_from_int(tp, 1e-3, (32, 24))
    side.synchronize()
    assert np.array_equal(_bits(first.cpu().numpy()), _bits(second.cpu().numpy()))
    assert np.array_equal(_bits(firstp.cpu().numpy()), _bits(secondp.cpu().numpy()))
    assert np.array_equal(_bits(first.cpu().numpy()), _bits(R.target_from_u8(img, BG, (32, 24))))
    assert np.array_equal(_bits(secondp.cpu().numpy()), _bits(R.plane_from_int(p, 1e-3, (32, 24))))


def test_argument_checks_name_the_offender():
    from gs_fused import plane_from_int, target_from_u8

    img = torch.zeros((8, 6, 4), dtype=torch.uint8, device=DEV)
    bg = torch.zeros(3, device=DEV)
    bad = [
        ("image_u8", lambda: target_from_u8(img.float(), bg, (4, 3))),
        ("image_u8", lambda: target_from_u8(img.cpu(), bg.cpu(), (4, 3))),
        ("contiguous", lambda: target_from_u8(img[:, ::2], bg, (4, 3))),
        ("channels", lambda: target_from_u8(torch.zeros((8, 6, 2), dtype=torch.uint8, device=DEV), bg, (4, 3))),
        ("out_hw", lambda: target_from_u8(img, bg, (9, 3))),
        ("out_hw", lambda: target_from_u8(img, bg, (4, 7))),
        ("out_hw", lambda: target_from_u8(img, bg, (0, 3))),
        ("background", lambda: target_from_u8(img, bg.double(), (4, 3))),
        ("background", lambda: target_from_u8(img, torch.zeros(4, device=DEV), (4, 3))),
        ("background", lambda: target_from_u8(img, bg.cpu(), (4, 3))),
        ("background", lambda: target_from_u8(img, None, (4, 3))),
        ("plane", lambda: plane_from_int(torch.zeros((8, 6), device=DEV), 1.0, (4, 3))),
        ("plane", lambda: plane_from_int(torch.zeros((8, 6), dtype=torch.uint8), 1.0, (4, 3))),
        ("plane", lambda: plane_from_int(img, 1.0, (4, 3))),
        ("contiguous", lambda: plane_from_int(img[..., 0], 1.0, (4, 3))),
        ("out_hw", lambda: plane_from_int(img[..., 0].contiguous(), 1.0, (4, 0))),
    ]
    for word, call in bad:
        with pytest.raises(ValueError, match=word):
            call()


def test_image_cache_serves_targets_masks_depth():
    from gs_fused import ImageCache

    rng = np.random.default_rng(8)
    H, W, n = 37, 23, 3
    imgs = [rng.integers(0, 256, (H, W, 4), dtype=np.uint8) for _ in range(n)]
    masks = [rng.integers(0, 2, (H, W)).astype(np.uint8) for _ in range(n)]
    depths = [rng.integers(0, 65536, (H, W)).astype(np.uint16) for _ in range(n)]
    cache = ImageCache(imgs, masks, depths, depth_unit=1e-3, device=DEV)
    assert len(cache) == n and cache.nbytes == n * H * W * (4 + 1 + 2)
    bg = torch.from_numpy(BG).to(DEV)
    for d in (1, 2):
        hw = (H // d, W // d)
        assert np.array_equal(_bits(cache.target(1, d, bg).cpu().numpy()), _bits(R.target_from_u8(imgs[1], BG, hw)))
        m = cache.mask(2, d)
        assert m.shape == (*hw, 1) and cache.mask(2, d) is m  # cached per (view, factor)
        assert np.array_equal(_bits(m[..., 0].cpu().numpy()), _bits(R.plane_from_int(masks[2], 1.0, hw)))
        z = cache.depth(0, d)
        assert cache.depth(0, d) is z
        assert np.array_equal(_bits(z.cpu().numpy()), _bits(R.plane_from_int(depths[0], 1e-3, hw)))
    out = torch.empty((H // 2, W // 2, 3), device=DEV)
    cache.deferred_target(0, 2, bg).write(out)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(R.target_from_u8(imgs[0], BG, (H // 2, W // 2))))
