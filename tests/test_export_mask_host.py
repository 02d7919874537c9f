"""gs_fusion.export_mask on CPU tensors: the object mask of the toolkit's TSDF export, against the NumPy restatement
of tests/export_mask_reference.py and against pixels worked out by hand from the rule
gray = uint8(0.21 R + 0.72 G + 0.07 B), kept where gray != 0."""
import numpy as np
import pytest
import torch

import export_mask_reference as R
from gs_fusion import export_mask


def _np(t):
    assert isinstance(t, torch.Tensor) and t.dtype == torch.bool
    return t.numpy()


def test_random_rgb_mask_matches_the_restatement():
    rng = np.random.default_rng(0)
    m = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    m[rng.uniform(size=(37, 53)) < 0.5] = 0
    low = rng.uniform(size=(37, 53)) < 0.3           # many values around the thresholds
    m[low] = rng.integers(0, 16, (int(low.sum()), 3), dtype=np.uint8)
    want = R.export_mask(m)
    assert 0.2 < want.mean() < 0.8
    assert np.array_equal(_np(export_mask(m)), want)
    assert np.array_equal(_np(export_mask(torch.from_numpy(m))), want)
    rgba = np.concatenate([m, rng.integers(0, 256, (37, 53, 1), dtype=np.uint8)], -1)  # a fourth channel is not read
    assert np.array_equal(_np(export_mask(rgba)), want)
    for margin in (0, 5):
        assert np.array_equal(_np(export_mask(m, bounding_box=True, margin=margin)),
                              R.export_mask(m, bounding_box=True, margin=margin))


@pytest.mark.parametrize("rgb,keep", [((4, 0, 0), False), ((5, 0, 0), True),      # 0.84 | 1.05
                                      ((0, 1, 0), False), ((0, 2, 0), True),      # 0.72 | 1.44
                                      ((0, 0, 14), False), ((0, 0, 15), True),    # 0.98 | 1.05
                                      ((255, 255, 255), True),                    # 255: the sum is formed in float64
                                      ((2, 1, 1), True), ((0, 0, 0), False)])     # 0.42 + 0.72 + 0.07 = 1.21
def test_threshold_pixels(rgb, keep):
    m = np.zeros((3, 4, 3), np.uint8)
    m[1, 2] = rgb
    got = _np(export_mask(m))
    assert bool(got[1, 2]) == keep and int(got.sum()) == int(keep)


def test_bounding_box_margin_and_clipping():
    H, W = 30, 40
    inner = np.zeros((H, W, 3), np.uint8)
    inner[10:13, 20:22] = 255                      # rows 10..12, columns 20..21
    got = _np(export_mask(inner, bounding_box=True))
    want = np.zeros((H, W), bool)
    want[5:18, 15:27] = True                       # rows 5..17, columns 15..26
    assert np.array_equal(got, want)
    got = _np(export_mask(inner, bounding_box=True, margin=0))
    assert int(got.sum()) == 6 and got[10:13, 20:22].all()
    for (y, x), (ys, xs) in {(2, 3): (slice(0, 8), slice(0, 9)),                     # clipped at the top and left
                             (H - 2, W - 3): (slice(H - 7, H), slice(W - 8, W)),     # at the bottom and right
                             (0, W - 1): (slice(0, 6), slice(W - 6, W)),
                             (H - 1, 0): (slice(H - 6, H), slice(0, 6))}.items():
        one = np.zeros((H, W, 3), np.uint8)
        one[y, x, 1] = 9
        want = np.zeros((H, W), bool)
        want[ys, xs] = True
        assert np.array_equal(_np(export_mask(one, bounding_box=True)), want), (y, x)
    both = np.zeros((H, W, 3), np.uint8)
    both[1, 1] = both[H - 2, W - 2] = (0, 200, 0)
    assert _np(export_mask(both, bounding_box=True)).all()


def test_single_pixel():
    m = np.zeros((21, 21, 3), np.uint8)
    m[10, 10] = (5, 0, 0)
    assert int(_np(export_mask(m)).sum()) == 1
    box = _np(export_mask(m, bounding_box=True))
    assert int(box.sum()) == 121 and box[5:16, 5:16].all()


def test_empty_mask():
    m = np.zeros((8, 9, 3), np.uint8)
    m[2, 2] = (4, 0, 0)                            # below the threshold: still empty
    assert not _np(export_mask(m)).any()
    with pytest.raises(ValueError):
        export_mask(m, bounding_box=True)
    with pytest.raises(ValueError):
        export_mask(np.zeros((8, 9), np.uint8), bounding_box=True)


def test_gray_input_and_bad_input():
    rng = np.random.default_rng(1)
    g = (rng.integers(0, 4, (12, 17)) == 0).astype(np.uint8) * rng.integers(1, 256, (12, 17)).astype(np.uint8)
    assert np.array_equal(_np(export_mask(g)), g != 0)
    assert np.array_equal(_np(export_mask(torch.from_numpy(g != 0))), g != 0)
    assert np.array_equal(_np(export_mask(g, bounding_box=True)), R.export_mask(g, bounding_box=True))
    with pytest.raises(ValueError):
        export_mask(np.zeros((4, 5, 2), np.uint8))
    with pytest.raises(ValueError):
        export_mask(np.zeros((4, 5, 3), np.float32))
    with pytest.raises(ValueError):
        export_mask(np.zeros((5,), np.uint8))
