"""Host: the NumPy + SciPy restatement of the Canny rule (tests/canny_reference.py; the rule is the specification in
include/gsraster.h) against written-out answers, against a second, pixel-by-pixel restatement in plain Python with a
flood-fill stack, and on the two images whose counts the GPU tests rely on.  The rule restates OpenCV's `cv::Canny`;
OpenCV is not available to these tests, so none of them claims agreement with OpenCV itself."""
import numpy as np
import pytest

import canny_reference as R


def _edges(levels, t1=50, t2=150):
    return (R.canny(R.grey(np.asarray(levels)), t1, t2) > 0).astype(np.int32)


def test_vertical_step_of_the_specification():
    img = np.zeros((5, 8, 3), np.float32)
    img[:, 4:] = 1.0                                   # columns 0-3 at 0, columns 4-7 at 255
    want = np.zeros((5, 8), np.uint8)
    want[:, 3] = 255                                   # mag is 1020 in columns 3 and 4: `>` left, `>=` right keeps 3
    edges, cand, strong = R.canny_maps(img)
    assert edges.dtype == np.uint8 and np.array_equal(edges, want)
    assert np.array_equal(cand, want > 0) and np.array_equal(strong, want > 0)


def test_weak_step_alone_is_dropped_and_a_step_of_40_is_a_line():
    lv = np.full((9, 12), 100)
    lv[:, 6:] += 20                                    # mag 4 * 20 = 80: above low = 50, not above high = 150
    edges, cand, strong = R.canny_maps(R.grey(lv))
    assert cand[:, 5].all() and cand.sum() == 9 and not strong.any() and not edges.any()
    lv[:, 6:] += 20                                    # mag 160 > 150
    e = _edges(lv)
    assert e[:, 5].all() and e.sum() == 9


def test_each_branch_of_the_suppression_on_dyadic_images():
    yy, xx = np.mgrid[:7, :7]
    # |dy| >> |dx|: the vertical branch keeps the upper of the two rows of equal magnitude
    want = np.zeros((7, 7), np.int32)
    want[2] = 1
    assert np.array_equal(_edges(np.where(yy >= 3, 64, 0)), want)
    # dx = dy (same sign): compared along (row-1, col-1) / (row+1, col+1); the two pixels that straddle the step have
    # the same magnitude (768 against 256 on either side) and both stay
    diag = np.array([[0, 0, 0, 0, 0, 1, 0],
                     [0, 0, 0, 0, 1, 1, 0],
                     [0, 0, 0, 1, 1, 0, 0],
                     [0, 0, 1, 1, 0, 0, 0],
                     [0, 1, 1, 0, 0, 0, 0],
                     [1, 1, 0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0, 0, 0]])
    assert np.array_equal(_edges(np.where(xx + yy >= 6, 128, 0)), diag)
    # dx = -dy (opposite sign): compared along (row-1, col+1) / (row+1, col-1)
    anti = np.array([[0, 0, 0, 0, 0, 0, 0],
                     [1, 1, 0, 0, 0, 0, 0],
                     [0, 1, 1, 0, 0, 0, 0],
                     [0, 0, 1, 1, 0, 0, 0],
                     [0, 0, 0, 1, 1, 0, 0],
                     [0, 0, 0, 0, 1, 1, 0],
                     [0, 0, 0, 0, 0, 1, 0]])
    lv = np.where(xx - yy >= 0, 128, 0)
    assert np.array_equal(_edges(lv), anti)
    mag, dx, dy = R.gradient(R.to_u8(R.grey(lv)))
    assert (mag[3, 3], dx[3, 3], dy[3, 3]) == (768, 384, -384)


def test_uint8_conversion_truncates_saturates_and_zeroes_nan():
    k = np.arange(256)
    exact = (k / 255.0).astype(np.float32)
    assert np.array_equal(R.to_u8(exact), (exact * np.float32(255.0)).astype(np.uint8))
    below = R.to_u8(exact - np.float32(1e-7))
    assert below[0] == 0 and (below[1:] <= k[1:]).all() and (below[1:] >= k[1:] - 1).all() and (below[1:] < k[1:]).any()
    assert R.to_u8(np.array([np.nan, -0.5, 1.5, np.inf, -np.inf, 0.999999], np.float32)).tolist() == [0, 0, 255, 255, 0, 254]


def test_thresholds_floor_and_swap():
    assert R.thresholds(50, 150) == (50, 150) and R.thresholds(150.9, 50.2) == (50, 150) and R.thresholds(-0.5, 3) == (-1, 3)


def _plain_python_canny(image, t1=50, t2=150):
    """The rule once more, one pixel at a time, with a flood-fill stack for the hysteresis."""
    u8 = R.to_u8(image)
    H, W = u8.shape[:2]
    low, high = R.thresholds(t1, t2)
    px = lambda r, c, ch: int(u8[min(max(r, 0), H - 1), min(max(c, 0), W - 1), ch])
    mag = [[0] * (W + 2) for _ in range(H + 2)]   # one pixel of zeros around
    gx = [[0] * W for _ in range(H)]
    gy = [[0] * W for _ in range(H)]
    for r in range(H):
        for c in range(W):
            best = -1
            for ch in range(3):
                dx = (px(r - 1, c + 1, ch) + 2 * px(r, c + 1, ch) + px(r + 1, c + 1, ch)) \
                    - (px(r - 1, c - 1, ch) + 2 * px(r, c - 1, ch) + px(r + 1, c - 1, ch))
                dy = (px(r + 1, c - 1, ch) + 2 * px(r + 1, c, ch) + px(r + 1, c + 1, ch)) \
                    - (px(r - 1, c - 1, ch) + 2 * px(r - 1, c, ch) + px(r - 1, c + 1, ch))
                if abs(dx) + abs(dy) > best:
                    best, gx[r][c], gy[r][c] = abs(dx) + abs(dy), dx, dy
            mag[r + 1][c + 1] = best
    state = [[0] * W for _ in range(H)]  # 0 none, 1 weak, 2 strong
    for r in range(H):
        for c in range(W):
            m = mag[r + 1][c + 1]
            if m <= low:
                continue
            x, y = abs(gx[r][c]), abs(gy[r][c]) << 15
            t22 = x * 13573
            t67 = t22 + (x << 16)
            if y < t22:
                ok = m > mag[r + 1][c] and m >= mag[r + 1][c + 2]
            elif y > t67:
                ok = m > mag[r][c + 1] and m >= mag[r + 2][c + 1]
            else:
                s = -1 if (gx[r][c] ^ gy[r][c]) < 0 else 1
                ok = m > mag[r][c + 1 - s] and m > mag[r + 2][c + 1 + s]
            if ok:
                state[r][c] = 2 if m > high else 1
    edges = np.zeros((H, W), np.uint8)
    stack = [(r, c) for r in range(H) for c in range(W) if state[r][c] == 2]
    for r, c in stack:
        edges[r, c] = 255
    while stack:
        r, c = stack.pop()
        for rr in range(max(r - 1, 0), min(r + 2, H)):
            for cc in range(max(c - 1, 0), min(c + 2, W)):
                if state[rr][cc] and not edges[rr, cc]:
                    edges[rr, cc] = 255
                    stack.append((rr, cc))
    return edges, np.array(state)


@pytest.mark.parametrize("shape,seed", [((33, 47), 1), ((40, 29), 2), ((17, 64), 3)])
def test_reference_equals_the_pixel_by_pixel_restatement(shape, seed):
    img = R.smooth_random(*shape, seed=seed)
    edges, cand, strong = R.canny_maps(img)
    mine, state = _plain_python_canny(img)
    assert np.array_equal(cand, state > 0) and np.array_equal(strong, state == 2)
    assert np.array_equal(edges, mine)
    assert edges.any() and (cand & (edges == 0)).any()  # the case has kept and dropped candidates


@pytest.mark.parametrize("transposed", [False, True])
def test_two_line_image_keeps_a_weak_line_through_its_distant_head(transposed):
    lv = R.two_line_levels()
    edges, cand, strong = R.canny_maps(R.grey(lv.T if transposed else lv))
    if transposed:
        edges, cand, strong = edges.T, cand.T, strong.T
    assert cand.sum() == 619 and strong.sum() == 23 and np.argwhere(strong)[:, 1].max() <= 3
    assert (edges > 0).sum() == 319
    assert (edges[19] > 0).all() and edges.shape[1] == 300  # kept whole, up to 296 pixels from its strong head
    assert cand[49].sum() == 300 and not edges[49].any()   # the same line without a head: dropped whole


def test_smooth_random_image_has_weak_pixels_kept_and_dropped():
    """The property every random case of the GPU tests must have (65 x 127, default_rng(0), sigma 2): on this
    restatement 2 483 candidates, 2 144 strong, 2 428 edges, 55 weak pixels dropped."""
    edges, cand, strong = R.canny_maps(R.smooth_random(65, 127, 0))
    dropped = int((cand & (edges == 0)).sum())
    kept_weak = int(((edges > 0) & ~strong).sum())
    print(f"candidates {cand.sum()}, strong {strong.sum()}, edges {(edges > 0).sum()}, dropped {dropped}, weak kept {kept_weak}")
    assert dropped >= 20 and kept_weak >= 100
    assert not (edges[~cand] > 0).any() and (edges[strong] == 255).all()


def test_ring_image_keeps_and_drops_whole_rings():
    from scipy import ndimage

    edges, cand, strong = R.canny_maps(R.grey(R.ring_levels(200)))
    labels, n = ndimage.label(cand, structure=np.ones((3, 3)))
    sizes = ndimage.sum(cand, labels, range(1, n + 1))
    kept = np.array([(edges[labels == i] > 0).all() for i in range(1, n + 1)])
    gone = np.array([not (edges[labels == i] > 0).any() for i in range(1, n + 1)])
    assert (kept | gone).all()
    assert (kept & (sizes > 200)).sum() >= 4 and (gone & (sizes > 200)).sum() >= 4  # rings through dozens of tiles


def test_degenerate_shapes():
    for shape in ((1, 1), (1, 37), (37, 1), (2, 2)):
        img = R.smooth_random(max(shape[0], 8), max(shape[1], 8), 5)[:shape[0], :shape[1]]
        e = R.canny(img)
        assert e.shape == shape and e.dtype == np.uint8
    assert R.canny(np.zeros((0, 5, 3), np.float32)).shape == (0, 5)
    step = np.zeros((1, 8, 3), np.float32)
    step[:, 4:] = 1.0
    assert (R.canny(step) > 0).tolist() == [[False, False, False, True, False, False, False, False]]
    for v in (0.0, 0.5, 1.0):
        assert not R.canny(np.full((16, 16, 3), v, np.float32)).any()
