"""GPU: the Canny edge mask (gs_fused.canny / image2canny, csrc/canny.hip) against the NumPy + SciPy oracle of
tests/canny_reference.py.  Every comparison is exact: the uint8 edges equal the oracle's.  What the shared images are
assumed to hold (kept and dropped weak lines, whole rings) is asserted on the oracle alone in tests/test_canny_host.py.
"""
import numpy as np
import pytest
import torch

import canny_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def _same_as_oracle(img, t1=50, t2=150):
    from gs_fused import canny

    got = canny(_t(img), t1, t2)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == img.shape[:2]
    want = R.canny(img, t1, t2)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), f"{(got != want).sum()} of {want.size} pixels differ"
    return want


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (37, 1), (2, 2), (3, 3), (16, 16), (17, 31), (64, 64), (65, 127),
                                   (257, 300)])
def test_smooth_random_images_across_every_tile_border(shape):
    big = R.smooth_random(max(shape[0], 8), max(shape[1], 8), seed=shape[0] * 1000 + shape[1])
    img = np.ascontiguousarray(big[:shape[0], :shape[1]])
    want = _same_as_oracle(img)
    if min(shape) >= 16:
        assert want.any()
    # a 1-pixel-high or -wide step still has its edge
    if shape in ((1, 37), (37, 1)):
        step = np.zeros(shape + (3,), np.float32)
        step.reshape(-1, 3)[20:] = 1.0
        assert (_same_as_oracle(step) > 0).sum() == 1


def test_the_generator_of_the_random_cases_at_its_pinned_seed():
    want = _same_as_oracle(R.smooth_random(65, 127, 0))
    assert (want > 0).sum() == 2428


@pytest.mark.parametrize("transposed", [False, True])
def test_two_line_image(transposed):
    lv = R.two_line_levels()
    want = _same_as_oracle(R.grey(lv.T if transposed else lv))
    assert (want > 0).sum() == 319


def test_rings_are_kept_or_dropped_as_wholes():
    want = _same_as_oracle(R.grey(R.ring_levels(200)))
    assert (want > 0).sum() > 2000


@pytest.mark.parametrize("value", [0.0, 1.0, 0.5])
def test_constant_images_have_no_edges(value):
    assert not _same_as_oracle(np.full((48, 70, 3), value, np.float32)).any()


def test_truncation_at_exact_and_just_below_levels():
    rng = np.random.default_rng(3)
    k = rng.integers(0, 256, (40, 56, 3))
    # smooth the levels a little so that the image has edges of every strength, then hit k / 255 exactly
    from scipy import ndimage

    k = np.rint(ndimage.gaussian_filter(k.astype(np.float64), (1.5, 1.5, 0))).astype(np.int64)
    k = np.clip((k - k.min()) * 255 // max(int(k.max() - k.min()), 1), 0, 255)
    exact = (k / 255.0).astype(np.float32)
    below = exact - np.float32(1e-7)
    assert np.array_equal(R.to_u8(exact), k) and (R.to_u8(below) == k - 1)[k > 0].all()
    assert _same_as_oracle(exact).any()
    _same_as_oracle(below)
    # half the values exact, half just below: neighbouring levels now differ by the truncation alone, and the edges
    # are no longer those of the exact image (a kernel that rounded to nearest would return exactly those)
    mixed = np.where(rng.uniform(size=k.shape) < 0.5, exact, below)
    assert not np.array_equal(_same_as_oracle(mixed), R.canny(exact))


def test_nan_and_out_of_range_values_follow_the_stated_saturation():
    img = R.smooth_random(40, 50, 11)
    rng = np.random.default_rng(12)
    where = rng.uniform(size=img.shape)
    img[where < 0.02] = np.nan
    img[(where >= 0.02) & (where < 0.04)] = -0.5
    img[(where >= 0.04) & (where < 0.06)] = 1.5
    img[0, 0] = (np.inf, -np.inf, np.nan)
    assert _same_as_oracle(img).any()


def test_thresholds_floor_swap_and_other_values():
    img = R.smooth_random(50, 60, 21)
    a = _same_as_oracle(img, 50, 150)
    assert np.array_equal(_same_as_oracle(img, 150.7, 50.3), a)
    b = _same_as_oracle(img, 20, 60)
    assert (b > 0).sum() > (a > 0).sum()
    _same_as_oracle(img, 300, 300)


def test_argument_checks_and_non_contiguous_input():
    from gs_fused import canny, image2canny

    img = R.smooth_random(30, 44, 31)
    wide = _t(np.concatenate([img, img[:, ::-1]], axis=1))
    view = wide[:, :44]
    assert not view.is_contiguous()
    assert np.array_equal(canny(view).cpu().numpy(), R.canny(img))
    chan = _t(np.ascontiguousarray(img.transpose(2, 0, 1))).permute(1, 2, 0)  # planar storage, [H,W,3] view
    assert not chan.is_contiguous() and np.array_equal(canny(chan).cpu().numpy(), R.canny(img))
    with pytest.raises(RuntimeError):
        canny(torch.from_numpy(img))                       # a CPU tensor: there is no CPU path
    with pytest.raises(RuntimeError):
        image2canny(torch.from_numpy(img), 50, 150)
    with pytest.raises(RuntimeError):
        canny(_t(img).double())
    with pytest.raises(RuntimeError):
        canny(_t(img).half())
    with pytest.raises(ValueError):
        canny(_t(img[..., :2]))
    with pytest.raises(ValueError):
        canny(_t(img[..., 0]))
    with pytest.raises(RuntimeError):
        canny(_t(img), workspace=torch.empty(64, dtype=torch.uint8, device=DEV))   # too small
    for shape in ((0, 5, 3), (5, 0, 3)):
        e = canny(torch.empty(shape, device=DEV))
        assert e.dtype == torch.uint8 and tuple(e.shape) == shape[:2]


def test_two_runs_are_bit_equal_and_the_workspace_needs_no_zeroing():
    from gs_fused import canny, canny_workspace_bytes

    img = R.grey(R.ring_levels(200))
    want = R.canny(img)
    t = _t(img)
    need = canny_workspace_bytes(200, 200)
    assert need >= 6 * 200 * 200 and need < 6 * 200 * 200 + 3 * 256 and need % 256 == 0
    first = canny(t)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
    second = canny(t, workspace=ws)
    assert torch.equal(first, second) and np.array_equal(second.cpu().numpy(), want)
    # the same workspace, now holding the leftovers of another image's run
    other = R.smooth_random(200, 200, 41)
    assert np.array_equal(canny(_t(other), workspace=ws).cpu().numpy(), R.canny(other))
    assert np.array_equal(canny(t, workspace=ws).cpu().numpy(), want)


def test_guard_rows_around_the_output_stay_untouched():
    from gs_fused import canny

    img = R.smooth_random(65, 127, 0)
    buf = torch.full((65 + 8, 127), 0xAB, dtype=torch.uint8, device=DEV)
    out = canny(_t(img), out=buf[4:69])
    assert out.data_ptr() == buf[4:69].data_ptr()
    got = buf.cpu().numpy()
    assert (got[:4] == 0xAB).all() and (got[69:] == 0xAB).all()
    assert np.array_equal(got[4:69], R.canny(img))


def test_image2canny_has_the_references_signature_and_values():
    from gs_fused import image2canny

    img = R.smooth_random(65, 127, 0)
    t = _t(img).requires_grad_(True)   # the model hands it a tensor that may carry a graph: it is detached
    for is_edge in (True, False):
        got = image2canny(t, 50, 150, isEdge1=is_edge)
        assert got.dtype == torch.float32 and got.is_cuda and not got.requires_grad and tuple(got.shape) == (65, 127)
        assert np.array_equal(got.cpu().numpy(), R.image2canny(img, 50, 150, is_edge))
    assert np.array_equal(image2canny(t, 50, 150).cpu().numpy(), R.image2canny(img, 50, 150))  # isEdge1 defaults to True
    assert set(np.unique(image2canny(t, 50, 150, False).cpu().numpy())) == {0.0, 1.0}
