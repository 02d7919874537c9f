"""GPU: the three fused monocular-depth heads of the co-gs loss (gs_fused.local_pearson_loss, log_depth_loss, tv_loss;
csrc/mono_depth.hip) against the float64 restatement of tests/mono_depth_reference.py.

Tolerances, per term: the kernels are held to float64 at 4 x the error the torch restatement has in float32 on the CPU
against float64 on the golden cases (tests/test_mono_depth_host.py measures r_loss, r_grad on every run), never below
4 * 2^-24 = 2.38e-7 -- the rule of tests/test_gpu_depth_reg.py.  Losses relative, gradients relative to the largest
float64 entry:
    local Pearson  r = (5.04e-8, 2.74e-7)  ->  loss 2.38e-7, gradient 1.10e-6
    log-depth      r = (8.72e-8, 3.22e-7)  ->  loss 3.49e-7, gradient 1.29e-6
    TV             r = (3.51e-8, 4.54e-8)  ->  loss 2.38e-7, gradient 2.38e-7
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mono_depth_reference as M
from test_mono_depth_host import R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cogs_losses.npz")
FLOOR = 4 * 2.0 ** -24
TOL = {k: (max(4 * r_loss, FLOOR), max(4 * r_grad, FLOOR)) for k, (r_loss, r_grad) in R.items()}
SCALE, SHIFT = 0.875, 0.125   # (exact in float32: the heads take scale and shift as float32)


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def _want(name, pred, gt, img=None, box=None, rows=None, cols=None, scale=SCALE, shift=SHIFT, mask=None):
    """The restatement's (loss, gradient); a mask enters as the float32 products, as the kernels form them."""
    m = None if mask is None else np.asarray(mask, np.float32).reshape(pred.shape)
    p, g = (pred.astype(np.float64), gt.astype(np.float64)) if m is None else M.products(pred, gt, m)
    if name == "local_pearson":
        return M.local_pearson(p, g, box, rows, cols, m)
    if name == "log_depth":
        return M.log_depth(p, g, img, scale, shift, m)
    return M.tv(p, m)


def _got(name, pred, gt, img=None, box=None, rows=None, cols=None, scale=SCALE, shift=SHIFT, mask=None, upstream=1.0,
         index=torch.int64):
    """The head's (loss, gradient as float64 of pred's shape); pred / mask: NumPy arrays or device tensors."""
    import gs_fused

    p = (pred if isinstance(pred, torch.Tensor) else _t(pred)).detach().requires_grad_(True)
    m = mask if mask is None or isinstance(mask, torch.Tensor) else _t(mask)
    if name == "local_pearson":
        loss = gs_fused.local_pearson_loss(p, _t(gt), box, _t(np.asarray(rows)).to(index), _t(np.asarray(cols)).to(index),
                                           mask=m)
    elif name == "log_depth":
        loss = gs_fused.log_depth_loss(p, _t(gt), _t(img), scale, shift, mask=m)
    else:
        loss = gs_fused.tv_loss(p, mask=m)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda
    (upstream * loss).backward()
    assert p.grad.shape == p.shape
    return loss.detach(), p.grad


def _compare(name, got, want, upstream=1.0, what=""):
    loss, grad = float(got[0]), got[1].cpu().numpy().astype(np.float64).reshape(want[1].shape)
    loss64, grad64 = want[0], upstream * want[1]
    finite = np.isfinite(grad64)
    top = np.abs(grad64[finite]).max() if finite.any() else 0.0
    e_loss = 0.0 if np.isnan(loss64) else abs(loss - loss64) / (abs(loss64) if loss64 != 0 else 1.0)
    e_grad = float(np.abs(grad - grad64)[finite].max() / (top if top > 0 else 1.0)) if finite.any() else 0.0
    print(f"{name} {what}: loss {loss:.9g} (float64 {loss64:.12g}, rel {e_loss:.2e}), gradient rel {e_grad:.2e}")
    assert np.isnan(loss) == np.isnan(loss64), (name, what, loss, loss64)
    assert np.array_equal(np.isnan(grad), np.isnan(grad64)), (name, what, int(np.isnan(grad).sum()), int(np.isnan(grad64).sum()))
    assert e_loss <= TOL[name][0], (name, what, e_loss)
    assert e_grad <= TOL[name][1], (name, what, e_grad)
    return loss, grad


def _check(name, pred, gt, img=None, upstream=1.0, what="", index=torch.int64, **kw):
    return _compare(name, _got(name, pred, gt, img, upstream=upstream, index=index, **kw), _want(name, pred, gt, img, **kw),
                    upstream, what)


def _corners(H, W, box, count, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, H - box + 1, count), rng.integers(0, W - box + 1, count)


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_every_golden_case():
    z = np.load(GOLDEN)
    for c in ("c0", "c1", "c2"):
        pred, gt, img = z[f"{c}_pred"], z[f"{c}_gt"], z[f"{c}_img"]
        scale, shift = (float(v) for v in z[f"{c}_scale_shift"])
        kw = {"local_pearson": dict(box=int(z[f"{c}_box_pcorr"][0]), rows=z[f"{c}_patch_rows"], cols=z[f"{c}_patch_cols"]),
              "log_depth": dict(scale=scale, shift=shift), "tv": {}}
        for name in R:
            got, _ = _check(name, pred, gt, img, what=c, **kw[name])
            # and against what the reference's own float32 code produced, at its error plus the kernels'
            ref = float(z[f"{c}_{name}"])
            assert abs(got - ref) <= (R[name][0] + TOL[name][0]) * abs(ref), (c, name, got, ref)


@pytest.mark.parametrize("H,W,box,count", [(2, 2, 2, 1), (9, 11, 2, "all"), (40, 56, 5, 30), (33, 47, 17, 12),
                                           (130, 257, 128, 6), (64, 64, 64, 1)])
def test_local_pearson_shapes_against_float64(H, W, box, count):
    pred, gt, _ = M.smooth_noise(H, W, seed=H * 1000 + W)
    if count == "all":
        rows, cols = (a.reshape(-1) for a in np.mgrid[0:H - box + 1, 0:W - box + 1])
        assert len(rows) == 80
    else:
        rows, cols = _corners(H, W, box, count, seed=box)
    if (H, W) == (130, 257):
        rows[:2], cols[:2] = (0, 2), (0, 129)      # the first and the last valid corner
    _check("local_pearson", pred, gt, box=box, rows=rows, cols=cols, what=f"{H}x{W} box {box}")


def test_local_pearson_repeated_corner_and_more_patches_than_any_list():
    pred, gt, _ = M.smooth_noise(40, 56, 1)
    _check("local_pearson", pred, gt, box=5, rows=np.array([7, 7, 7]), cols=np.array([20, 20, 20]), what="one corner x 3")
    pred, gt, _ = M.smooth_noise(64, 64, 2)
    rows, cols = _corners(64, 64, 4, 3000, seed=3)
    _, g = _check("local_pearson", pred, gt, box=4, rows=rows, cols=cols, what="3000 patches")
    # another patch order: the same sums in another order
    perm = np.random.default_rng(4).permutation(3000)
    _, gp = _check("local_pearson", pred, gt, box=4, rows=rows[perm], cols=cols[perm], what="3000 patches, permuted")
    assert np.abs(gp - g).max() <= TOL["local_pearson"][1] * np.abs(g).max()


def test_local_pearson_nan_patterns():
    pred, gt, _ = M.smooth_noise(33, 47, 5)
    none = np.zeros(0, np.int64)
    loss, _ = _got("local_pearson", pred, gt, box=8, rows=none, cols=none)
    assert torch.isnan(loss)
    flat = pred.copy()
    flat[4:12, 6:14] = 2.5
    _, g = _check("local_pearson", flat, gt, box=8, rows=np.array([4, 20, 3]), cols=np.array([6, 30, 7]), what="constant patch")
    assert np.isnan(g).sum() == 64 and np.isnan(g[4:12, 6:14]).all()
    flat_gt = gt.copy()
    flat_gt[20:28, 30:38] = 1.0
    _, g = _check("local_pearson", pred, flat_gt, box=8, rows=np.array([4, 20]), cols=np.array([6, 30]), what="constant target")
    assert np.isnan(g).sum() == 64 and np.isnan(g[20:28, 30:38]).all()
    _, g = _check("local_pearson", pred, gt, box=1, rows=np.array([3]), cols=np.array([4]), what="box 1")
    assert np.isnan(g).sum() == 1


def test_local_pearson_out_of_range_corner_reads_and_writes_nothing_outside():
    """Through the C ABI, with v_pred inside a guard band: corners that would leave the image (negative, past the last
    valid one, beyond int32) give a NaN loss and add nothing; the band stays untouched."""
    from rasterizer.cuda import _call, _ptr, _stream

    H, W, box, guard = 33, 47, 17, 4096
    pred, gt, _ = M.smooth_noise(H, W, 6)
    rows, cols = np.array([0, 17, -1, 2 ** 40, 3, 16]), np.array([0, 5, 2, 1, 31, 30])
    want = M.local_pearson(pred, gt, box, rows, cols)
    assert np.isnan(want[0]) and np.isfinite(want[1]).all()
    p, g, r, c = _t(pred), _t(gt), _t(rows), _t(cols)
    dev = p.device
    stats = torch.empty((len(rows), 5), dtype=torch.float64, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    buf = torch.full((H * W + 2 * guard,), -7.0, dtype=torch.float32, device=dev)
    up = torch.ones(1, dtype=torch.float32, device=dev)
    v_pred = buf[guard:guard + H * W]
    _call("gsr_local_pearson_forward", C.c_uint(H), C.c_uint(W), C.c_int(box), C.c_int(len(rows)), _ptr(p), _ptr(g),
          C.c_void_p(None), _ptr(r), _ptr(c), C.c_int(1), _ptr(stats), _ptr(loss), _stream(dev))
    _call("gsr_local_pearson_backward", C.c_uint(H), C.c_uint(W), C.c_int(box), C.c_int(len(rows)), _ptr(up), _ptr(p),
          _ptr(g), C.c_void_p(None), _ptr(r), _ptr(c), C.c_int(1), _ptr(stats), _ptr(v_pred), _stream(dev))
    torch.cuda.synchronize()
    assert bool((buf[:guard] == -7.0).all()) and bool((buf[guard + H * W:] == -7.0).all())
    _compare("local_pearson", (loss, v_pred.reshape(H, W)), want, what="out-of-range corners")
    patch = torch.isnan(stats[:, 4]).cpu().numpy()
    assert patch.tolist() == [False, True, True, True, True, False]     # row 17 > 33 - 17, column 31 > 47 - 17


def test_local_pearson_int32_and_int64_corners_are_bit_equal():
    pred, gt, _ = M.smooth_noise(40, 56, 7)
    rows, cols = _corners(40, 56, 5, 30, seed=8)
    a = _got("local_pearson", pred, gt, box=5, rows=rows, cols=cols, index=torch.int64)
    b = _got("local_pearson", pred, gt, box=5, rows=rows, cols=cols, index=torch.int32)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


@pytest.mark.parametrize("shape", [(2, 2), (2, 37), (37, 2), (17, 31), (65, 127), (257, 300)])
def test_log_depth_and_tv_shapes_against_float64(shape):
    pred, gt, img = M.smooth_noise(*shape, seed=shape[0] * 1000 + shape[1])
    _check("log_depth", pred, gt, img, what=f"{shape}")
    _check("tv", pred, gt, what=f"{shape}")


def test_scale_and_shift_as_numbers_and_as_device_tensors_are_bit_equal():
    pred, gt, img = M.smooth_noise(17, 31, 9)
    a = _got("log_depth", pred, gt, img, scale=0.83, shift=-0.17)
    b = _got("log_depth", pred, gt, img, scale=torch.tensor(0.83, device=DEV), shift=torch.tensor(-0.17, device=DEV))
    c = _got("log_depth", pred, gt, img, scale=torch.tensor([0.83], device=DEV, dtype=torch.float64), shift=-0.17)
    for other in (b, c):
        assert torch.equal(_bits(a[0]), _bits(other[0])) and torch.equal(_bits(a[1]), _bits(other[1]))
    assert float(a[0]) != float(_got("log_depth", pred, gt, img, scale=1.0, shift=0.0)[0])


def test_exact_ties_have_gradient_zero_and_one_row_is_nan():
    pred, gt, img = M.smooth_noise(17, 31, 10)
    gt = gt.copy()
    gt[7, 3] = pred[7, 3]                                  # pred == gt (scale 1, shift 0): sign(0) = 0
    _, g = _check("log_depth", pred, gt, img, scale=1.0, shift=0.0, what="tie")
    assert g[7, 3] == 0.0 and (g[:-1, :-1] != 0).sum() == g[:-1, :-1].size - 1
    flat = np.full((9, 12), 2.0, np.float32)
    flat[4:, 5:] = 3.0                                     # equal neighbours everywhere but along one step
    _, g = _check("tv", flat, flat, what="ties")
    assert not g[:3, :4].any() and not g[5:, 6:].any() and g[3:5, 4:6].any()
    pred, gt, img = M.smooth_noise(1, 37, 11)
    for name in ("log_depth", "tv"):
        _check(name, pred, gt, img, what="H == 1")
        assert torch.isnan(_got(name, pred, gt, img)[0])
        assert torch.isnan(_got(name, pred.T.copy(), gt.T.copy(), np.ascontiguousarray(img.transpose(1, 0, 2)))[0])


def _case(name):
    pred, gt, img = M.smooth_noise(40, 56, 12)
    rows, cols = _corners(40, 56, 9, 24, seed=13)          # 24 patches of 81 pixels on 2240: they overlap
    return pred, gt, img, (dict(box=9, rows=rows, cols=cols) if name == "local_pearson" else {})


@pytest.mark.parametrize("name", list(R))
def test_masks_of_every_kind(name):
    pred, gt, img, kw = _case(name)
    rng = np.random.default_rng(14)
    real = rng.uniform(0.0, 1.5, pred.shape).astype(np.float32)
    binary = rng.uniform(size=pred.shape) < 0.7
    _check(name, pred, gt, img, mask=real, what="float mask", **kw)
    _check(name, pred, gt, img, mask=real[..., None], what="[H,W,1] mask", **kw)
    want = _want(name, pred, gt, img, mask=binary.astype(np.float32), **kw)
    for m in (_t(binary), _t(binary.astype(np.uint8))):
        _, g = _compare(name, _got(name, pred, gt, img, mask=m, **kw), want, what=f"{m.dtype} mask")
        assert not g[~binary].any()
    _, g = _check(name, pred, gt, img, mask=np.zeros(pred.shape, np.float32), what="mask of zeros", **kw)
    if name != "local_pearson":                            # (local Pearson of two zero images is 0 / 0)
        assert not g.any()


@pytest.mark.parametrize("name", list(R))
def test_upstream_trailing_axis_and_non_contiguous_input(name):
    pred, gt, img, kw = _case(name)
    _, g1 = _check(name, pred, gt, img, what="upstream 1", **kw)
    _, g3 = _check(name, pred, gt, img, upstream=-2.5, what="upstream -2.5", **kw)
    assert np.abs(g3 + 2.5 * g1).max() <= 2.0 ** -22 * np.abs(g3).max()
    want = _want(name, pred, gt, img, **kw)
    _, gt1 = _compare(name, _got(name, _t(pred[..., None]), gt, img, **kw), want, what="[H,W,1]")
    assert np.array_equal(gt1, g1)
    strided = _t(np.ascontiguousarray(pred.T)).t()         # the same image, column-major
    assert not strided.is_contiguous()
    _, gs = _compare(name, _got(name, strided, gt, img, **kw), want, what="non-contiguous")
    assert np.array_equal(gs, g1)


@pytest.mark.parametrize("name", list(R))
def test_loss_and_gradient_are_bit_equal_over_two_runs(name):
    """For local Pearson over overlapping patches: the case the torch path (index_put_ with atomics) cannot pass."""
    pred, gt, img = M.smooth_noise(257, 300, 15)
    kw = {}
    if name == "local_pearson":
        rows, cols = _corners(257, 300, 32, 200, seed=16)
        kw = dict(box=32, rows=rows, cols=cols)
        cover = np.zeros((257, 300), np.int32)
        for r, c in zip(rows, cols):
            cover[r:r + 32, c:c + 32] += 1
        assert cover.max() >= 4
    a = _got(name, pred, gt, img, **kw)
    b = _got(name, pred, gt, img, **kw)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    assert float(a[1].abs().max()) > 0


def test_argument_checks():
    import gs_fused

    p, img = torch.ones(6, 8, device=DEV), torch.ones(6, 8, 3, device=DEV)
    idx = torch.zeros(2, dtype=torch.int64, device=DEV)
    lp, ld, tv = gs_fused.local_pearson_loss, gs_fused.log_depth_loss, gs_fused.tv_loss
    for bad in (0, -1, 7):
        with pytest.raises(ValueError):
            lp(p, p, bad, idx, idx)                                    # box outside [1, min(H, W)]
    with pytest.raises(RuntimeError):
        lp(p.cpu(), p.cpu(), 2, idx.cpu(), idx.cpu())                  # CPU tensors: no CPU path
    with pytest.raises(RuntimeError):
        lp(p, p, 2, idx.cpu(), idx.cpu())
    with pytest.raises(RuntimeError):
        lp(p, p.cpu(), 2, idx, idx)
    with pytest.raises(RuntimeError):
        lp(p.double(), p, 2, idx, idx)
    with pytest.raises(ValueError):
        lp(p, p[:5], 2, idx, idx)
    with pytest.raises(ValueError):
        lp(p, p, 2, idx.float(), idx.float())
    with pytest.raises(ValueError):
        lp(p, p, 2, idx, idx[:1])
    with pytest.raises(ValueError):
        lp(p, p, 2, idx, idx.int())
    with pytest.raises(RuntimeError):
        ld(p.cpu(), p.cpu(), img.cpu())
    with pytest.raises(RuntimeError):
        ld(p, p, img.cpu())
    with pytest.raises(ValueError):
        ld(p, p, img[..., :1])
    with pytest.raises(ValueError):
        ld(p, p, img, scale=torch.ones(2, device=DEV))
    with pytest.raises(RuntimeError):
        ld(p, p, img, scale=torch.ones(1))
    with pytest.raises(RuntimeError):
        tv(p.cpu())
    with pytest.raises(RuntimeError):
        tv(p.double())
    with pytest.raises(ValueError):
        tv(torch.ones(0, 5, device=DEV))
    with pytest.raises(ValueError):
        tv(torch.ones(6, device=DEV))
    for head in (lambda m: lp(p, p, 2, idx, idx, mask=m), lambda m: ld(p, p, img, mask=m), lambda m: tv(p, mask=m)):
        with pytest.raises(ValueError):
            head(torch.ones(8, 6, device=DEV))
        with pytest.raises(ValueError):
            head(torch.ones(6, 8, device=DEV, dtype=torch.float64))
        with pytest.raises(RuntimeError):
            head(torch.ones(6, 8))
    x = torch.rand(6, 8, device=DEV)
    assert tv(x).requires_grad is False and ld(x, p, img).requires_grad is False     # nothing to differentiate
    g = p.clone().requires_grad_(True)
    ld(x.requires_grad_(True), g, img).backward()
    assert g.grad is None                                                              # the ground truth is data
