"""The typed handle computes what the raw one does: one entry called through `_backend.lib()` with every argument
wrapped by hand, and through `_call` with plain values, on the same inputs -- bit-equal outputs."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _raw(name, *args):
    from rasterizer.cuda._backend import lib

    rc = getattr(lib(), name)(*args)
    assert rc == 0, lib().gsr_last_error().decode()


def test_sh_forward_raw_and_typed_agree():
    """n = 65 (one wave and one), degree 3: unsigned scalars and pointers."""
    from rasterizer.cuda import _call, _ptr, _stream

    n, degree = 65, 3
    g = torch.Generator().manual_seed(3)
    dirs = torch.nn.functional.normalize(torch.randn((n, 3), generator=g), dim=-1).to(DEV)
    coeffs = torch.randn((n, 16, 3), generator=g).to(DEV)
    raw = torch.full((n, 3), float("nan"), device=DEV)
    typed = torch.full((n, 3), float("nan"), device=DEV)
    _raw("gsr_sh_forward", C.c_uint(n), C.c_uint(degree), C.c_uint(degree), _ptr(dirs), _ptr(coeffs), _ptr(raw),
         _stream(DEV))
    _call("gsr_sh_forward", n, degree, degree, dirs, coeffs, typed, _stream(DEV))
    torch.cuda.synchronize()
    assert torch.isfinite(raw).all() and raw.abs().max() > 0
    assert torch.equal(raw, typed)


def test_l1_forward_raw_and_typed_agree():
    """A 12 x 13 x 3 image: 468 values, no multiple of 4 (the tail), a `long long` and a `float` parameter."""
    from rasterizer.cuda import _call, _ptr, _stream

    g = torch.Generator().manual_seed(4)
    pred = (torch.rand((12, 13, 3), generator=g) * 1.2).to(DEV)  # some values above the clamp
    gt = torch.rand((12, 13, 3), generator=g).to(DEV)
    weight, sums_slots = 0.8, 64  # GSR_LOSS_SUM_SLOTS
    out = []
    for typed in (False, True):
        sums = torch.full((sums_slots,), float("nan"), dtype=torch.float64, device=DEV)
        loss = torch.full((1,), float("nan"), device=DEV)
        if typed:
            _call("gsr_l1_forward", pred.numel(), weight, 1, pred, gt, sums, loss, _stream(DEV))
        else:
            _raw("gsr_l1_forward", C.c_longlong(pred.numel()), C.c_float(weight), C.c_int(1), _ptr(pred), _ptr(gt),
                 _ptr(sums), _ptr(loss), _stream(DEV))
        out.append(loss)
    torch.cuda.synchronize()
    expected = weight * (pred.clamp(max=1.0) - gt).abs().double().mean()
    assert abs(out[0].item() - expected.item()) < 1e-6
    assert torch.equal(out[0], out[1])
