"""The degree-3 SH forward that leaves LDS to kernels on another stream (`GSR_SH_SHARE_CU`, include/gsraster.h;
`sh16_fwd_light_kernel`, csrc/sh.hip) against `sh16_fwd_kernel<4>` through the same entry: the same bits."""
import pytest
import torch

import rasterizer.cuda as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    """NaNs in the same places, every other value equal to the last bit."""
    nan = torch.isnan(a)
    assert torch.equal(nan, torch.isnan(b))
    assert torch.equal(_bits(a)[~nan], _bits(b)[~nan])


NARROW = C.SH_SHARE_CU | C.SH_NARROW
# (the narrow grid has 512 waves of 64 rows: above 32768 rows a wave takes a second run, the last one a partial one)
CASES = [(n, C.SH_SHARE_CU) for n in (1, 63, 64, 65, 4097)] + [(n, NARROW) for n in (1, 63, 64, 65, 4097, 32768 + 65)]


@pytest.mark.parametrize("use", [0, 1, 2, 3])
@pytest.mark.parametrize("n,flags", CASES)
def test_light_forward_equals_the_heavy_one_bit_for_bit(n, flags, use):
    gen = torch.Generator(device="cpu").manual_seed(1000 * n + use)
    dirs = torch.randn(n, 3, generator=gen)
    coeffs = torch.randn(n, 16, 3, generator=gen)
    zero_row, big_row = n - 1, 0
    dirs[zero_row] = 0.0  # NaN in the bands 1 .. `use`, nothing at use == 0
    first_unused = (use + 1) ** 2
    sign = torch.where(torch.arange(3 * (16 - first_unused)) % 2 == 0, 1.0, -1.0).reshape(-1, 3)
    coeffs[big_row, first_unused:] = 1e30 * sign  # (empty at use == 3)
    tame = coeffs.clone()
    tame[big_row, first_unused:] = 0.0
    dirs, coeffs, tame = dirs.to(DEV), coeffs.to(DEV), tame.to(DEV)
    assert coeffs.data_ptr() % 16 == 0

    heavy = C.compute_sh_forward(n, 3, use, dirs, coeffs)
    light = C.compute_sh_forward(n, 3, use, dirs, coeffs, flags=flags)
    torch.cuda.synchronize()
    _same_bits(light, heavy)
    # the zero direction: NaN exactly where a band above 0 is in use
    assert bool(torch.isnan(light[zero_row]).all()) == (use >= 1)
    if n > 1:
        assert torch.isfinite(light[:zero_row]).all()
    # the unused bands do not leak
    _same_bits(light, C.compute_sh_forward(n, 3, use, dirs, tame, flags=flags))
    if n > 1:
        assert light[big_row].abs().max() < 1e3


def test_the_flag_changes_nothing_at_other_degrees_or_alignments():
    gen = torch.Generator(device="cpu").manual_seed(5)
    n = 300
    dirs = torch.randn(n, 3, generator=gen).to(DEV)
    for degree, K in ((0, 1), (1, 4), (2, 9), (4, 25)):
        coeffs = torch.randn(n, K, 3, generator=gen).to(DEV)
        _same_bits(C.compute_sh_forward(n, degree, degree, dirs, coeffs, flags=NARROW),
                   C.compute_sh_forward(n, degree, degree, dirs, coeffs))
    # degree 3 at a 4-byte offset: the dword kernel, with or without the flag
    store = torch.randn(n * 48 + 1, generator=gen).to(DEV)
    odd = store[1:].view(n, 16, 3)
    assert odd.data_ptr() % 16 != 0
    _same_bits(C.compute_sh_forward(n, 3, 3, dirs, odd, flags=C.SH_SHARE_CU), C.compute_sh_forward(n, 3, 3, dirs, odd))
    with pytest.raises(RuntimeError):  # the narrow grid is a grid of the kernel that shares
        C.compute_sh_forward(n, 3, 3, dirs, odd, flags=C.SH_NARROW)
