"""The bilateral-grid rule of include/gsraster.h restated with torch's own ops on the CPU, in
whatever dtype the inputs have: float64 is the oracle of the GPU tests, float32 the baseline their tolerance is taken
from.  `grids` [V,L,Gh,Gw,12] channel last, `rgb` [H,W,3]."""
import functools

import torch
import torch.nn.functional as F

IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
GUIDE = (0.299, 0.587, 0.114)
ULP = 2.0 ** -23


def slice_ref(grids: torch.Tensor, rgb: torch.Tensor, view: int) -> torch.Tensor:
    """grid_sample(grids_channel_first[v:v+1], 2 (xyz - 0.5), bilinear, align_corners, border) + the 3x4 affine map."""
    H, W, _ = rgb.shape
    dt = rgb.dtype
    x = ((torch.arange(W, dtype=dt) + 0.5) / W)[None, :].expand(H, W)
    y = ((torch.arange(H, dtype=dt) + 0.5) / H)[:, None].expand(H, W)
    g = GUIDE[0] * rgb[..., 0] + GUIDE[1] * rgb[..., 1] + GUIDE[2] * rgb[..., 2]
    xyz = torch.stack((x, y, g), dim=-1)                       # grid_sample's order: (W, H, D) = (Gw, Gh, L)
    vol = grids[view:view + 1].permute(0, 4, 1, 2, 3)          # [1,12,L,Gh,Gw]
    m = F.grid_sample(vol, (2.0 * (xyz - 0.5))[None, None], mode="bilinear", align_corners=True, padding_mode="border")
    m = m[0, :, 0].permute(1, 2, 0).reshape(H, W, 3, 4)
    return (m[..., :3] * rgb[..., None, :]).sum(-1) + m[..., 3]


def tv_ref(grids: torch.Tensor) -> torch.Tensor:
    """sum over the axes L, Gh, Gw of mean(squared forward difference)."""
    return ((grids[:, 1:] - grids[:, :-1]) ** 2).mean() + ((grids[:, :, 1:] - grids[:, :, :-1]) ** 2).mean() + \
        ((grids[:, :, :, 1:] - grids[:, :, :, :-1]) ** 2).mean()


def identity_grids(V: int, gw: int, gh: int, gl: int, dtype=torch.float32) -> torch.Tensor:
    return torch.tensor(IDENTITY, dtype=dtype).repeat(V, gl, gh, gw, 1).contiguous()


def guide64(rgb: torch.Tensor) -> torch.Tensor:
    d = rgb.double()
    return GUIDE[0] * d[..., 0] + GUIDE[1] * d[..., 1] + GUIDE[2] * d[..., 2]


def draw_rgb(H: int, W: int, gl: int, gen: torch.Generator) -> torch.Tensor:
    """float32 [H,W,3] uniform in [-0.3, 1.4]; from three pixels on, the first pixel is drawn from [-0.3, -0.05] and the
    last from [1.05, 1.4], so that both clamps of the guide occur at every size.  A pixel whose guide times (L - 1) lies
    within 1e-3 of an integer, or whose guide lies within 1e-3 of 0 or 1, is drawn again: the guide's gradient jumps
    there, and float32 and float64 may pick different sides."""
    def draw():
        x = torch.rand((H, W, 3), generator=gen, dtype=torch.float32) * 1.7 - 0.3
        if H * W >= 3:
            x.view(-1, 3)[0] = torch.rand(3, generator=gen) * 0.25 - 0.3
            x.view(-1, 3)[-1] = torch.rand(3, generator=gen) * 0.35 + 1.05
        return x

    rgb = draw()
    for _ in range(1000):
        g = guide64(rgb)
        s = g * (gl - 1)
        bad = ((s - s.round()).abs() < 1e-3) | (g.abs() < 1e-3) | ((g - 1).abs() < 1e-3)
        if not bool(bad.any()):
            return rgb
        rgb = torch.where(bad[..., None], draw(), rgb)
    raise AssertionError("draw_rgb: could not move every pixel off the guide's kinks")


@functools.lru_cache(maxsize=4)
def slice_case(H: int, W: int, gw: int, gh: int, gl: int, view: int, V: int = 3):
    """One case of the slice tests, computed once: float32 inputs (grids, rgb, v_out) and, per dtype in (float64,
    float32), the restatement's (out, v_rgb, v_grids) on the CPU.  -> (inputs, want64, base32); nobody writes to them."""
    gen = torch.Generator().manual_seed(1000003 * H + 1009 * W + 101 * gw + 11 * gh + gl)
    grids = identity_grids(V, gw, gh, gl) + 0.25 * torch.randn((V, gl, gh, gw, 12), generator=gen)
    rgb = draw_rgb(H, W, gl, gen)
    v_out = torch.randn((H, W, 3), generator=gen)
    res = []
    for dt in (torch.float64, torch.float32):
        a = grids.to(dt).clone().requires_grad_(True)
        x = rgb.to(dt).clone().requires_grad_(True)
        out = slice_ref(a, x, view)
        out.backward(v_out.to(dt))
        res.append((out.detach(), x.grad, a.grad))
    return (grids, rgb, v_out), res[0], res[1]


def rel_err(got: torch.Tensor, want64: torch.Tensor) -> float:
    """e(X) = max |X - X64| / max |X64|."""
    top = float(want64.abs().max())
    return float((got.double().cpu() - want64).abs().max()) / (top if top > 0 else 1.0)
