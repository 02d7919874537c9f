"""CPU: the float64 restatement the GPU tests of csrc/normals.hip are held to (tests/_normals_ref.py) is pinned against
analytic planes and central differences, and the public surface of the feature -- gs_fused.gaussian_normals /
depth_to_normal / normal_consistency_loss, `render_view(render_normals=...)`, the trainer's option -- is checked as far
as it goes without a GPU: every refusal raises what it states."""
import math

import pytest
import torch

import _normals_ref as R
from gs_fused import depth_to_normal, gaussian_normals, normal_consistency_loss
from gs_fused.normals import workspace_doubles

F64 = torch.float64
K = (41.0, 43.5, 16.3, 11.8)


# ---- the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b,c", [(0.0, 0.0, 2.5), (0.35, -0.2, 3.0), (-0.5, 0.45, 1.7)],
                         ids=["fronto-parallel", "tilted", "tilted-back"])
def test_restatement_returns_an_analytic_planes_normal(a, b, c):
    """The plane a x + b y + z = c seen through pixel rays (xn, yn, 1) has depth z = c / (1 + a xn + b yn), written in
    the module's docstring form with -a, -b; its unit normal facing the camera is -(a, b, 1) / |(a, b, 1)|."""
    H, W = 23, 31
    fx, fy, cx, cy = K
    xn = (torch.arange(W, dtype=F64) + 0.5 - cx) / fx
    yn = (torch.arange(H, dtype=F64) + 0.5 - cy) / fy
    depth = c / (1 + a * xn[None, :] + b * yn[:, None])
    assert float(depth.min()) > 0
    normals, valid = R.depth_normals(depth, torch.ones(H, W, dtype=F64), *K)
    want = -torch.tensor([a, b, 1.0], dtype=F64) / math.sqrt(a * a + b * b + 1)
    assert int(valid.sum()) == (H - 2) * (W - 2) and not bool(valid[0].any()) and not bool(valid[:, -1].any())
    err = float((normals[valid] - want).abs().max())
    print(f"plane ({a}, {b}, {c}): max error {err:.3g}")
    assert err <= 1e-12
    assert not bool(normals[~valid].any())
    if a == 0.0 and b == 0.0:
        assert torch.equal(normals[valid], torch.tensor([0.0, 0.0, -1.0], dtype=F64).expand(int(valid.sum()), 3))


def test_restatement_validity_rule():
    H, W = 7, 9
    depth = torch.full((H, W), 2.0, dtype=F64)
    alpha = torch.ones(H, W, dtype=F64)
    alpha[3, 4] = 0.0              # a hole: the pixel and its four neighbours lose their normal, the diagonals keep it
    depth[1, 1] = float("inf")     # a non-finite depth does the same
    alpha[5, 7] = -0.5
    _, valid = R.depth_normals(depth, alpha, *K)
    want = torch.zeros(H, W, dtype=torch.bool)
    want[1:-1, 1:-1] = True
    for (i, j) in ((3, 4), (1, 1), (5, 7)):
        for (di, dj) in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):
            if 0 <= i + di < H and 0 <= j + dj < W:
                want[i + di, j + dj] = False
    assert torch.equal(valid, want) and bool(valid[2, 3]) and bool(valid[4, 5])
    # an invalid pixel contributes m * 1: all-invalid images give exactly mean(m)
    for shape in ((1, 1), (2, 2), (2, 5)):
        m = torch.rand(*shape, dtype=F64)
        loss = R.normal_consistency_loss(torch.rand(*shape, 3, dtype=F64), torch.ones(shape, dtype=F64),
                                         torch.ones(shape, dtype=F64), *K, mask=m)
        assert float(loss) == float(m.mean())


def _central_differences(f, x, h):
    g = torch.zeros_like(x)
    flat, gf = x.view(-1), g.view(-1)
    for k in range(flat.numel()):
        old = float(flat[k])
        flat[k] = old + h
        up = float(f())
        flat[k] = old - h
        dn = float(f())
        flat[k] = old
        gf[k] = (up - dn) / (2 * h)
    return g


def test_restatement_gradients_agree_with_central_differences():
    case = R.image_case(6, 7, 5, True)
    depth, nimg = case["depth"].double(), case["nimg"].double()
    f = lambda: R.normal_consistency_loss(nimg, depth, case["alpha"], *case["K"], mask=case["mask"])  # noqa: E731
    d, n = depth.clone().requires_grad_(True), nimg.clone().requires_grad_(True)
    R.normal_consistency_loss(n, d, case["alpha"], *case["K"], mask=case["mask"]).backward()
    _, valid = R.depth_normals(depth, case["alpha"], *case["K"])
    assert int(valid.sum()) >= 3 and bool(d.grad.abs().max() > 0)
    for name, x, got in (("depth", depth, d.grad), ("normals_img", nimg, n.grad)):
        fd = _central_differences(f, x, 1e-6)
        err = float((fd - got).abs().max()) / float(got.abs().max())
        print(f"d loss / d {name}: central differences differ by {err:.3g} of the largest entry")
        assert err < 1e-6
    g, _ = R.gaussian_case(12, 9)
    q = g["quats"].double()
    w = torch.randn(12, 3, dtype=F64, generator=torch.Generator().manual_seed(1))
    fq = lambda: (R.gaussian_normals(q, g["scales"], g["means"], g["viewmat"])[0] * w).sum()  # noqa: E731
    qq = q.clone().requires_grad_(True)
    (R.gaussian_normals(qq, g["scales"], g["means"], g["viewmat"])[0] * w).sum().backward()
    for row in range(12):  # (per row: the quaternions' norms, and with them the gradients, span six decades)
        h = 1e-6 * float(q[row].norm())
        fd = _central_differences(fq, q[row], h)
        err = float((fd - qq.grad[row]).abs().max()) / float(qq.grad[row].abs().max())
        assert err < 1e-5, (row, err)


def test_restatement_gaussian_normals_by_hand():
    V = torch.eye(4)[:3]
    q = torch.tensor([[2.0, 0.0, 0.0, 0.0], [math.sqrt(0.5), math.sqrt(0.5), 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]])
    s = torch.tensor([[1.0, 1.0, 0.01], [0.5, 0.5, 0.7], [-3.0, -1.0, -2.0]])
    m = torch.tensor([[0.0, 0.0, 3.0], [0.0, 1.0, 3.0], [1.0, 0.0, 3.0]])
    n, axis, _ = R.gaussian_normals(q, s, m, V)
    assert axis.tolist() == [2, 0, 0]  # the smallest; a tie goes to the lowest index; log-scales by value
    assert torch.allclose(n[0], torch.tensor([0.0, 0.0, -1.0], dtype=F64))       # z axis, turned to the camera
    assert torch.allclose(n[1], torch.tensor([1.0, 0.0, 0.0], dtype=F64))        # n . p == 0: not negated
    assert torch.allclose(n[2], torch.tensor([-1.0, 0.0, 0.0], dtype=F64))       # n . p > 0: negated
    assert torch.equal(R.smallest_axis(s), R.smallest_axis(s.exp()))


def test_input_generators_meet_their_conditions():
    for n in (1, 63, 64, 65, 1000):
        case, rounds = R.gaussian_case(n, 200 + n)
        assert rounds < 64
        norms = case["quats"].double().norm(dim=-1)
        assert float(norms.min()) >= 0.999e-3 and float(norms.max()) <= 1.001e3
        srt = case["scales"].sort(dim=-1).values
        assert bool((srt[case["tied"], 0] == srt[case["tied"], 1]).all())
        if n == 1000:
            assert int(case["tied"].sum()) == 100 and bool((case["scales"] < 0).any()) and bool((case["scales"] > 0).any())
    case = R.image_case(17, 33, 1, False)
    assert float(case["depth"].min()) >= 1 and float(case["depth"].max()) <= 5
    a = case["alpha"]
    assert bool(((a == 0) | ((a > 0.2) & (a <= 1))).all()) and 0.03 < float((a == 0).float().mean()) < 0.2


# ---- the public surface ----------------------------------------------------------------------------------------------
def test_workspace_size_follows_the_header_macro():
    assert [workspace_doubles(*s) for s in ((1, 1), (16, 16), (17, 33), (1080, 1920))] == [1, 1, 6, 68 * 120]


def test_shape_errors_are_value_errors_and_come_first():
    z = torch.zeros
    with pytest.raises(ValueError, match="quats"):
        gaussian_normals(z(5, 3), z(5, 3), z(5, 3), z(3, 4))
    with pytest.raises(ValueError, match="scales"):
        gaussian_normals(z(5, 4), z(4, 3), z(5, 3), z(3, 4))
    with pytest.raises(ValueError, match="means"):
        gaussian_normals(z(5, 4), z(5, 3), z(5, 2), z(3, 4))
    with pytest.raises(ValueError, match="viewmat"):
        gaussian_normals(z(5, 4), z(5, 3), z(5, 3), z(12))
    with pytest.raises(ValueError, match="depth"):
        depth_to_normal(z(4, 5, 2), z(4, 5), *K)
    with pytest.raises(ValueError, match="depth"):
        depth_to_normal(z(0, 5), z(0, 5), *K)
    with pytest.raises(ValueError, match="alpha"):
        depth_to_normal(z(4, 5), z(5, 4), *K)
    with pytest.raises(ValueError, match="fx"):
        depth_to_normal(z(4, 5), z(4, 5), 0.0, 1.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="normals_img"):
        normal_consistency_loss(z(4, 5), z(4, 5), z(4, 5), *K)
    with pytest.raises(ValueError, match="alpha"):
        normal_consistency_loss(z(4, 5, 3), z(4, 5, 1), z(4, 6), *K)
    with pytest.raises(ValueError, match="mask"):
        normal_consistency_loss(z(4, 5, 3), z(4, 5), z(4, 5), *K, mask=z(5, 4))
    with pytest.raises(ValueError, match="mask"):  # (a shape error wins over the CPU tensors it comes with)
        normal_consistency_loss(z(4, 5, 3), z(4, 5), z(4, 5), *K, mask=z(4, 5, 2))
    with pytest.raises(ValueError, match="2\\^31"):
        big = z(1).expand(1 << 15, 1 << 15)  # (a view of one element: 3 H W = 3 * 2^30)
        depth_to_normal(big, big, *K)


def test_cpu_tensors_and_other_types_are_runtime_errors():
    z = torch.zeros
    with pytest.raises(RuntimeError, match="CUDA"):
        gaussian_normals(z(5, 4), z(5, 3), z(5, 3), z(3, 4))
    with pytest.raises(RuntimeError, match="CUDA"):
        gaussian_normals(z(0, 4), z(0, 3), z(0, 3), z(4, 4))
    with pytest.raises(RuntimeError, match="CUDA"):
        depth_to_normal(z(4, 5), z(4, 5, 1), *K)
    with pytest.raises(RuntimeError, match="CUDA"):
        normal_consistency_loss(z(4, 5, 3), z(4, 5), z(4, 5), *K)
    with pytest.raises(RuntimeError, match="CUDA"):
        normal_consistency_loss(z(4, 5, 3), z(4, 5, 1), z(4, 5, 1), *K, mask=z(4, 5, 1))
    with pytest.raises(RuntimeError, match="tensor"):
        gaussian_normals([[1.0, 0, 0, 0]], z(1, 3), z(1, 3), z(3, 4))
    with pytest.raises(RuntimeError, match="tensor"):
        depth_to_normal(z(4, 5), None, *K)
    with pytest.raises(RuntimeError, match="tensor"):
        normal_consistency_loss(z(4, 5, 3), z(4, 5), z(4, 5), *K, mask=1.0)


def test_trainer_refusals_name_the_option():
    from harness.train import TrainConfig, _check_normal_consistency

    cpu, cuda = torch.device("cpu"), torch.device("cuda:0")
    _check_normal_consistency(TrainConfig(), cpu, 2)  # off: nothing to refuse
    _check_normal_consistency(TrainConfig(normal_consistency=True), cuda, 1)
    _check_normal_consistency(TrainConfig(normal_consistency=True, model="co-gs"), cuda, 1)
    for kw, dev, world, what in (({"fused_render": True}, cuda, 1, "fused_render"), ({"use_graph": True}, cuda, 1, "use_graph"),
                                 ({}, cuda, 2, "world size"), ({}, cpu, 1, "CUDA")):
        with pytest.raises(ValueError, match=what) as info:
            _check_normal_consistency(TrainConfig(normal_consistency=True, **kw), dev, world)
        assert "normal_consistency" in str(info.value)
    cfg = TrainConfig()
    assert (cfg.normal_consistency, cfg.normal_lambda, cfg.normal_start_iteration) == (False, 0.05, 7000)
    from harness.train import train

    with pytest.raises(ValueError, match="normal_consistency"):
        train(TrainConfig(normal_consistency=True, iters=1), cpu)


def test_train_dataset_tool_takes_the_option():
    import importlib.util
    import os

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "train_dataset.py")
    spec = importlib.util.spec_from_file_location("train_dataset_tool", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.parse_args(["DATA", "--normal-consistency", "--normal-lambda", "0.1", "--normal-start", "500"])
    assert (a.normal_consistency, a.normal_lambda, a.normal_start) == (True, 0.1, 500)
    a = mod.parse_args(["DATA"])
    assert (a.normal_consistency, a.normal_lambda, a.normal_start) == (False, 0.05, 7000)


def test_the_default_render_returns_the_dictionary_it_always_did(monkeypatch):
    import cpu_standins as SI
    import harness.pipeline as HP
    from harness import scene as S

    monkeypatch.setattr(HP, "project_gaussians", SI.project_gaussians)
    monkeypatch.setattr(HP, "spherical_harmonics", SI.spherical_harmonics)
    monkeypatch.setattr(HP, "rasterize_gaussians", SI.rasterize_gaussians)
    cam_np = S.make_camera(32, 24)
    sc = S.make_scene(40, cam_np, sh_degree=1, seed=3, scale_lo=0.05, scale_hi=0.2)
    cam = HP.CameraTensors.from_numpy(cam_np, "cpu")
    t = {k: torch.from_numpy(v) for k, v in sc.items()}
    args = (t["means3d"], t["scales"], t["quats"], t["opacities"], t["sh_coeffs"], cam, torch.tensor(S.BACKGROUND), 1)
    keys = {"rgb", "alpha", "depth", "depth_acc", "xys", "radii", "depths", "conics", "num_tiles_hit", "rgbs"}
    assert set(HP.render_view(*args)) == keys
    assert set(HP.render_view(*args, render_normals=False, render_depth=True)) == keys
    assert set(HP.render_view(*args, render_normals=True)) == keys  # (no depth image: no normal pass)
    with pytest.raises(RuntimeError, match="CUDA"):  # asked for: the native normals, which take no CPU tensors
        HP.render_view(*args, render_depth=True, render_normals=True)
