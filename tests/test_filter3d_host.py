"""The 3D smoothing filter on the host: the restatements of tests/filter3d_reference.py against
float64 and torch.autograd, baking, the interface and the checkpoint.  No GPU."""
import inspect
import os

import numpy as np
import pytest
import torch

import filter3d_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
NEW_ENTRIES = ("gsr_filter3d_sampling", "gsr_activate_filtered_forward", "gsr_activate_filtered_backward")


# ---- the sampling restatement against float64 -----------------------------------------------------------------------
@pytest.mark.parametrize("n,nv,seed", [(1000, 7, 0), (257, 33, 1), (4000, 2, 2)])
def test_sampling_restatement_against_float64(n, nv, seed):
    """float32 `seen` decisions equal the float64 ones on every pair that is clear of a threshold (at most 1 % of the
    pairs are not), and with the decisions agreed the filters match to 1e-5 relative."""
    means, cams = R.sampling_case(n, nv, seed)
    table = R.camera_table(cams)
    got = R.sampling(means, table, dtype=F32)
    ref = R.sampling(means, table, dtype=F64)
    robust = R.robust_pairs(ref, table)
    left_out = 1.0 - robust.mean()
    disagree = got["seen"] != ref["seen"]
    print(f"N={n} V={nv}: {100 * left_out:.3f} % of the pairs within 1e-4 of a threshold, "
          f"{int(disagree.sum())} decisions differ, {int((disagree & robust).sum())} of them on clear pairs; "
          f"seen pairs {int(ref['seen'].sum())}, Gaussians seen by none {int((ref['nu'] == 0).sum())}")
    assert left_out <= 0.01
    assert not (disagree & robust).any()
    assert ref["seen"].any() and (~ref["seen"]).any()
    # the values, under the float32 decisions: rows all of whose decisions agree, the fallback included
    val = R.sampling(means, table, dtype=F64, seen_override=got["seen"])
    rows = ~disagree.any(axis=1)
    rel = np.abs(got["filter"][rows].astype(F64) - val["filter"][rows]) / val["filter"][rows]
    print(f"  filter: worst relative difference {rel.max():.3e} over {int(rows.sum())} rows")
    assert rows.sum() >= 0.98 * n and (val["filter"][rows] > 0).all() and rel.max() <= 1e-5


def test_sampling_restatement_edges():
    means, cams = R.sampling_case(257, 2, 3)
    table = R.camera_table(cams)
    got = R.sampling(means, table)
    k = R.filter_constant()
    assert k == F32(np.sqrt(0.2)) and got["filter"].dtype == F32
    seen = got["nu"] > 0
    assert np.array_equal(got["filter"][seen], (k / got["nu"][seen]).astype(F32))
    # a Gaussian no camera sees, the NaN centre among them, takes the largest filter of any seen one
    assert (~seen).any() and not seen[5] and np.isnan(means[5]).all()
    assert (got["filter"][~seen] == got["filter"][seen].max()).all()
    # nothing seen: all zeros
    means, cams = R.unseen_case(100, 3)
    none = R.sampling(means, R.camera_table(cams))
    assert not none["seen"].any() and (none["filter"] == 0).all()


# ---- the activation restatement -------------------------------------------------------------------------------------
def _torch_reference(case):
    """torch.autograd over gs_fused.apply_filter_3d in float64."""
    from gs_fused import apply_filter_3d

    t = lambda a: torch.from_numpy(np.asarray(a, F64))  # noqa: E731
    l, q, a = (t(case[k]).requires_grad_(True) for k in ("log_scales", "raw_quats", "logits"))
    s, o = apply_filter_3d(torch.exp(l), torch.sigmoid(a), t(case["filter"]))
    quats = q / q.norm(dim=-1, keepdim=True)
    loss = (s * t(case["v_scales"])).sum() + (o * t(case["v_opac"])).sum() + (quats * t(case["v_quats"])).sum()
    g_l, g_q, g_a = torch.autograd.grad(loss, (l, q, a))
    return {"scales": s, "quats": quats, "opacities": o, "v_log_scales": g_l, "v_raw_quats": g_q, "v_logits": g_a}


@pytest.mark.parametrize("n,seed", [(1, 0), (65, 1), (1000, 2)])
def test_activation_restatement_against_autograd(n, seed):
    case = R.activation_case(n, seed)
    ours = R.activation(case["log_scales"], case["raw_quats"], case["logits"], case["filter"], case["v_scales"],
                        case["v_quats"], case["v_opac"], dtype=F64)
    want = _torch_reference(case)
    for key, ref in want.items():
        e = R.rel_error(ours[key], ref.detach().numpy())
        print(f"N={n} {key}: e = {e:.3e}")
        assert ours[key].shape == tuple(ref.shape) and e <= 1e-12, key
    if n >= 65:  # the case spans what the bound is for: f >> s (c ~ (s/f)^3) and f << s, and rows without a filter
        c = ours["opacities"][:, 0] * (1.0 + np.exp(-case["logits"][:, 0].astype(F64)))
        assert c.min() < 1e-9 and c[case["filter"] > 0].max() > 0.999 and (case["filter"] == 0).sum() >= n // 3


@pytest.mark.parametrize("dtype", [F32, F64])
def test_a_zero_filter_is_plain_exp_and_sigmoid(dtype):
    case = R.activation_case(300, 4)
    zero = np.zeros(300, F32)
    out = R.activation(case["log_scales"], case["raw_quats"], case["logits"], zero, case["v_scales"], None,
                       case["v_opac"], dtype=dtype)
    l, a = case["log_scales"].astype(dtype), case["logits"].astype(dtype)
    s = np.exp(l).astype(dtype)
    o = (dtype(1) / (dtype(1) + np.exp(-a).astype(dtype))).astype(dtype)
    assert np.array_equal(out["scales"], s) and np.array_equal(out["opacities"], o)
    assert np.array_equal(out["v_log_scales"], case["v_scales"].astype(dtype) * s)
    assert np.array_equal(out["v_logits"], (case["v_opac"].astype(dtype) * o) * (dtype(1) - o))
    assert not out["v_raw_quats"].any()  # a missing cotangent is zero
    # and a mixed case keeps those bits on its zero rows
    mixed = R.activation(case["log_scales"], case["raw_quats"], case["logits"], case["filter"], case["v_scales"], None,
                         case["v_opac"], dtype=dtype)
    rows = case["filter"] == 0
    assert rows.any() and (~rows).any()
    for key in ("scales", "opacities", "v_log_scales", "v_logits"):
        assert np.array_equal(mixed[key][rows], out[key][rows]), key
        assert not np.array_equal(mixed[key][~rows], out[key][~rows]), key


def test_apply_filter_3d_sends_no_gradient_to_the_filter_and_checks_shapes():
    from gs_fused import apply_filter_3d

    s = torch.rand(5, 3, dtype=torch.float64, requires_grad=True)
    o = torch.rand(5, 1, dtype=torch.float64, requires_grad=True)
    f = torch.rand(5, dtype=torch.float64, requires_grad=True)
    s2, o2 = apply_filter_3d(s, o, f)
    assert s2.shape == (5, 3) and o2.shape == (5, 1) and (s2 > s).all() and (o2 < o).all()
    (s2.sum() + o2.sum()).backward()
    assert f.grad is None and s.grad is not None and o.grad is not None
    assert apply_filter_3d(s, o[:, 0], f)[1].shape == (5,)
    with pytest.raises(ValueError, match="apply_filter_3d"):
        apply_filter_3d(s, o, f[:4])
    with pytest.raises(ValueError, match="apply_filter_3d"):
        apply_filter_3d(s[:, :2], o, f)


# ---- baking ---------------------------------------------------------------------------------------------------------
def test_baked_parameters_activate_to_the_filtered_model():
    """exp / sigmoid of the baked float32 parameters against the filtered activations of the raw ones, in float64.
    Scales: 1e-6 relative on every element (l' is stored to |l'| 2^-24 <= 9.3 * 6e-8).  Opacities: 1e-6 of the largest,
    and on every row |a'| 2^-23 relative: d ln sigmoid(a') / d a' = 1 - o' <= 1 and a' is stored to |a'| 2^-24, so that
    is twice what the storage alone costs -- below 1e-6 wherever |a'| < 8.4; where c ~ (s/f)^3 ~ exp(-36) the logit is
    ~ -40 and no float32 logit holds the opacity to 1e-6 of its value."""
    from gs_fused import bake_filter_3d

    case = R.activation_case(2000, 5)
    l32, a32, f32 = (torch.from_numpy(case[k]) for k in ("log_scales", "logits", "filter"))
    bl, ba = bake_filter_3d(l32, a32, f32)
    assert bl.dtype == torch.float32 and ba.dtype == torch.float32 and bl.shape == l32.shape and ba.shape == a32.shape
    want = R.activation(case["log_scales"], case["raw_quats"], case["logits"], case["filter"], dtype=F64)
    s = np.exp(bl.numpy().astype(F64))
    o = 1.0 / (1.0 + np.exp(-ba.numpy().astype(F64)))
    rel_s = (np.abs(s - want["scales"]) / want["scales"]).max()
    e_o = R.rel_error(o, want["opacities"])
    rel_o = np.abs(o - want["opacities"]) / want["opacities"]
    bound_o = np.abs(ba.numpy().astype(F64)) * 2.0 ** -23 + 1e-12  # (1e-12: the float64 arithmetic on either side)
    print(f"baked: scales worst relative {rel_s:.3e}, opacities e = {e_o:.3e}, worst row {rel_o.max():.3e} relative, "
          f"{(rel_o / bound_o).max():.3f} of its bound; logits from {ba.min():.1f} to {ba.max():.1f}")
    assert rel_s <= 1e-6 and e_o <= 1e-6
    assert (want["opacities"] > 0).all() and (rel_o <= bound_o).all()
    assert float(ba.min()) < -30 and (np.abs(ba.numpy()) * 2.0 ** -23 < 1e-6).mean() > 0.5  # both regimes occur
    # rows without a filter keep their raw parameters
    rows = f32 == 0
    assert rows.any() and torch.equal(bl[rows], l32[rows]) and torch.equal(ba[rows], a32[rows])
    with pytest.raises(ValueError, match="bake_filter_3d"):
        bake_filter_3d(l32, a32, f32[:-1])


def test_the_exported_ply_is_the_baked_model(tmp_path):
    import harness.train as HT
    from gs_fused import bake_filter_3d
    from gs_io.ply import read_gaussian_ply

    model = HT.GaussianParams(HT.blob_scene(50, seed=3, sh_degree=1), torch.device("cpu"))
    raw = HT.export_parameters(model)
    assert all(np.array_equal(raw[k], model.gauss[k].detach().numpy()) for k in HT.PARAM_NAMES)
    model.filter_3d = torch.linspace(0.0, 0.5, 50)
    baked = HT.export_parameters(model)
    bl, ba = bake_filter_3d(model.gauss["scales"].detach(), model.gauss["opacities"].detach(), model.filter_3d)
    assert np.array_equal(baked["scales"], bl.numpy()) and np.array_equal(baked["opacities"], ba.numpy())
    assert not np.array_equal(baked["scales"], raw["scales"]) and np.array_equal(baked["means"], raw["means"])
    assert all(np.array_equal(HT.export_parameters(model, bake_filter=False)[k], raw[k]) for k in HT.PARAM_NAMES)
    # the file's layout does not change
    from gs_io import write_gaussian_ply

    write_gaussian_ply(str(tmp_path / "a.ply"), raw)
    write_gaussian_ply(str(tmp_path / "b.ply"), baked)
    assert os.path.getsize(tmp_path / "a.ply") == os.path.getsize(tmp_path / "b.ply")
    back = read_gaussian_ply(str(tmp_path / "b.ply"))
    assert np.array_equal(back["scales"], baked["scales"]) and np.array_equal(back["opacities"], baked["opacities"])


# ---- interface ------------------------------------------------------------------------------------------------------
def test_the_entries_are_declared_and_exported():
    from rasterizer.cuda import _backend

    src = open(os.path.join(ROOT, "include", "gsraster.h")).read()
    for s in NEW_ENTRIES:
        assert s + "(" in src and s in _backend.SYMBOLS and hasattr(_backend.lib(), s), s
    assert _backend.PROTOTYPES["gsr_filter3d_sampling"] == ("i", "ipipfffppp")
    assert _backend.PROTOTYPES["gsr_activate_filtered_forward"] == ("i", "i" + "p" * 11)
    assert _backend.PROTOTYPES["gsr_activate_filtered_backward"] == ("i", "i" + "p" * 12)
    import gs_fused
    from gs_fused import filter3d

    for name in ("filter_cameras", "sampling_filter_3d", "apply_filter_3d", "bake_filter_3d", "activate_gaussians"):
        assert callable(getattr(gs_fused, name)), name
    assert f"#define GSR_FILTER3D_WORKSPACE_BYTES {filter3d.WORKSPACE_BYTES}\n" in src


def test_the_new_keywords_default_to_off():
    import gs_fused
    import harness.train as HT

    assert inspect.signature(gs_fused.activate_gaussians).parameters["filter_3d"].default is None
    sig = inspect.signature(gs_fused.sampling_filter_3d).parameters
    assert (sig["variance"].default, sig["near"].default, sig["margin"].default) == (0.2, 0.2, 0.15)
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("variance", "near", "margin", "out"))
    assert sig["out"].default is None
    cfg = HT.TrainConfig()
    assert cfg.filter_3d is False and cfg.filter_3d_every == 100
    assert HT.GaussianParams.filter_3d is None and "filter_3d" not in HT.PARAM_NAMES


def test_filter_cameras_from_either_camera_type():
    from gs_fused import filter_cameras
    from harness import scene as S
    from harness.pipeline import CameraTensors

    cams = [S.make_camera(128, 96, yaw=0.1), S.make_camera(200, 120, fov_x_deg=45.0, pitch=-0.2, trans=(0.1, 0, 0.3))]
    a = filter_cameras(cams, "cpu")
    b = filter_cameras([CameraTensors.from_numpy(c, "cpu") for c in cams], "cpu")
    assert a.shape == (2, 20) and a.dtype == torch.float32 and torch.equal(a, b)
    assert np.array_equal(a.numpy(), R.camera_table(cams))
    for v, c in enumerate(cams):
        assert np.array_equal(a[v, :12].numpy(), c.viewmat[:3].reshape(12))
        assert a[v, 12:18].tolist() == [F32(x) for x in (c.fx, c.fy, c.cx, c.cy, c.width, c.height)]
    assert filter_cameras([], "cpu").shape == (0, 20)


def test_cpu_tensors_are_refused_by_name():
    from gs_fused import activate_gaussians, sampling_filter_3d
    from harness import scene as S

    means = torch.zeros(4, 3)
    cams = [S.make_camera(64, 48)]
    with pytest.raises(ValueError, match="sampling_filter_3d: means is a CPU tensor"):
        sampling_filter_3d(means, cams)
    with pytest.raises(ValueError, match=r"activate_gaussians\(filter_3d=\.\.\.\): log_scales is a CPU tensor"):
        activate_gaussians(None, torch.zeros(4, 3), torch.ones(4, 4), torch.zeros(4, 1), None, filter_3d=torch.ones(4))
    with pytest.raises(ValueError, match="expected scales"):  # shapes first, as without a filter
        activate_gaussians(None, torch.zeros(4, 2), torch.ones(4, 4), torch.zeros(4, 1), None, filter_3d=torch.ones(4))


@pytest.mark.parametrize("option,kw,world", [
    ("fused_render", dict(fused_render=True), 1), ("use_graph", dict(use_graph=True), 1),
    ("strategy='mcmc'", dict(strategy="mcmc"), 1), ("world size", dict(), 2),
    ("fused_activations", dict(fused_activations=False), 1), ("filter_3d_every", dict(filter_3d_every=0), 1)])
def test_the_trainer_refuses_by_option(option, kw, world):
    import harness.train as HT

    cfg = HT.TrainConfig(filter_3d=True, **kw)
    with pytest.raises(ValueError, match="filter_3d.*" + option.replace("(", r"\(")):
        HT._check_filter_3d(cfg, torch.device("cuda", 0), world)
    HT._check_filter_3d(HT.TrainConfig(**kw), torch.device("cpu"), world)  # off: nothing is refused


def test_the_trainer_refuses_cpu_tensors_and_a_cpu_model_refuses_a_filter():
    import harness.train as HT
    from harness import scene as S
    from harness.pipeline import CameraTensors

    with pytest.raises(ValueError, match="filter_3d needs CUDA tensors"):
        HT.train(HT.TrainConfig(filter_3d=True, num_gaussians=50, iters=1), torch.device("cpu"))
    for kw in (dict(fused_render=True), dict(use_graph=True)):
        with pytest.raises(ValueError, match="filter_3d"):
            HT.train(HT.TrainConfig(filter_3d=True, num_gaussians=50, iters=1, **kw), torch.device("cpu"))
    model = HT.GaussianParams(HT.blob_scene(20, seed=1, sh_degree=1), torch.device("cpu"))
    model.filter_3d = torch.ones(20)
    cam = CameraTensors.from_numpy(S.make_camera(32, 32), "cpu")
    with pytest.raises(ValueError, match="filter_3d needs fused_activations on CUDA"):
        model.render(cam, torch.zeros(3), 1)
    from harness.pipeline import contribution_stats

    with pytest.raises(ValueError, match="filter_3d needs fused_activations on CUDA"):
        contribution_stats(model, [cam], HT.TrainConfig())


# ---- checkpoint -----------------------------------------------------------------------------------------------------
def _model(n, seed):
    from harness.train import GaussianParams, blob_scene

    return GaussianParams(blob_scene(n, seed=seed, sh_degree=1), torch.device("cpu"))


def _optims(model):
    from harness.train import LRS

    return {k: torch.optim.Adam([model.gauss[k]], lr=lr, eps=1e-15) for k, lr in LRS.items()}


def test_a_checkpoint_restores_the_filter_bit_for_bit(tmp_path):
    from harness import checkpoint as CK

    a = _model(300, 1)
    a.filter_3d = torch.from_numpy(np.random.default_rng(0).uniform(0, 0.1, 300).astype(F32))
    a.filter_3d[:7] = 0.0
    path = CK.save_checkpoint(str(tmp_path), 40, a, _optims(a))
    blob = torch.load(path, map_location="cpu", weights_only=True)
    assert torch.equal(blob["pipeline"]["_model.filter_3d"], a.filter_3d)
    b = _model(80, 2)
    b.filter_3d = torch.ones(80)
    assert CK.load_checkpoint(path, b, _optims(b)) == 41
    assert b.num_points == 300 and b.filter_3d.dtype == torch.float32 and torch.equal(b.filter_3d, a.filter_3d)
    assert "filter_3d" not in dict(b.named_parameters()) and all("filter" not in k for k, _ in b.named_parameters())


def test_a_checkpoint_without_a_filter_still_loads(tmp_path):
    from harness import checkpoint as CK

    a = _model(120, 3)
    path = CK.save_checkpoint(str(tmp_path), 7, a, _optims(a))
    blob = torch.load(path, map_location="cpu", weights_only=True)
    assert set(blob["pipeline"]) == {"_model.gauss_params." + k for k in CK.PARAM_NAMES}
    b = _model(120, 4)
    assert CK.load_checkpoint(path, b, _optims(b)) == 8 and b.filter_3d is None
    assert all(torch.equal(b.gauss[k], a.gauss[k]) for k in CK.PARAM_NAMES)
    c = _model(50, 5)  # a buffer of another size does not survive the resize
    c.filter_3d = torch.ones(50)
    CK.load_checkpoint(path, c, _optims(c))
    assert c.num_points == 120 and c.filter_3d is None


def test_export_gaussians_bakes_unless_told_not_to(tmp_path, capsys):
    import json
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import export_gaussians as G
    from gs_fused import bake_filter_3d
    from gs_io.ply import read_gaussian_ply
    from harness import checkpoint as CK

    a = _model(90, 6)
    a.filter_3d = torch.linspace(0.0, 0.3, 90)
    path = CK.save_checkpoint(str(tmp_path), 3, a, _optims(a))
    bl, ba = bake_filter_3d(a.gauss["scales"].detach(), a.gauss["opacities"].detach(), a.filter_3d)
    G.main([path, str(tmp_path / "baked.ply"), "--device", "cpu"])
    assert json.loads(capsys.readouterr().out.strip())["filter_3d"] == "baked"
    baked = read_gaussian_ply(str(tmp_path / "baked.ply"))
    assert np.array_equal(baked["scales"], bl.numpy()) and np.array_equal(baked["opacities"], ba.numpy())
    G.main([path, str(tmp_path / "raw.ply"), "--device", "cpu", "--no-bake-filter"])
    assert json.loads(capsys.readouterr().out.strip())["filter_3d"].startswith("left out")
    raw = read_gaussian_ply(str(tmp_path / "raw.ply"))
    assert np.array_equal(raw["scales"], a.gauss["scales"].detach().numpy())
    assert np.array_equal(raw["opacities"], a.gauss["opacities"].detach().numpy())
    assert torch.equal(G.checkpoint_filter_3d(path), a.filter_3d)
