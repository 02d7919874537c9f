"""GPU: the 3D smoothing filter (csrc/filter3d.hip, gs_fused.filter3d) -- the sampling pass bit for
bit against the float32 restatement, the filtered activations against float64 under the project's rule

    e(X) = max|X - X64| / max|X64|  <=  4 * (the float32 restatement's e) + 2^-23,

rows without a filter bit for bit against the unfiltered kernels, a small view end to end and the trainer."""
import numpy as np
import pytest
import torch

import filter3d_reference as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
IMAGE_PARITY = 1e-4  # the project's image parity bound, absolute


def dev():
    return torch.device("cuda", 0)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def same_bits(a: torch.Tensor, b) -> bool:
    b = b if isinstance(b, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(b))
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


# ---- the sampling pass ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", [1, 2, 7, 33])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_sampling_pass_equals_the_float32_restatement(n, nv):
    from gs_fused import filter_cameras, sampling_filter_3d

    means, cams = R.sampling_case(n, nv, seed=n + nv)
    table = filter_cameras(cams, dev())
    assert same_bits(table, R.camera_table(cams))
    want = R.sampling(means, R.camera_table(cams))
    if n >= 63:  # by construction, and checked: every branch of the rule occurs
        z, u, w, seen = want["z"], want["u"], want["w"], want["seen"]
        W, H = R.camera_table(cams)[None, :, 16], R.camera_table(cams)[None, :, 17]
        outside_image = (u < 0) | (u > W) | (w < 0) | (w > H)
        assert (z < 0).any() and z[0, 0] < 0                            # behind a camera
        assert ((z > 0) & (z <= R.NEAR)).any() and 0 < z[1, 0] <= R.NEAR  # in front, not beyond near
        assert (seen & outside_image).any() and seen[2, 0] and outside_image[2, 0]  # inside the margin band
        assert ((z > R.NEAR) & ~seen).any() and z[3, 0] > R.NEAR and not seen[3, 0]  # outside the band
        assert want["nu"][4] == 0 and np.isfinite(means[4]).all() and (want["nu"] > 0).any()  # seen by none: fallback
        assert np.isnan(means[5]).all() and want["nu"][5] == 0          # a NaN centre
        assert want["filter"][4] == want["filter"][5] == want["filter"].max() > 0
    got = sampling_filter_3d(cu(means), table)
    assert got.shape == (n,) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), torch.from_numpy(want["filter"])), (got.cpu().numpy() - want["filter"])
    # the same from the sequence of cameras, and with other constants
    assert torch.equal(sampling_filter_3d(cu(means), cams), got)
    other = sampling_filter_3d(cu(means), table, variance=0.35, near=0.6, margin=0.02)
    assert torch.equal(other.cpu(), torch.from_numpy(R.sampling(means, R.camera_table(cams), 0.35, 0.6, 0.02)["filter"]))


def test_sampling_pass_a_scene_no_camera_sees_is_all_zeros():
    from gs_fused import sampling_filter_3d

    means, cams = R.unseen_case(300, 3)
    assert not R.sampling(means, R.camera_table(cams))["seen"].any()
    got = sampling_filter_3d(cu(means), cams, out=torch.full((300,), 7.0, device=dev()))
    assert got.shape == (300,) and not bool(got.any())


def test_sampling_pass_empty_inputs_and_out():
    from gs_fused import filter_cameras, sampling_filter_3d

    means, cams = R.sampling_case(65, 2, 1)
    table = filter_cameras(cams, dev())
    empty = sampling_filter_3d(torch.zeros((0, 3), device=dev()), table)
    assert empty.shape == (0,) and empty.dtype == torch.float32 and empty.is_cuda
    with pytest.raises(ValueError, match="sampling_filter_3d: cameras holds no camera"):
        sampling_filter_3d(cu(means), table[:0])
    with pytest.raises(ValueError, match="sampling_filter_3d: cameras holds no camera"):
        sampling_filter_3d(cu(means), [])
    with pytest.raises(ValueError, match="sampling_filter_3d: means must be float32"):
        sampling_filter_3d(cu(means).double(), table)
    with pytest.raises(ValueError, match="sampling_filter_3d: cameras must be float32"):
        sampling_filter_3d(cu(means), table[:, :18])
    with pytest.raises(ValueError, match="sampling_filter_3d: out must be"):
        sampling_filter_3d(cu(means), table, out=torch.zeros(64, device=dev()))
    with pytest.raises(ValueError, match="sampling_filter_3d: need variance > 0"):
        sampling_filter_3d(cu(means), table, near=0.0)
    out = torch.full((65,), float("nan"), device=dev())
    ptr = out.data_ptr()
    back = sampling_filter_3d(cu(means), table, out=out)
    assert back is out and out.data_ptr() == ptr
    assert torch.equal(out.cpu(), torch.from_numpy(R.sampling(means, R.camera_table(cams))["filter"]))


def test_the_entry_rejects_before_any_launch():
    from rasterizer.cuda import _call, _stream

    means, cams = R.sampling_case(65, 2, 1)
    m, table = cu(means), cu(R.camera_table(cams))
    out = torch.full((65,), 3.0, device=dev())
    ws = torch.zeros(4, dtype=torch.int32, device=dev())
    k = float(R.filter_constant())
    with pytest.raises(RuntimeError, match="num_cameras must be positive"):
        _call("gsr_filter3d_sampling", 65, m, 0, table, k, 0.2, 0.15, out, ws, _stream(dev()))
    with pytest.raises(RuntimeError, match="null pointer"):
        _call("gsr_filter3d_sampling", 65, m, 2, None, k, 0.2, 0.15, out, ws, _stream(dev()))
    shifted = torch.zeros(2 * 20 + 4, device=dev())[1:41].reshape(2, 20)  # 4 bytes off the allocation's alignment
    assert shifted.data_ptr() % 16 == 4
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        _call("gsr_filter3d_sampling", 65, m, 2, shifted, k, 0.2, 0.15, out, ws, _stream(dev()))
    _call("gsr_filter3d_sampling", 0, None, 0, None, k, 0.2, 0.15, None, None, _stream(dev()))  # N = 0: returns at once
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())


def test_sampling_pass_is_bit_reproducible():
    from gs_fused import sampling_filter_3d

    means, cams = R.sampling_case(1000, 7, 5)
    first = sampling_filter_3d(cu(means), cams).clone()
    # (a large scratch allocation filled with NaN and released: what torch.empty hands out next is not zeros)
    scratch = torch.full(((64 << 20) // 4,), float("nan"), device=dev())
    del scratch
    second = sampling_filter_3d(cu(means), cams)
    assert same_bits(first, second) and torch.equal(first.cpu(), torch.from_numpy(R.sampling(means, R.camera_table(cams))["filter"]))


# ---- the filtered activation ----------------------------------------------------------------------------------------
def _run_activation(case, filt, cotangents=("v_scales", "v_quats", "v_opac"), with_dirs=True):
    """gs_fused.activate_gaussians on the case -> outputs and the three gradients (None for a filter: unfiltered)."""
    from gs_fused import activate_gaussians

    l, q, a = (cu(case[k]).requires_grad_(True) for k in ("log_scales", "raw_quats", "logits"))
    kw = {} if filt is None else {"filter_3d": cu(filt)}
    scales, quats, opac, dirs = activate_gaussians(cu(case["means"]), l, q, a, cu(case["campos"]) if with_dirs else None,
                                                   **kw)
    outs = {"v_scales": scales, "v_quats": quats, "v_opac": opac}
    loss = sum((outs[k] * cu(case[k])).sum() for k in cotangents)
    g_l, g_q, g_a = torch.autograd.grad(loss, (l, q, a), allow_unused=True)
    return {"scales": scales.detach(), "quats": quats.detach(), "opacities": opac.detach(), "viewdirs": dirs,
            "v_log_scales": g_l, "v_raw_quats": g_q, "v_logits": g_a}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_filtered_activation_against_float64(n):
    case = R.activation_case(n, seed=n)
    got = _run_activation(case, case["filter"])
    plain = _run_activation(case, None)
    args = (case["log_scales"], case["raw_quats"], case["logits"], case["filter"], case["v_scales"], case["v_quats"],
            case["v_opac"])
    ref, twin = R.activation(*args, dtype=F64), R.activation(*args, dtype=F32)
    failed = []
    for key in ("scales", "quats", "opacities", "v_log_scales", "v_raw_quats", "v_logits"):
        assert got[key].shape == ref[key].shape and got[key].dtype == torch.float32, key
        e32 = R.rel_error(twin[key], ref[key])
        e = R.rel_error(got[key].cpu().numpy(), ref[key])
        bound = 4.0 * e32 + 2.0 ** -23
        print(f"N={n} {key}: e = {e:.3e}, float32 restatement {e32:.3e}, bound {bound:.3e}")
        if not e <= bound:
            failed.append(key)
    assert not failed, failed
    # exact: rows without a filter carry the unfiltered call's bits, outputs and all three gradients
    rows = torch.from_numpy(case["filter"] == 0)
    if n >= 3:
        assert rows.any() and (~rows).any()
    for key in ("scales", "opacities", "v_log_scales", "v_logits"):
        assert same_bits(got[key][rows], plain[key][rows]), key
        if n >= 3:
            assert not torch.equal(got[key][~rows], plain[key][~rows]), key
    # exact: quaternions, their gradient and the view directions on every row
    for key in ("quats", "v_raw_quats", "viewdirs"):
        assert same_bits(got[key], plain[key]), key
    assert got["viewdirs"].shape == (n, 3) and not got["viewdirs"].requires_grad


def test_filtered_activation_missing_cotangents_and_no_directions():
    case = R.activation_case(65, seed=9)
    full = _run_activation(case, case["filter"])
    only_s = _run_activation(case, case["filter"], cotangents=("v_scales",), with_dirs=False)
    assert only_s["viewdirs"] is None
    assert not bool(only_s["v_raw_quats"].any()) and not bool(only_s["v_logits"].any())
    ref = R.activation(case["log_scales"], case["raw_quats"], case["logits"], case["filter"], case["v_scales"],
                       dtype=F64)
    assert R.rel_error(only_s["v_log_scales"].cpu().numpy(), ref["v_log_scales"]) <= 1e-5
    only_o = _run_activation(case, case["filter"], cotangents=("v_opac",))
    assert not bool(only_o["v_raw_quats"].any()) and bool(only_o["v_log_scales"][torch.from_numpy(case["filter"] > 0)].any())
    assert not bool(only_o["v_log_scales"][torch.from_numpy(case["filter"] == 0)].any())
    assert same_bits(only_o["v_logits"], full["v_logits"])
    only_q = _run_activation(case, case["filter"], cotangents=("v_quats",))
    assert not bool(only_q["v_log_scales"].any()) and not bool(only_q["v_logits"].any())
    assert same_bits(only_q["v_raw_quats"], full["v_raw_quats"])
    # an all-zero filter is the unfiltered call on every row
    zero = _run_activation(case, np.zeros(65, F32))
    plain = _run_activation(case, None)
    for key in zero:
        assert same_bits(zero[key], plain[key]), key


def test_the_filtered_opacity_is_what_is_announced(monkeypatch):
    """`rasterizer.ahead.announce_opacity` receives the tensor the projection that follows composites with: the
    FILTERED opacity the call returns, not sigmoid(logits)."""
    import rasterizer.ahead as AH
    from gs_fused import activate_gaussians

    seen = []
    monkeypatch.setattr(AH, "announce_opacity", seen.append)
    case = R.activation_case(65, seed=3)
    l, q, a = (cu(case[k]) for k in ("log_scales", "raw_quats", "logits"))
    _, _, opac, _ = activate_gaussians(None, l, q, a, None, filter_3d=cu(case["filter"]))
    assert len(seen) == 1 and seen[0] is opac
    on = torch.from_numpy(case["filter"] > 0)
    _, _, raw, _ = activate_gaussians(None, l, q, a)
    assert len(seen) == 2 and seen[1] is raw  # (without a filter: sigmoid(logits), as before)
    # (c <= 1, and = 1 in float32 where f is far below every scale: never above, below on most rows)
    assert bool((opac[on] <= raw[on]).all()) and float((opac[on] < raw[on]).float().mean()) > 0.5
    assert torch.equal(opac[~on], raw[~on])


def test_filtered_activation_refusals():
    from gs_fused import activate_gaussians

    case = R.activation_case(8, 0)
    l, q, a = (cu(case[k]) for k in ("log_scales", "raw_quats", "logits"))
    with pytest.raises(ValueError, match=r"filter_3d must be float32 \[8\]"):
        activate_gaussians(None, l, q, a, None, filter_3d=torch.ones(7, device=dev()))
    with pytest.raises(ValueError, match=r"filter_3d must be float32 \[8\]"):
        activate_gaussians(None, l, q, a, None, filter_3d=torch.ones(8, device=dev(), dtype=torch.float64))
    with pytest.raises(ValueError, match="filter_3d is a CPU tensor"):
        activate_gaussians(None, l, q, a, None, filter_3d=torch.ones(8))


# ---- end to end, small ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_view():
    import harness.train as HT
    from harness import scene as S
    from harness.pipeline import CameraTensors

    cam_np = S.make_camera(64, 48, yaw=0.1, pitch=-0.05)
    raw = S.make_scene(300, cam_np, sh_degree=1, seed=11, scale_lo=0.005, scale_hi=0.08)
    params = {"means": raw["means3d"], "scales": np.log(raw["scales"]).astype(F32), "quats": raw["quats"],
              "opacities": np.log(raw["opacities"] / (1 - raw["opacities"])).astype(F32).reshape(-1, 1),
              "features_dc": np.ascontiguousarray(raw["sh_coeffs"][:, 0, :]),
              "features_rest": np.ascontiguousarray(raw["sh_coeffs"][:, 1:, :])}
    model = HT.GaussianParams({k: np.ascontiguousarray(v, F32) for k, v in params.items()}, dev())
    return model, CameraTensors.from_numpy(cam_np, dev()), cam_np, cu(np.array(S.BACKGROUND, F32))


def test_render_with_a_zero_filter_is_the_unfiltered_render(small_view):
    model, cam, _, bg = small_view
    with torch.no_grad():
        model.filter_3d = None
        plain = model.render(cam, bg, 1)["rgb"]
        model.filter_3d = torch.zeros(model.num_points, device=dev())
        zero = model.render(cam, bg, 1)["rgb"]
        model.filter_3d = None
    assert plain.shape == (48, 64, 3) and torch.equal(plain, zero)


def test_filtered_render_against_torch_ops_and_the_baked_model(small_view):
    import harness.train as HT
    from gs_fused import activate_gaussians, apply_filter_3d, bake_filter_3d, sampling_filter_3d
    from harness.pipeline import render_view

    model, cam, cam_np, bg = small_view
    g = {k: v.detach() for k, v in model.gauss.items()}
    # the view's own sampling rate at a quarter of its resolution: a filter of a few pixels
    filt = sampling_filter_3d(g["means"], [HT.rescale_camera(cam_np, 4)])
    assert bool((filt > 0).all())
    coeffs = (g["features_dc"], g["features_rest"])
    with torch.no_grad():
        s_k, q_k, o_k, dirs = activate_gaussians(g["means"], g["scales"], g["quats"], g["opacities"], cam.campos,
                                                 filter_3d=filt)
        s_0, q_0, o_0, _ = activate_gaussians(g["means"], g["scales"], g["quats"], g["opacities"], cam.campos)
        s_t, o_t = apply_filter_3d(s_0, o_0, filt)
        e_s = R.rel_error(s_k.cpu().numpy(), s_t.double().cpu().numpy())
        e_o = R.rel_error(o_k.cpu().numpy(), o_t.double().cpu().numpy())
        args = (g["scales"].cpu().numpy(), g["quats"].cpu().numpy(), g["opacities"].cpu().numpy(), filt.cpu().numpy())
        ref, twin = R.activation(*args, dtype=F64), R.activation(*args, dtype=F32)
        tol = max(4.0 * R.rel_error(twin[k], ref[k]) + 2.0 ** -23 for k in ("scales", "opacities"))
        print(f"kernel against apply_filter_3d: scales e = {e_s:.3e}, opacities e = {e_o:.3e}; the activation bound "
              f"here {tol:.3e}")
        assert e_s <= 2 * tol and e_o <= 2 * tol  # (both sides are float32: each within `tol` of float64)
        img_k = render_view(g["means"], s_k, q_k, o_k, coeffs, cam, bg, 1, viewdirs=dirs)["rgb"]
        img_t = render_view(g["means"], s_t, q_0, o_t, coeffs, cam, bg, 1, viewdirs=dirs)["rgb"]
        img_0 = render_view(g["means"], s_0, q_0, o_0, coeffs, cam, bg, 1, viewdirs=dirs)["rgb"]
        model.filter_3d = filt
        img_m = model.render(cam, bg, 1)["rgb"]
        model.filter_3d = None
        bl, ba = bake_filter_3d(g["scales"], g["opacities"], filt)
        baked = HT.GaussianParams({k: (bl if k == "scales" else ba if k == "opacities" else v).cpu().numpy()
                                   for k, v in g.items()}, dev())
        img_b = baked.render(cam, bg, 1)["rgb"]
    d_t, d_b = float((img_k - img_t).abs().max()), float((img_k - img_b).abs().max())
    d_0 = float((img_k - img_0).abs().max())
    print(f"images: kernel against torch ops {d_t:.3e}, against the baked model {d_b:.3e}; the filter moves the image "
          f"by {d_0:.3e}")
    assert torch.equal(img_m, img_k)         # Model.render passes the buffer on
    assert d_0 > 100 * IMAGE_PARITY          # the filter matters in this view
    # kernel against torch ops: the tolerance the activations are held to, printed above; the baked model (float32
    # storage of l' and a'): the project's image bound
    assert d_t <= tol, (d_t, tol)
    assert d_b <= IMAGE_PARITY


# ---- the trainer ----------------------------------------------------------------------------------------------------
def _train_cfg(**kw):
    from gs_fused import RefineConfig
    from harness.train import TrainConfig

    rcfg = RefineConfig(warmup_length=10, refine_every=10, reset_alpha_every=6, stop_screen_size_at=200,
                        stop_split_at=60, densify_grad_thresh=0.0002)
    base = dict(num_gaussians=2000, width=160, height=96, num_views=4, iters=41, sh_degree=1, sh_degree_interval=12,
                densify=True, refine=rcfg, num_downscales=1, resolution_schedule=12, filter_3d=True, filter_3d_every=15,
                save_every=40)
    base.update(kw)
    return TrainConfig(**base)


def _run(tmp, name, **kw):
    """One training run in deterministic mode -> (the record, the tensors of its last checkpoint)."""
    from harness import checkpoint as CK
    from harness.train import train
    from rasterizer import rasterize as RZ

    d = tmp / name
    was = RZ.is_deterministic()
    RZ.set_deterministic(True)
    try:
        res = train(_train_cfg(checkpoint_dir=str(d), **kw), dev())
    finally:
        RZ.set_deterministic(was)
    saved = torch.load(CK.latest_checkpoint(str(d)), map_location="cpu", weights_only=True)
    return res, saved


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("filter3d")
    return tmp, _run(tmp, "a")


def _same_state(a, b):
    pa, pb = a["pipeline"], b["pipeline"]
    return set(pa) == set(pb) and all(same_bits(pa[k], pb[k]) for k in pa)


def test_trainer_refines_and_the_buffer_follows(trained):
    import harness.train as HT
    from gs_fused import sampling_filter_3d

    _, (res, saved) = trained
    print(f"refinements {res['refinements']}, filter_3d {res['filter_3d']}, PSNR {res['psnr_start']:.2f} -> "
          f"{res['psnr_end']:.2f}")
    assert res["render"] == "separate ops" and saved["step"] == 40
    steps = [s for s, _ in res["refinements"]]
    assert steps and set(steps) <= {20, 30, 40} and 40 in steps and res["num_gaussians_end"] != 2000
    # before step 0; steps 0, 15, 30 (step 0 once); the change of factor at step 12; every refinement that moved rows
    assert res["filter_3d"] == {"every": 15, "updates": 4 + len(steps)}
    means, filt = saved["pipeline"]["_model.gauss_params.means"], saved["pipeline"]["_model.filter_3d"]
    assert filt.shape == (res["num_gaussians_end"],) == (means.shape[0],) and filt.dtype == torch.float32
    # the checkpoint of step 40 was written after that step's refinement: the buffer is a fresh pass over the new means
    data = HT.make_data(_train_cfg(), dev())
    fresh = sampling_filter_3d(means.to(dev()), data.cams_by_d[1])
    assert same_bits(filt, fresh) and bool((filt > 0).all())
    assert np.isfinite(res["param_checksum"]) and all(np.isfinite(v) for v in res["losses"])


def test_trainer_two_runs_produce_the_same_bytes(trained):
    tmp, (res, saved) = trained
    again, saved2 = _run(tmp, "b")
    assert again["refinements"] == res["refinements"] and again["param_checksum"] == res["param_checksum"]
    assert _same_state(saved, saved2)


def test_trainer_the_filter_changes_the_run(trained):
    tmp, (res, saved) = trained
    off, saved_off = _run(tmp, "off", filter_3d=False)
    assert "filter_3d" not in off and "_model.filter_3d" not in saved_off["pipeline"]
    assert off["param_checksum"] != res["param_checksum"] and off["psnr_start"] != res["psnr_start"]


def test_trainer_save_and_resume_reproduces_the_uninterrupted_run(trained):
    tmp, (res, saved) = trained
    half, mid = _run(tmp, "c", iters=21, save_every=20)
    assert mid["step"] == 20 and "_model.filter_3d" in mid["pipeline"]
    rest, end = _run(tmp, "d", resume_from=str(tmp / "c"))
    assert rest["start_step"] == 21 and end["step"] == 40
    assert rest["num_gaussians_end"] == res["num_gaussians_end"] and _same_state(saved, end)
