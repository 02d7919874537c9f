"""GPU: the equidistant fisheye projection (csrc/project.hip behind the FISH flag, gs_fused.project_gaussians_fisheye,
DESIGN.md section 4.23) against the float64 restatement of tests/fisheye_reference.py on the cases of
tests/fisheye_cases.py, against the pinhole op on the optical axis, end to end through `render_view`, the trainer and
the dataset tools.

Forward: integer outputs equal on every row the reference does not flag; float outputs per row within 4 x the error
of the float32 evaluation of the same reference plus 1e-6 of the row's magnitude (the project's standing rule).
Backward: 1e-3 of the row's largest magnitude, the bar tests/test_gpu_projection.py sets for the pinhole backward."""
import functools
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import fisheye_cases as FC
import fisheye_reference as FR
import projection_cases as PC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD = ("cov3d", "xys", "depths", "radii", "conics", "compensation", "num_tiles_hit")
BWD = ("v_cov2d", "v_cov3d", "v_mean3d", "v_scale", "v_quat")


def cu(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def npy(t):
    return None if t is None else t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(float64 reference, its float32 evaluation) of a case: computed once, read-only."""
    c, _ = FC.case(name)
    kw = {"cov3d": c.cov3d} if c.precomputed else {}
    return (FR.project_forward_fisheye_fp64(*FC.reference_args(c), **kw),
            FR.project_forward_fisheye_fp64(*FC.reference_args(c), dtype=np.float32, **kw))


def gpu_forward(c, opacities=None, entry="fisheye"):
    import rasterizer.cuda as C

    a = [cu(x) if isinstance(x, np.ndarray) else x for x in c.forward_args()]
    if entry == "pinhole":
        return dict(zip(FWD, (npy(t) for t in C.project_gaussians_forward(*a))))
    kw = {"cov3d_precomp": cu(c.cov3d)} if c.precomputed else {}
    out = C.project_gaussians_forward_fisheye(*a, opacities=cu(opacities), **kw)
    res = dict(zip(FWD, (npy(t) for t in out[:7])))
    res["opacities_aa"] = npy(out[7])
    return res


def gpu_backward(c, o, cot, opacities=None, v_opacities_aa=None, entry="fisheye"):
    import rasterizer.cuda as C

    sq = (None, None) if c.precomputed else (cu(c.scales), cu(c.quats))
    head = (c.n, cu(c.means3d), sq[0], c.glob_scale, sq[1], cu(c.viewmat[:3]), cu(c.projmat), c.fx, c.fy, c.cx, c.cy,
            c.H, c.W, cu(o["cov3d"]), cu(o["radii"]), cu(o["conics"]), cu(o["compensation"]))
    if entry == "pinhole":
        return dict(zip(BWD, (npy(t) for t in C.project_gaussians_backward(*head, *(cu(v) for v in cot)))))
    out = C.project_gaussians_backward_fisheye(*head, cu(opacities), *(cu(v) for v in cot), cu(v_opacities_aa))
    res = dict(zip(BWD, (npy(t) for t in out[:5])))
    res["v_opacities"] = npy(out[5])
    return res


def _forward_against(name, o, r64, r32, rows, what):
    """Integers equal on unflagged rows; floats within 4 x the float32 reference's error + 1e-6 of the row."""
    ok = rows & ~r64["ambiguous"]
    for k in ("radii", "num_tiles_hit"):
        bad = ok & (o[k] != r64[k])
        assert not bad.any(), f"{name} {what} {k}: {int(bad.sum())} unflagged rows differ, first {np.flatnonzero(bad)[:5]}"
    both = ok & r64["visible"] & (o["radii"] > 0)
    for k in FR.OUTPUTS:
        e, e32, m = FR.row_err(o[k], r64[k]), FR.row_err(r32[k], r64[k]), FR.row_max(r64[k])
        over = both & (e > 4.0 * e32 + 1e-6 * m)
        worst = float((e[both] / (4.0 * e32[both] + 1e-6 * m[both] + 1e-300)).max()) if both.any() else 0.0
        print(f"{name} {what} {k}: {int(both.sum())} rows, worst error / bound {worst:.3f}, "
              f"worst relative error {float((e[both] / np.maximum(m[both], 1e-30)).max()) if both.any() else 0.0:.3e}")
        assert not over.any(), f"{name} {what} {k}: {int(over.sum())} rows beyond the bound, first {np.flatnonzero(over)[:5]}"


# ---- 1. forward against float64 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FC.names())
def test_forward_against_float64(name):
    (c, groups), (r64, r32) = FC.case(name), reference(name)
    handed = c.cov3d.copy() if c.precomputed else None
    o = gpu_forward(c)
    if c.precomputed:
        assert np.array_equal(o["cov3d"], handed)  # the caller's, untouched
    for k in FWD:
        assert np.isfinite(o[k]).all(), f"{name} {k}: NaN or infinity"
    for g in ("on_axis", "near_axis_1e-20"):  # r = 0 and r^2 underflowing, by name
        if g in groups:
            s = groups[g]
            assert all(np.isfinite(o[k][s]).all() for k in FWD), g
            assert (o["radii"][s] > 0).all(), g
    cul = o["radii"] == 0
    for k in FWD + (() if c.precomputed else ()):
        if not (c.precomputed and k == "cov3d"):
            assert not o[k][cul].any(), f"{name} {k}: a culled row is not all zeros"
    if "tz_is_clip" in groups:  # tz == clip exactly is culled (`<=`); these rows are flagged by construction
        assert cul[groups["tz_is_clip"]].all()
    if "behind" in groups:
        assert cul[groups["behind"]].all()
    unplanned = r64["ambiguous"].copy()
    if "tz_is_clip" in groups:
        unplanned[groups["tz_is_clip"]] = False
    print(f"{name}: {c.n} rows, visible {r64['visible'].mean():.3f}, flagged {unplanned.mean():.4f}")
    assert unplanned.mean() <= 0.01 and r64["visible"].mean() >= 0.30
    _forward_against(name, o, r64, r32, np.ones(c.n, bool), "vs float64")


# ---- 2. on-axis rows against the existing op ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["main", "exact"])
def test_on_axis_rows_equal_the_pinhole_op(name):
    (c, groups), (r64, r32) = FC.case(name), reference(name)
    rows = np.zeros(c.n, bool)
    rows[groups["on_axis"]] = True
    fish, pin = gpu_forward(c), gpu_forward(c, entry="pinhole")
    assert (pin["radii"][rows] > 0).all() and (fish["radii"][rows] > 0).all()
    ok = rows & ~r64["ambiguous"]
    for k in ("radii", "num_tiles_hit"):
        assert np.array_equal(fish[k][ok], pin[k][ok]), k
    for k in FR.OUTPUTS:
        # the two ops against each other, under the bound each is held to against float64
        e, e32, m = FR.row_err(fish[k], pin[k].astype(np.float64)), FR.row_err(r32[k], r64[k]), FR.row_max(r64[k])
        over = ok & (e > 4.0 * e32 + 1e-6 * m)
        print(f"{name} on-axis {k}: worst |fisheye - pinhole| / row {float((e[ok] / np.maximum(m[ok], 1e-30)).max()):.3e}")
        assert not over.any(), f"{k}: {int(over.sum())} on-axis rows differ from the pinhole op"
    _forward_against(name, pin, r64, r32, rows, "pinhole op vs fisheye float64")


# ---- 3. backward against float64 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["main", "exact", "near_plane", "needles", "precomputed", "blockedge-257"])
def test_backward_against_float64(name):
    (c, groups), (r64, _) = FC.case(name), reference(name)
    o = gpu_forward(c)
    cot = PC.cotangents(c)
    hip = gpu_backward(c, o, cot)
    sq = (None, None) if c.precomputed else (c.scales, c.quats)
    f64 = FR.project_vjp_fisheye_fp64(c.means3d, sq[0], c.glob_scale, sq[1], c.viewmat[:3], c.projmat, c.fx, c.fy, c.cx,
                                      c.cy, c.H, c.W, o["compensation"], *cot, clip_thresh=c.clip,
                                      cov3d=c.cov3d if c.precomputed else None)
    vis = o["radii"] > 0
    assert vis.sum() >= 0.3 * c.n
    if c.precomputed:
        assert hip["v_scale"] is None and hip["v_quat"] is None  # the chain ends at v_cov3d
    failures = []
    for nm, f in zip(("v_mean3d", "v_cov3d") if c.precomputed else ("v_mean3d", "v_scale", "v_quat"), f64):
        h = hip[nm]
        assert np.isfinite(h).all(), nm
        assert not h[~vis].any(), f"{nm}: a culled row has a gradient"
        rowmax = np.abs(f).max(axis=-1, keepdims=True)
        e = (np.abs(h - f) / np.maximum(rowmax, 1e-6 * np.abs(f[vis]).max())).max(axis=-1)
        for g, s in groups.items():
            v = vis[s]
            if v.any():
                print(f"{name} {nm} {g}: {int(v.sum())} rows, worst per-row error {float(e[s][v].max()):.3e}")
                if e[s][v].max() >= 1e-3:
                    failures.append((nm, g, float(e[s][v].max())))
    assert not failures, failures
    for k in ("v_cov2d", "v_cov3d"):
        assert not hip[k][~vis].any(), k


@pytest.mark.parametrize("name", ["main", "precomputed"])
def test_a_null_cotangent_is_a_zero_cotangent(name):
    c, _ = FC.case(name)
    o = gpu_forward(c)
    cot = PC.cotangents(c)
    for k in range(4):
        null = gpu_backward(c, o, tuple(None if j == k else v for j, v in enumerate(cot)))
        zero = gpu_backward(c, o, tuple(np.zeros_like(v) if j == k else v for j, v in enumerate(cot)))
        for nm in BWD:
            assert (null[nm] is None and zero[nm] is None) or np.array_equal(null[nm], zero[nm]), (k, nm)
    none = gpu_backward(c, o, (None, None, None, None))
    assert all(none[nm] is None or not none[nm].any() for nm in BWD)


# ---- 4. the antialiased route ---------------------------------------------------------------------------------------
def test_antialiased_route():
    from gs_fused import project_gaussians_fisheye

    c, _ = FC.case("main")
    rng = np.random.default_rng(77)
    opac = rng.uniform(0.05, 0.95, (c.n, 1)).astype(np.float32)
    plain, aa = gpu_forward(c), gpu_forward(c, opacities=opac)
    for k in FWD:
        assert np.array_equal(plain[k], aa[k]), k
    assert plain["opacities_aa"] is None and aa["opacities_aa"].shape == opac.shape
    assert np.array_equal(aa["opacities_aa"], opac * plain["compensation"][:, None])  # one float32 multiply, bit for bit
    # gradients: the one node against the two-line form (tests/test_gpu_antialiased.py's bound for the pinhole pair)
    v_xy, v_depth, v_conic, v_oaa = (cu(v) for v in PC.cotangents(c))
    v_oaa = v_oaa[:, None]
    res = []
    for route in ("two lines", "one node"):
        lv = {"means": cu(c.means3d).requires_grad_(), "scales": cu(c.scales).requires_grad_(),
              "quats": cu(c.quats).requires_grad_(), "opacities": cu(opac).requires_grad_()}
        args = (lv["means"], lv["scales"], c.glob_scale, lv["quats"], cu(c.viewmat[:3]), cu(c.projmat), c.fx, c.fy, c.cx,
                c.cy, c.H, c.W, c.bw)
        if route == "two lines":
            xys, depths, radii, conics, comp, tiles, cov3d = project_gaussians_fisheye(*args)
            oaa = lv["opacities"] * comp[:, None]
        else:
            xys, depths, radii, conics, comp, tiles, cov3d, oaa = project_gaussians_fisheye(*args, opacities=lv["opacities"])
            assert oaa.shape == lv["opacities"].shape
        ((xys * v_xy).sum() + (depths * v_depth).sum() + (conics * v_conic).sum() + (oaa * v_oaa).sum()).backward()
        res.append((oaa.detach(), lv))
    assert torch.equal(res[0][0], res[1][0])
    for k in ("means", "scales", "quats", "opacities"):
        a, b = res[0][1][k].grad, res[1][1][k].grad
        assert a.abs().max().item() > 0 and torch.isfinite(b).all()
        assert (a - b).abs().max().item() <= 2e-5 * a.abs().max().item() + 1e-12, k


# ---- 5. same bits, no shared state ----------------------------------------------------------------------------------
def test_same_bits_across_calls_and_next_to_the_pinhole_entries():
    c, _ = FC.case("main")
    cot = PC.cotangents(c)
    pin0 = gpu_forward(c, entry="pinhole")
    gpin0 = gpu_backward(c, pin0, cot, entry="pinhole")
    f1 = gpu_forward(c)
    g1 = gpu_backward(c, f1, cot)
    f2 = gpu_forward(c)
    g2 = gpu_backward(c, f2, cot)
    pin1 = gpu_forward(c, entry="pinhole")
    gpin1 = gpu_backward(c, pin1, cot, entry="pinhole")
    for k in FWD:
        assert np.array_equal(f1[k], f2[k]) and np.array_equal(pin0[k], pin1[k]), k
    for k in BWD:
        assert np.array_equal(g1[k], g2[k]) and np.array_equal(gpin0[k], gpin1[k]), k
    assert not np.array_equal(f1["xys"], pin0["xys"])  # (the two cameras are two cameras)


# ---- the public op's refusals that need a GPU tensor ----------------------------------------------------------------
def test_a_camera_that_requires_a_gradient_is_refused():
    from gs_fused import project_gaussians_fisheye

    c, _ = FC.case("blockedge-255")
    base = [cu(c.means3d), cu(c.scales), 1.0, cu(c.quats), cu(c.viewmat[:3]), cu(c.projmat), c.fx, c.fy, c.cx, c.cy,
            c.H, c.W, c.bw]
    for slot, nm in ((4, "viewmat"), (5, "projmat")):
        a = list(base)
        a[slot] = a[slot].clone().requires_grad_()
        with pytest.raises(ValueError, match=nm):
            project_gaussians_fisheye(*a)
    out = project_gaussians_fisheye(*base)
    assert len(out) == 7 and out[2].dtype == torch.int32


# ---- 6. geometry end to end -----------------------------------------------------------------------------------------
def test_peaks_sit_where_the_equidistant_rule_puts_them():
    from harness import scene as S
    from harness.pipeline import CameraTensors, render_view

    phi = math.atan2((FC.H - FC.CY) * 0.9, (FC.W - FC.CX) * 0.9)  # along the image diagonal, towards the bottom right
    V = np.eye(4, dtype=np.float32)
    P = (PC._projection(0.001, 1000.0, 0.5 * FC.W / FC.FX, 0.5 * FC.H / FC.FY)).astype(np.float32)
    bg = torch.zeros(3, device=DEV)
    sh = np.zeros((1, 1, 3), np.float32)
    sh[:, 0, :] = 0.5 / S.SH_C0
    for k, deg in enumerate((0.0, 20.0, 45.0, 65.0, 74.0)):
        th = math.radians(deg)
        # the diagonal in the image: direction (cos phi', sin phi') in view space with fx theta cos phi' : fy theta sin phi'
        # on the diagonal
        pphi = math.atan2(math.sin(phi) / FC.FY, math.cos(phi) / FC.FX)
        p = 3.0 * np.array([[math.sin(th) * math.cos(pphi), math.sin(th) * math.sin(pphi), math.cos(th)]], np.float32)
        want = (FC.FX * th * math.cos(pphi) + FC.CX - 0.5, FC.FY * th * math.sin(pphi) + FC.CY - 0.5)
        args = (cu(p), cu(np.full((1, 3), 0.01, np.float32)), cu(np.float32([[1, 0, 0, 0]])), cu(np.float32([[0.99]])),
                cu(sh))
        peaks = {}
        for model in ("fisheye", "pinhole"):
            cam = CameraTensors(FC.W, FC.H, FC.FX, FC.FY, FC.CX, FC.CY, cu(V), cu(P), torch.zeros(3, device=DEV),
                                None, model)
            a = render_view(*args, cam, bg, 0)["alpha"][..., 0]
            i = int(a.argmax())
            peaks[model] = (i % FC.W, i // FC.W, float(a.max()))
        fx_, fy_, fa = peaks["fisheye"]
        print(f"{deg:4.0f} deg: expected ({want[0]:.2f}, {want[1]:.2f}), fisheye peak ({fx_}, {fy_}) alpha {fa:.3f}, "
              f"pinhole peak {peaks['pinhole']}")
        assert fa > 0.05 and abs(fx_ - want[0]) <= 1.0 and abs(fy_ - want[1]) <= 1.0
        if k >= 2:  # the pinhole camera of the same intrinsics puts it elsewhere, or off screen
            px_, py_, pa = peaks["pinhole"]
            assert pa == 0.0 or abs(px_ - want[0]) > 1.0 or abs(py_ - want[1]) > 1.0


# ---- 7. the trainer -------------------------------------------------------------------------------------------------
SMALL = dict(num_gaussians=5000, init_gaussians=2000, width=160, height=96, num_views=8, eval_views=2, iters=30,
             sh_degree=1, sh_degree_interval=10, scene_scale=(0.03, 0.15), log_every=1, cam_radius=3.0, densify=True)
VARIANTS = {"default": dict(mask="box"),
            # (the depth term from the first step on: the first and the last loss hold the same terms)
            "aa_absgrad_depth": dict(rasterize_mode="antialiased", absgrad=True, model="co-gs",
                                     depth_loss_start_iteration=-1)}
# ONE refinement inside the run, the densification of step 12: a step is due every 3, densifies where step % 30 >
# num_views + 3 and step < 13 (gs_fused.refinement_branch); the opacity reset of step 3 falls inside the warm-up and
# nothing is culled after the last split.  The 17 steps behind it are what the split Gaussians need to settle: with the
# densification at step 20 of 30 both cameras' runs end above their first loss
REFINE = dict(warmup_length=3, refine_every=3, reset_alpha_every=10, stop_screen_size_at=30, stop_split_at=13,
              continue_cull_post_densification=False, densify_grad_thresh=2e-5, cull_alpha_thresh=0.05)
_runs = {}


def _train(variant, model, again=False):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_trajectory as TT

    import harness.train as HT
    from gs_fused import RefineConfig
    from rasterizer import rasterize as R

    key = (variant, model, again)
    if key not in _runs:
        was = R.is_deterministic()
        R.set_deterministic(True)
        try:
            res = HT.train(HT.TrainConfig(refine=RefineConfig(**REFINE), sharded_adam=False, camera_model=model,
                                          **SMALL, **VARIANTS[variant]), torch.device("cuda", 0))
        finally:
            R.set_deterministic(was)
        # the bytes tools/train_trajectory.py prints: everything but the timings, floats as hex
        _runs[key] = (res, json.dumps({k: TT._hex(v) for k, v in res.items()
                                       if k not in TT.TIMING and not k.startswith("phase_")}, sort_keys=True))
    return _runs[key]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_trainer_on_a_fisheye_scene(variant):
    (a, bytes_a), (_, bytes_b) = _train(variant, "fisheye"), _train(variant, "fisheye", again=True)
    (p, bytes_p) = _train(variant, "pinhole")
    assert a["render"] == "separate ops" and a["camera_model"] == "fisheye" and "camera_model" not in p
    assert len(a["losses"]) == 30 and all(math.isfinite(v) for v in a["losses"])
    print(f"{variant}: loss {a['losses'][0]:.5f} -> {a['losses'][-1]:.5f}, N {a['num_gaussians_start']} -> "
          f"{a['num_gaussians_end']}, PSNR {a['psnr_start']:.2f} -> {a['psnr_end']:.2f}; pinhole loss {p['losses'][0]:.5f}")
    assert a["num_gaussians_end"] > a["num_gaussians_start"] and len(a["refinements"]) == 1
    assert a["losses"][-1] < a["losses"][0]
    assert bytes_a == bytes_b
    assert a["losses"][0] != p["losses"][0] and bytes_a != bytes_p


# ---- 8. dataset round trip ------------------------------------------------------------------------------------------
def test_dataset_round_trip(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_synthetic_dataset as MSD
    import train_dataset as TD

    import harness.train as HT
    from gs_io.dataset import load_dataset

    data = str(tmp_path / "fisheye")
    meta = MSD.make_synthetic_dataset(data, views=6, width=96, height=64, device="cuda", camera_model="OPENCV_FISHEYE")
    assert meta["camera_model"] == "OPENCV_FISHEYE" and meta["k1"] == 0.0
    with pytest.raises(ValueError, match="camera_model"):
        load_dataset(data, "train")
    assert load_dataset(data, "train", allow_fisheye=True).camera_model == "fisheye"
    res = TD.main([data, "--iters", "10", "--output-dir", str(tmp_path / "out"), "--sh-degree", "1", "--num-downscales", "0",
                   "--eval-mode", "interval", "--eval-interval", "3"])
    assert res["camera_model"] == "fisheye" and len(res["losses"]) == 10
    held = res["dataset"]["heldout"]
    print(f"held-out PSNR {held['psnr']:.3f} over {held['num_images']} images")
    assert held["num_images"] == 2 and math.isfinite(held["psnr"]) and math.isfinite(held["ssim"])
    # ... and `evaluate_dataset` on its own, from the model a second short run leaves behind
    model = HT.GaussianParams(HT._hidden_scene(HT.TrainConfig(num_gaussians=600, sh_degree=1, scene_scale=(0.03, 0.15))),
                              torch.device(DEV))
    cfg = HT.TrainConfig(dataset=data, sh_degree=1, dataset_eval_mode="interval", dataset_eval_interval=3,
                         dataset_allow_fisheye=True)
    ev = HT.evaluate_dataset(model, data, cfg, "val", torch.device(DEV))
    assert ev["num_images"] == 2 and math.isfinite(ev["psnr"]) and ev["psnr"] > 15.0  # (the scene that was rendered)
