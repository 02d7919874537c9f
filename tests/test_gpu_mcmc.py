"""GPU: the MCMC densification kernels (csrc/mcmc.hip through gs_fused.mcmc) against the float64 / Python-integer
restatement of tests/mcmc_reference.py, and the trainer's `strategy="mcmc"`.

Plan, draws and data movement are compared bit for bit (the restatement is fed the kernel's own `opac` by-product);
the float64 relocation values to "equal to, or the float32 neighbour of, the reference rounded to float32"."""
import math

import numpy as np
import pytest
import torch

import mcmc_reference as MR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
MIN_OPACITY = 0.005


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def npy(t):
    return t.detach().cpu().numpy()


def neighbour_ok(got: np.ndarray, ref64: np.ndarray) -> np.ndarray:
    r = np.asarray(ref64, np.float64).astype(F32)
    return (got == r) | (got == np.nextafter(r, F32(np.inf))) | (got == np.nextafter(r, F32(-np.inf)))


def ulp32(x):
    x = np.abs(np.asarray(x, np.float64)).astype(F32)
    return (np.nextafter(x, F32(np.inf)) - x).astype(np.float64)


# ---- (a) relocation values ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raw", (False, True))
def test_relocation_kernel_against_float64(raw):
    from gs_fused import relocation

    os_ = [0.005, 0.2, 0.8, 0.999, 1 - 1e-6]
    ns = [1, 2, 3, 8, 51, 60]
    o = np.array([a for a in os_ for _ in ns], F32)
    n = np.array([b for _ in os_ for b in ns], np.int32)
    s = np.random.default_rng(0).uniform(1e-3, 2.0, (len(o), 3)).astype(F32)
    got_o, got_s = (npy(t) for t in relocation(cu(o), cu(s), cu(n), min_opacity=0.0, raw=raw))
    ref_o, ref_s = MR.relocation(o, s, n, 0.0, raw=raw)
    assert neighbour_ok(got_o, ref_o).all(), (got_o, ref_o)
    assert neighbour_ok(got_s, ref_s).all()
    if not raw:  # ratio 1: the inputs, unchanged
        one = n == 1
        assert np.array_equal(got_o[one], o[one]) and np.array_equal(got_s[one], s[one])
    # the lower clamp
    got_c, _ = relocation(cu(o), cu(s), cu(n), min_opacity=MIN_OPACITY, raw=False)
    ref_c, _ = MR.relocation(o, s, n, MIN_OPACITY, raw=False)
    assert neighbour_ok(npy(got_c), ref_c).all() and (npy(got_c)[n > 1] >= F32(MIN_OPACITY)).all()


# ---- (b)-(d) plan, draws, apply ------------------------------------------------------------------------------------
def make_model(n, seed, dead_fraction=0.3, rest=15, moments=True, logits=None):
    rng = np.random.default_rng(seed)
    p = {"means": rng.standard_normal((n, 3)), "scales": rng.uniform(-6, -1, (n, 3)),
         "quats": rng.standard_normal((n, 4)), "features_dc": rng.standard_normal((n, 3)),
         "features_rest": rng.standard_normal((n, rest, 3)), "opacities": rng.uniform(-4.5, 4.0, (n, 1))}
    if logits is None:
        dead = rng.uniform(size=n) < dead_fraction
        p["opacities"][dead] = rng.uniform(-9.0, -5.4, (int(dead.sum()), 1))  # logit(0.005) = -5.293
    else:
        p["opacities"] = np.asarray(logits, np.float64).reshape(n, 1)
    p = {k: v.astype(F32) for k, v in p.items()}
    mom = None
    if moments:
        mom = {k: (rng.standard_normal(v.shape).astype(F32), rng.uniform(0.1, 1, v.shape).astype(F32))
               for k, v in p.items()}
    return p, mom


def to_gpu(p, mom):
    return {k: cu(v) for k, v in p.items()}, (None if mom is None else {k: (cu(a), cu(b)) for k, (a, b) in mom.items()})


def check_phase(p, mom, phase, n_new, step, seed, gp, gm, got_p, got_m, plan):
    """Compare one phase's device plan and outputs with the restatement fed the kernel's own opacities."""
    n = p["means"].shape[0]
    opac = npy(plan["opac"])
    ref64 = 1.0 / (1.0 + np.exp(-p["opacities"].astype(np.float64).reshape(-1)))
    assert (np.abs(opac.astype(np.float64) - ref64) <= 2 * ulp32(ref64)).all()
    ref_p, ref_m, pl, updated = MR.phase(p, mom, opac, MIN_OPACITY, phase, n_new, step, seed)
    total, n_dead = (int(v) for v in npy(plan["totals"]))
    assert (total, n_dead) == (pl["total"], pl["n_dead"])
    assert [int(v) for v in npy(plan["prefix"])] == pl["prefix"]
    assert npy(plan["dead_index"])[:n_dead].tolist() == pl["dead_index"]
    nd = n_dead if phase == MR.RELOCATE else n_new
    assert npy(plan["draw_source"])[:nd].tolist() == pl["draw_source"]
    assert npy(plan["row_source"]).tolist() == pl["row_source"]
    assert npy(plan["counts"]).tolist() == pl["counts"]
    # rows: everything equals the restatement bit for bit, except the float64 relocation values (neighbours allowed)
    src_rows = np.array(sorted(updated), dtype=np.int64)
    for k in MR.PARAM_NAMES:
        g = npy(got_p[k])
        assert g.shape == ref_p[k].shape, k
        if k in ("scales", "opacities") and len(src_rows):
            want = np.stack([updated[i][1] if k == "scales" else np.array([updated[i][0]]) for i in src_rows])
            assert neighbour_ok(g[src_rows], want).all(), k
            mask = np.ones(g.shape[0], bool)
            touched = np.concatenate([src_rows, np.array([r for r, _ in pl["dest"]], dtype=np.int64)])
            mask[touched] = False
            assert np.array_equal(g[mask], ref_p[k][mask]), k
        else:
            assert np.array_equal(g, ref_p[k]), k
        for r, s in pl["dest"][:2000]:  # a destination row equals its source row AFTER the update
            assert np.array_equal(g[r], g[s]), (k, r, s)
        if len(pl["dest"]):
            d = np.array(pl["dest"], dtype=np.int64)
            assert np.array_equal(g[d[:, 0]], g[d[:, 1]]), k
    if mom is None:
        assert got_m is None
    else:
        for k in MR.PARAM_NAMES:  # zero at sources and destinations, untouched elsewhere
            for a, b in zip(got_m[k], ref_m[k]):
                assert np.array_equal(npy(a), b), k
    return pl


@pytest.mark.parametrize("n", (2, 257, 4099, 70001))
def test_relocate_is_bit_exact_against_the_integer_restatement(n):
    from gs_fused import MCMCConfig, mcmc_relocate

    p, mom = make_model(n, seed=n)
    if n == 2:
        p["opacities"][:] = [[-7.0], [1.5]]
    gp, gm = to_gpu(p, mom)
    out_p, out_m, info = mcmc_relocate(gp, gm, MCMCConfig(min_opacity=MIN_OPACITY), 700, seed=11)
    assert all(out_p[k] is gp[k] for k in gp) and all(out_m[k][0] is gm[k][0] for k in gm)  # in place
    pl = check_phase(p, mom, MR.RELOCATE, 0, 700, 11, gp, gm, out_p, out_m, info.plans["relocate"])
    assert info["dead"] == pl["n_dead"] == info["relocated"] and info["added"] == 0 and pl["n_dead"] > 0
    assert info["n_out"] == n


@pytest.mark.parametrize("n,n_new", ((1, 1), (2, 3), (257, 12), (4099, 204), (70001, 3500)))
def test_add_is_bit_exact_against_the_integer_restatement(n, n_new):
    from gs_fused import MCMCConfig, mcmc_add

    p, mom = make_model(n, seed=100 + n, moments=n != 257)
    gp, gm = to_gpu(p, mom)
    before = {k: v.clone() for k, v in gp.items()}
    out_p, out_m, info = mcmc_add(gp, gm, MCMCConfig(min_opacity=MIN_OPACITY), 900, seed=5, n_new=n_new)
    assert out_p["means"].shape[0] == n + n_new == info["n_out"] and info["added"] == n_new
    assert all(torch.equal(gp[k], before[k]) for k in gp)  # the inputs are left alone
    check_phase(p, mom, MR.ADD, n_new, 900, 5, gp, gm, out_p, out_m, info.plans["add"])


def test_none_dead_leaves_every_tensor_untouched():
    from gs_fused import MCMCConfig, mcmc_refine

    p, mom = make_model(4099, seed=1, dead_fraction=0.0)
    gp, gm = to_gpu(p, mom)
    out_p, out_m, info = mcmc_refine(gp, gm, MCMCConfig(min_opacity=MIN_OPACITY, cap_max=4099), 700, seed=3)
    assert all(out_p[k] is gp[k] for k in gp) and all(out_m[k][i] is gm[k][i] for k in gm for i in (0, 1))
    assert all(np.array_equal(npy(gp[k]), p[k]) for k in p)
    assert all(np.array_equal(npy(gm[k][i]), mom[k][i]) for k in p for i in (0, 1))
    assert info.counts() == {"dead": 0, "relocated": 0, "added": 0} and "add" not in info.plans


@pytest.mark.parametrize("n", (1, 300))
def test_all_dead_does_nothing(n):
    from gs_fused import MCMCConfig, mcmc_relocate

    p, mom = make_model(n, seed=2, logits=np.full(n, -8.0))
    gp, gm = to_gpu(p, mom)
    out_p, out_m, info = mcmc_relocate(gp, gm, MCMCConfig(min_opacity=MIN_OPACITY), 700, seed=3)
    assert all(np.array_equal(npy(gp[k]), p[k]) for k in p)
    assert all(np.array_equal(npy(gm[k][i]), mom[k][i]) for k in p for i in (0, 1))
    assert info.counts() == {"dead": n, "relocated": 0, "added": 0}
    assert int(info.plans["relocate"]["totals"][0]) == 0


def test_one_alive_and_a_hundred_dead_clamps_the_ratio():
    from gs_fused import MCMCConfig, mcmc_relocate

    logits = np.full(101, -7.0)
    logits[37] = 1.3862944  # opacity 0.8
    p, mom = make_model(101, seed=4, logits=logits)
    gp, gm = to_gpu(p, mom)
    out_p, out_m, info = mcmc_relocate(gp, gm, MCMCConfig(min_opacity=MIN_OPACITY), 700, seed=3)
    pl = check_phase(p, mom, MR.RELOCATE, 0, 700, 3, gp, gm, out_p, out_m, info.plans["relocate"])
    assert pl["counts"][37] == 100 and set(pl["draw_source"]) == {37}
    o = float(npy(info.plans["relocate"]["opac"])[37])
    o_new, ratio = MR.relocation_values(o, 51)  # min(100 + 1, 51)
    got = npy(out_p["opacities"]).reshape(-1)
    assert neighbour_ok(got, np.full(101, math.log(o_new / (1 - o_new)))).all()
    assert neighbour_ok(npy(out_p["scales"]), p["scales"][37].astype(np.float64)[None] + math.log(ratio)).all()


def test_more_dead_than_alive_without_moments_and_sh_degree_zero():
    from gs_fused import MCMCConfig, mcmc_relocate

    p, mom = make_model(1500, seed=6, dead_fraction=0.8, rest=0, moments=False)
    gp, gm = to_gpu(p, mom)
    out_p, out_m, info = mcmc_relocate(gp, gm, MCMCConfig(min_opacity=MIN_OPACITY), 40, seed=8)
    pl = check_phase(p, mom, MR.RELOCATE, 0, 40, 8, gp, gm, out_p, out_m, info.plans["relocate"])
    assert pl["n_dead"] > 1500 - pl["n_dead"] and out_p["features_rest"].shape == (1500, 0, 3)
    assert max(pl["counts"]) >= 3  # ratios above 2 occur


def test_growth_stops_exactly_at_the_cap_and_refine_composes_the_phases():
    from gs_fused import MCMCConfig, mcmc_add, mcmc_refine, mcmc_relocate

    n = 4099
    cfg = MCMCConfig(min_opacity=MIN_OPACITY, cap_max=n + 7)  # int(1.05 n) - n = 204 > 7
    p, mom = make_model(n, seed=9, rest=0)
    gp, gm = to_gpu(p, mom)
    gp2, gm2 = to_gpu(p, mom)
    out_p, out_m, info = mcmc_refine(gp, gm, cfg, 1200, seed=21)
    assert info["n_out"] == n + 7 == out_p["means"].shape[0] and info["added"] == 7
    assert out_p["features_rest"].shape == (n + 7, 0, 3) and out_m["features_rest"][0].shape == (n + 7, 0, 3)
    a_p, a_m, _ = mcmc_relocate(gp2, gm2, cfg, 1200, seed=21)
    b_p, b_m, _ = mcmc_add(a_p, a_m, cfg, 1200, seed=21)
    for k in MR.PARAM_NAMES:
        assert torch.equal(out_p[k], b_p[k]), k
        assert torch.equal(out_m[k][0], b_m[k][0]) and torch.equal(out_m[k][1], b_m[k][1]), k
    # at the cap: nothing is added, the relocated inputs themselves come back
    again_p, again_m, info2 = mcmc_refine(out_p, out_m, cfg, 1300, seed=21)
    assert all(again_p[k] is out_p[k] for k in out_p) and info2["added"] == 0 and info2["n_out"] == n + 7


def test_same_seed_and_step_give_identical_bytes():
    from gs_fused import MCMCConfig, mcmc_refine

    cfg = MCMCConfig(min_opacity=MIN_OPACITY, cap_max=10_000)
    p, mom = make_model(4099, seed=12)
    runs = []
    for step in (800, 800, 900):
        gp, gm = to_gpu(p, mom)
        out_p, out_m, info = mcmc_refine(gp, gm, cfg, step, seed=77)
        runs.append(({k: npy(v) for k, v in out_p.items()}, {k: (npy(a), npy(b)) for k, (a, b) in out_m.items()},
                     npy(info.plans["relocate"]["draw_source"])[:info["dead"]], npy(info.plans["add"]["draw_source"])))
    for k in MR.PARAM_NAMES:
        assert runs[0][0][k].tobytes() == runs[1][0][k].tobytes(), k
        assert runs[0][1][k][0].tobytes() == runs[1][1][k][0].tobytes(), k
    assert np.array_equal(runs[0][2], runs[1][2]) and np.array_equal(runs[0][3], runs[1][3])
    assert not np.array_equal(runs[0][2], runs[2][2]) and not np.array_equal(runs[0][3], runs[2][3])


# ---- (e) noise ---------------------------------------------------------------------------------------------------------
def noise_inputs(n, seed):
    rng = np.random.default_rng(seed)
    means = (rng.standard_normal((n, 3)) * 2).astype(F32)
    ls = rng.uniform(-5, -1, (n, 3))
    ls[::3, 0] += math.log(1000.0)  # needles: scale ratio 1000
    quats = rng.standard_normal((n, 4)).astype(F32)
    op = np.array([0.001, 0.004, 0.006, 0.5])[np.arange(n) % 4]
    logits = np.log(op / (1 - op)).astype(F32).reshape(n, 1)
    return means, ls.astype(F32), quats, logits, rng.standard_normal((n, 3)).astype(F32)


@pytest.mark.parametrize("n", (1, 257, 4099))
def test_noise_with_explicit_samples_against_float64(n):
    from gs_fused import mcmc_inject_noise_

    means, ls, quats, logits, eps = noise_inputs(n, n)
    scaler = 1.6e-4 * 5e5
    g = cu(means)
    out = mcmc_inject_noise_(g, cu(ls), cu(quats), cu(logits), scaler, seed=1, step=2, noise=cu(eps))
    assert out is g
    got = npy(g).astype(np.float64) - means.astype(np.float64)
    ref, cov_norm, v_norm = MR.noise_delta(ls, quats, logits, eps, scaler)
    # ulp(mean): of the larger of the mean before and after -- the one rounding of `mean += delta` happens at the sum
    bound = np.maximum(ulp32(means), ulp32(npy(g))) + 1e-4 * (cov_norm * v_norm)[:, None]
    assert (np.abs(got - ref) <= bound).all(), float((np.abs(got - ref) / bound).max())
    gate = MR.noise_gate(logits)
    assert (gate[np.arange(n) % 4 <= 1] > 0.5).all() and (gate[np.arange(n) % 4 == 3] < 1e-20).all()
    if n > 4:
        moved = np.abs(got).max(-1)
        assert moved[np.arange(n) % 4 == 0].max() > 0 and moved[np.arange(n) % 4 == 3].max() == 0


def test_noise_from_the_counter_based_generator_and_zero_scaler():
    from gs_fused import mcmc_inject_noise_

    n = 5000
    means = np.zeros((n, 3), F32)
    ls = np.zeros((n, 3), F32)  # Sigma = I
    quats = np.tile(np.array([1, 0, 0, 0], F32), (n, 1))
    logits = np.full((n, 1), -30.0, F32)  # opacity 0: gate = 1 / (1 + exp(-0.5))
    g = cu(means)
    mcmc_inject_noise_(g, cu(ls), cu(quats), cu(logits), 1.0, seed=0x1234567890, step=41)
    gate = MR.noise_gate(logits)[:, None]
    z = MR.noise_normals(0x1234567890, n, 41)
    # the in-kernel normals go through logf / sqrtf / cosf / sinf: the comparison tests/test_refine.py uses
    np.testing.assert_allclose(npy(g) / gate, z, rtol=1e-5, atol=2e-5)
    other = cu(means)
    mcmc_inject_noise_(other, cu(ls), cu(quats), cu(logits), 1.0, seed=0x1234567890, step=42)
    assert not torch.equal(other, g)
    m2, ls2, q2, lg2, eps = noise_inputs(257, 3)
    still = cu(m2)
    mcmc_inject_noise_(still, cu(ls2), cu(q2), cu(lg2), 0.0, seed=1, step=2, noise=cu(eps))
    assert npy(still).tobytes() == m2.tobytes()


# ---- (f) regularisers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 257, 70001))
def test_regulariser_forward_backward_and_central_differences(n):
    from gs_fused import mcmc_regularizer

    rng = np.random.default_rng(n)
    logits = rng.uniform(-6, 6, (n, 1)).astype(F32)
    ls = rng.uniform(-6, 0.5, (n, 3)).astype(F32)
    a, b = 0.01, 0.02
    L_ref, g_lo, g_ls = MR.regulariser(logits, ls, a, b)
    x, s = cu(logits).requires_grad_(True), cu(ls).requires_grad_(True)
    L = mcmc_regularizer(x, s, a, b)
    assert L.dtype == torch.float64 and L.dim() == 0
    assert abs(float(L.detach()) - L_ref) <= 1e-10 * abs(L_ref)
    (3.0 * L).backward()
    assert (np.abs(npy(x.grad).reshape(-1) - 3 * g_lo) <= 2 * ulp32(3 * g_lo)).all()
    assert (np.abs(npy(s.grad) - 3 * g_ls) <= 2 * ulp32(3 * g_ls)).all()
    assert float(mcmc_regularizer(x, s, a, b).detach()) == float(L.detach())  # a fixed summation order
    # central differences on up to 64 elements, h = 1e-2, to 1e-3 of the gradient
    flat = np.concatenate([logits.reshape(-1), ls.reshape(-1)])
    grads = np.concatenate([npy(x.grad).reshape(-1), npy(s.grad).reshape(-1)]).astype(np.float64) / 3
    for e in rng.choice(len(flat), min(64, len(flat)), replace=False):
        vals = []
        for sign in (+1, -1):
            f = flat.copy()
            f[e] = F32(flat[e] + sign * 1e-2)
            vals.append((float(mcmc_regularizer(cu(f[:n].reshape(n, 1)), cu(f[n:].reshape(n, 3)), a, b)), float(f[e])))
        fd = (vals[0][0] - vals[1][0]) / (vals[0][1] - vals[1][1])
        assert abs(fd - grads[e]) <= 1e-3 * abs(grads[e]), (e, fd, grads[e])


# ---- the trainer ---------------------------------------------------------------------------------------------------
def _train(route, tmp_path, name, monkeypatch):
    import harness.train as T
    from gs_fused import MCMCConfig
    from rasterizer import rasterize as R

    def no_default_refinement(*a, **k):
        raise AssertionError("refine_gaussians called under strategy='mcmc'")

    monkeypatch.setattr(T, "_refine", no_default_refinement)
    ply = str(tmp_path / f"{name}.ply")
    cfg = T.TrainConfig(num_gaussians=6000, init_gaussians=2000, width=160, height=90, num_views=4, iters=300,
                        sh_degree=3, sh_degree_interval=60, strategy="mcmc", export_ply=ply,
                        mcmc=MCMCConfig(cap_max=3000, refine_start_iter=20, refine_every=20),
                        fused_render=route != "separate", use_graph=route == "graph")
    R.set_deterministic(True)
    try:
        res = T.train(cfg, torch.device("cuda", 0))
    finally:
        R.set_deterministic(False)
    return res, open(ply, "rb").read()


@pytest.mark.parametrize("route", ("separate", "fused", "graph"))
def test_training_with_the_mcmc_strategy(route, tmp_path, monkeypatch):
    res, ply = _train(route, tmp_path, "a", monkeypatch)
    assert res["render"] == {"separate": "separate ops", "fused": "one fused op", "graph": "hip graph per view"}[route]
    assert res["strategy"] == "mcmc" and res["num_gaussians_start"] == 2000
    sizes = [2000] + [n for _, n in res["refinements"]]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and max(sizes) <= 3000
    assert res["num_gaussians_end"] == 3000 and len(res["refinements"]) == 9  # 5 % per refinement: nine to the cap
    assert np.isfinite(res["param_checksum"])
    assert res["psnr_end"] > res["psnr_start"], res
    if route == "separate":  # two runs in the deterministic mode: identical parameter bytes
        res2, ply2 = _train(route, tmp_path, "b", monkeypatch)
        assert ply == ply2 and res2["param_checksum"] == res["param_checksum"]
