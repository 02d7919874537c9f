"""GPU: the contribution walk (csrc/contribution.hip) on lists built by the existing binning entries, against the float64
restatement of tests/contribution_reference.py fed the same lists; against the existing forward's alpha image; and the
op, its accumulation, its reproducibility and the pruning it is for.

Bounds.  With e32 the largest float32 error of a weight (the restatement run in float32 on the float64 run's
decisions): `hits` exact on Gaussians with no near pair, `dominant` exact on those that in addition hold neither of the
two largest weights of a near-tie pixel, |max_w - ref| <= 4 e32, |sum_q - ref 2^24| <= hits (1 + 4 e32 2^24) -- the floor
loses under one unit per pair.  At most 2 % of the Gaussians with hits may be left out as near; that cap is asserted on
the CPU as well (tests/test_contribution_host.py).  Against the forward: sum_g sum_q / 2^24 equals the sum of the alpha
image within 4 * 2^-24 * sum_g hits (per pair: the floor, the product alpha T, the forward's running T, and one of
margin)."""
import numpy as np
import pytest
import torch

import contribution_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q_ONE = float(1 << 24)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_lists(sc):
    """ids, bins of a scene from the package's binning entries (the bounding-box pipeline of rasterizer.utils)."""
    from rasterizer.utils import bin_and_sort_gaussians, compute_cumulative_intersects

    H, W = sc["H"], sc["W"]
    tb = ((W + 15) // 16, (H + 15) // 16, 1)
    I, cum = compute_cumulative_intersects(cu(sc["num_tiles_hit"]))
    _, _, _, ids, bins = bin_and_sort_gaussians(sc["xys"].shape[0], I, cu(sc["xys"]), cu(sc["depths"]), cu(sc["radii"]),
                                                cum, tb, 16)
    return ids, bins, tb


def zeros(n):
    return (torch.zeros(n, dtype=torch.float32, device=DEV),) + tuple(
        torch.zeros(n, dtype=torch.int64, device=DEV) for _ in range(3))


def view_args(sc):
    return (cu(sc["xys"]), cu(sc["depths"]), cu(sc["radii"]), cu(sc["conics"]), cu(sc["num_tiles_hit"]),
            cu(sc["opacities"]), sc["H"], sc["W"])


def as_tuple(st):
    return st.max_weight, st.sum_q, st.hits, st.dominant


_cache = {}


def case(name):
    """Scene, lists, the kernel's four arrays and the float64 / float32 references: computed once per case."""
    if name in _cache:
        return _cache[name]
    import rasterizer.cuda as C

    sc = R.build_case(name)
    H, W, n = sc["H"], sc["W"], sc["xys"].shape[0]
    ids, bins, tb = gpu_lists(sc)
    got = zeros(n)
    C.contribution_accumulate(tb, (W, H, 1), ids, bins, cu(sc["xys"]), cu(sc["conics"]), cu(sc["opacities"]), *got)
    torch.cuda.synchronize()
    ids_h, bins_h = ids.cpu().numpy(), bins.cpu().numpy().reshape(-1, 2)[:tb[0] * tb[1]]
    args = (H, W, ids_h, bins_h, sc["xys"], sc["conics"], sc["opacities"])
    ref = R.contribution_reference(*args)
    ref32 = R.contribution_reference(*args, dtype=torch.float32, decisions=ref["decisions"])
    _cache[name] = dict(sc=sc, ids=ids, bins=bins, tb=tb, got=[t.cpu() for t in got], ref=ref, e32=R.e32_of(ref, ref32))
    return _cache[name]


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_statistics_against_float64(name):
    c = case(name)
    ref, e32 = c["ref"], c["e32"]
    max_w, sum_q, hits, dominant = c["got"]
    seen = ref["hits"] > 0
    share = R.near_share(ref)
    print(f"{name}: {int(seen.sum())} Gaussians with hits, near share {share:.4f}, e32 = {e32:.3e}")
    assert share <= 0.02
    calm = ~ref["near"]
    assert torch.equal(hits[calm], ref["hits"][calm])
    calm_dom = calm & ~ref["near_tie"]
    assert torch.equal(dominant[calm_dom], ref["dominant"][calm_dom])
    err_max = (max_w.double() - ref["max_w"]).abs()[calm]
    err_sum = (sum_q.double() - ref["sum_w"] * Q_ONE).abs()[calm]
    bound_sum = ref["hits"][calm].double() * (1.0 + 4.0 * e32 * Q_ONE)
    print(f"{name}: max |max_w - ref| = {float(err_max.max()):.3e} (bound {4 * e32:.3e}); worst |sum_q - ref 2^24| / "
          f"bound = {float((err_sum / bound_sum.clamp(min=1.0)).max()):.3e}, in units per pair "
          f"{float((err_sum / ref['hits'][calm].double().clamp(min=1.0)).max()):.3f}")
    assert bool((err_max <= 4.0 * e32).all())
    assert bool((err_sum <= bound_sum).all())
    # whoever the reference never counts has exact zeros in all four
    never = ~seen & calm
    for t in c["got"]:
        assert bool((t[never] == 0).all())
    assert int(dominant.sum()) <= c["sc"]["H"] * c["sc"]["W"] and bool((hits >= dominant).all())
    assert bool(((hits > 0) == (max_w > 0)).all())
    if name == "hidden":
        rows = R.hidden_rows()
        for k in ("stopper", "hidden", "faint"):
            for t in c["got"]:
                assert bool((t[rows[k]] == 0).all()), k
    if name == "edges":  # lanes outside the image count nothing: every pixel of the image has at most one dominant
        assert int(dominant.sum()) == int((ref["best"] >= 0).sum())


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_weight_sums_against_the_forwards_alpha_image(name):
    from gs_fused import view_contributions
    from rasterizer import rasterize_gaussians

    sc = R.build_case(name)
    args = view_args(sc)
    n = sc["xys"].shape[0]
    _, alpha = rasterize_gaussians(*args[:5], torch.full((n, 3), 0.5, device=DEV), args[5], sc["H"], sc["W"], 16,
                                   background=torch.zeros(3, device=DEV), return_alpha=True)
    st = view_contributions(*args)
    total, want = float(st.weight_sum.sum()), float(alpha.double().sum())
    pairs = int(st.hits.sum())
    bound = 4.0 * 2.0 ** -24 * pairs
    print(f"{name}: sum of weights {total:.9f}, sum of the alpha image {want:.9f}, difference {abs(total - want):.3e}, "
          f"bound {bound:.3e} ({pairs} pairs)")
    assert pairs > 0 and abs(total - want) <= bound
    # the op on the cached lists (which leave out pairs that cannot reach 1/255) = the low-level call on the
    # bounding-box lists, to the bit: integer sums and a max know no order
    c = case(name)
    for a, b in zip(as_tuple(st), c["got"]):
        assert torch.equal(a.cpu(), b)
    assert st.views == 1


def test_two_views_accumulate_to_the_max_and_the_sums():
    from gs_fused import ContributionStats, view_contributions

    sc1, sc2 = R.scene_edges(0), R.scene_edges(0, shift=(2.7, -1.9))
    assert not np.array_equal(sc1["xys"], sc2["xys"]) and np.array_equal(sc1["conics"], sc2["conics"])
    a, b = view_contributions(*view_args(sc1)), view_contributions(*view_args(sc2))
    both = ContributionStats(sc1["xys"].shape[0], DEV)
    both.accumulate(*view_args(sc1)).accumulate(*view_args(sc2))
    assert both.views == 2
    assert torch.equal(both.max_weight, torch.maximum(a.max_weight, b.max_weight))
    assert torch.equal(both.sum_q, a.sum_q + b.sum_q) and torch.equal(both.weight_sum, a.weight_sum + b.weight_sum)
    assert torch.equal(both.hits, a.hits + b.hits) and torch.equal(both.dominant, a.dominant + b.dominant)
    assert not torch.equal(a.hits, b.hits)  # (two different views)
    # the native entry adds in place: a second call on the same lists doubles the sums and keeps the max
    import rasterizer.cuda as C

    c = case("edges")
    sc = c["sc"]
    got = zeros(sc["xys"].shape[0])
    for _ in range(2):
        C.contribution_accumulate(c["tb"], (sc["W"], sc["H"], 1), c["ids"], c["bins"], cu(sc["xys"]), cu(sc["conics"]),
                                  cu(sc["opacities"]), *got)
    assert torch.equal(got[0].cpu(), c["got"][0])
    for t, once in zip(got[1:], c["got"][1:]):
        assert torch.equal(t.cpu(), 2 * once)


def test_three_runs_are_identical_also_in_deterministic_mode():
    from gs_fused import view_contributions
    from rasterizer import rasterize as RR

    sc = R.build_case("deep")
    runs = [as_tuple(view_contributions(*view_args(sc))) for _ in range(3)]
    was = RR.is_deterministic()
    RR.set_deterministic(True)
    try:
        runs += [as_tuple(view_contributions(*view_args(sc))) for _ in range(3)]
    finally:
        RR.set_deterministic(was)
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b)
    assert int(runs[0][2].sum()) > 0


def test_nothing_on_screen_launches_nothing():
    from gs_fused import ContributionStats

    n, H, W = 5, 17, 33
    st = ContributionStats(n, DEV)
    st.max_w.fill_(0.25)
    st.sum_q.fill_(7)
    st.hit_count.fill_(3)
    st.dominant_count.fill_(1)
    none = torch.zeros((n,), dtype=torch.int32, device=DEV)
    st.accumulate(torch.zeros((n, 2), device=DEV), torch.ones((n,), device=DEV), none, torch.ones((n, 3), device=DEV),
                  none, torch.full((n, 1), 0.5, device=DEV), H, W)
    assert st.views == 1
    assert bool((st.max_weight == 0.25).all()) and bool((st.sum_q == 7).all())
    assert bool((st.hits == 3).all()) and bool((st.dominant == 1).all())
    # ... and the native entry's wrapper with empty lists
    import rasterizer.cuda as C

    got = zeros(n)
    C.contribution_accumulate((3, 2, 1), (W, H, 1), torch.zeros((0,), dtype=torch.int32, device=DEV),
                              torch.zeros((6, 2), dtype=torch.int32, device=DEV), torch.zeros((n, 2), device=DEV),
                              torch.ones((n, 3), device=DEV), torch.full((n, 1), 0.5, device=DEV), *got)
    assert all(not bool(t.any()) for t in got)
    with pytest.raises(ValueError, match="ContributionStats.accumulate.*n = 5"):
        st.accumulate(torch.zeros((n + 1, 2), device=DEV), torch.ones((n + 1,), device=DEV),
                      torch.zeros((n + 1,), dtype=torch.int32, device=DEV), torch.ones((n + 1, 3), device=DEV),
                      torch.zeros((n + 1,), dtype=torch.int32, device=DEV), torch.full((n + 1, 1), 0.5, device=DEV), H, W)


def test_pruning_the_hidden_scene_leaves_the_image_alone():
    from gs_fused import prune_mask, view_contributions
    from rasterizer import rasterize as RR
    from rasterizer import rasterize_gaussians

    sc = R.build_case("hidden")
    H, W, n = sc["H"], sc["W"], sc["xys"].shape[0]
    rng = np.random.default_rng(5)
    colors, bg = cu(rng.uniform(0.05, 1.0, (n, 3)).astype(np.float32)), cu(np.array([0.2, 0.5, 0.3], np.float32))
    args = view_args(sc)
    full = rasterize_gaussians(*args[:5], colors, args[5], H, W, 16, background=bg)
    builds = dict(RR.counters)
    st = view_contributions(*args)
    assert dict(RR.counters) == builds  # behind the RGB pass: a cache hit, no list was built
    keep = prune_mask(st, rule="max_weight")
    rows = R.hidden_rows()
    want = torch.zeros(n, dtype=torch.bool)
    for k in ("front", "wall"):
        want[rows[k]] = True
    assert torch.equal(keep.cpu(), want)
    assert int((st.hits == 0).sum()) == n - int(want.sum())
    kept = [t[keep] for t in args[:5]] + [colors[keep], args[5][keep]]
    pruned = rasterize_gaussians(*kept, H, W, 16, background=bg)
    err = float((pruned - full).abs().max())
    print(f"hidden: {n} -> {int(keep.sum())} Gaussians, max |image difference| = {err:.3e}")
    assert err <= 1e-4
