"""CPU: the float64 restatement of the depth-distortion walk (tests/distortion_reference.py) against what it restates --
the double sum, central differences, the median rule on hand-built rays -- and the stability cap of every case the GPU
test runs (tests/test_gpu_distortion.py): the seeds are chosen so that the reference alone meets it."""
import numpy as np
import pytest
import torch

import distortion_reference as D


def ray(opac, z, sx=1e3):
    """A 1 x 1 image whose single pixel sees Gaussians centred 0.3 px beside it, so wide (sx) that alpha_i is opac_i
    up to 1e-7, in list order -> (ids, bins, scene arrays)."""
    n = len(opac)
    conic = 1.0 / (sx * sx)
    return (np.arange(n, dtype=np.int32), np.array([[0, n]], np.int32),
            dict(xys=np.tile(np.array([[0.3, 0.0]], np.float32), (n, 1)),
                 conics=np.tile(np.array([[conic, 0.0, conic]], np.float32), (n, 1)),
                 opacities=np.asarray(opac, np.float32), values=np.asarray(z, np.float32)))


def walk_ray(opac, z, v=None):
    ids, bins, sc = ray(opac, z)
    return D.distortion_reference(1, 1, ids, bins, sc["xys"], sc["conics"], sc["opacities"], sc["values"],
                                  v_distortion=None if v is None else np.array([[v]], np.float32))


def test_linear_form_equals_the_double_sum_on_sorted_values():
    rng = np.random.default_rng(0)
    for n in (1, 2, 7, 40):
        opac = rng.uniform(0.02, 0.3, n)
        z = np.sort(rng.uniform(0.5, 4.0, n))
        ref = walk_ray(opac, z)
        # the weights of the same ray, independently: alpha_i prod_{j<i} (1 - alpha_j) with the float32 inputs
        ids, bins, sc = ray(opac, z)
        a = sc["opacities"].astype(np.float64) * np.exp(-0.5 * sc["conics"][:, 0].astype(np.float64) * np.float64(np.float32(0.3)) ** 2)
        w = a * np.concatenate([[1.0], np.cumprod(1.0 - a)[:-1]])
        want = D.double_sum(w, sc["values"].astype(np.float64))
        got = float(ref["distortion"][0, 0])
        print(f"n = {n}: O(n) form {got:.15e}, double sum {want:.15e}")
        assert abs(got - want) <= 1e-12 * max(abs(want), 1e-30)
        assert abs(float(ref["vsum"][0, 0]) - float((w * sc["values"]).sum())) <= 1e-13
        assert abs(float(ref["final_T"][0, 0]) - float(np.prod(1.0 - a))) <= 1e-14


def test_autograd_gradients_agree_with_central_differences():
    sc = D.build_case("partial")
    ids, bins = D.oracle_lists(sc)
    H, W = sc["H"], sc["W"]
    ref = D.distortion_reference(H, W, ids, bins, sc["xys"], sc["conics"], sc["opacities"], sc["values"],
                                 sc["v_distortion"])
    keep = ~ref["unstable"]
    vD = torch.from_numpy(sc["v_distortion"]).double() * keep  # (a flipped decision is no derivative)
    ref = D.distortion_reference(H, W, ids, bins, sc["xys"], sc["conics"], sc["opacities"], sc["values"], vD.numpy())

    def loss(**over):  # float64 inputs, the decisions of the unperturbed walk
        arrs = {k: torch.from_numpy(np.asarray(sc[k], np.float64)).clone() for k in ("xys", "conics", "opacities", "values")}
        arrs["opacities"] = arrs["opacities"].reshape(-1)
        for k, (i, h) in over.items():
            arrs[k].reshape(-1)[i] += h
        total = 0.0
        tiles_x = (W + 15) // 16
        for tile, dec in ref["decisions"].items():
            ty, tx = divmod(tile, tiles_x)
            rows, cols = torch.arange(ty * 16, min(ty * 16 + 16, H)), torch.arange(tx * 16, min(tx * 16 + 16, W))
            py, px = (m.reshape(-1) for m in torch.meshgrid(rows, cols, indexing="ij"))
            g = torch.from_numpy(np.asarray(ids).astype(np.int64))[int(bins[tile, 0]):int(bins[tile, 1])]
            wk = D._walk(px.double(), py.double(), g, [arrs["xys"], arrs["conics"], arrs["opacities"], arrs["values"]],
                         torch.float64, decisions=dec)
            total += float((wk["D"] * vD[py, px]).sum())
        return total

    rng = np.random.default_rng(1)
    worst = 0.0
    for name, key, h in (("v_xy", "xys", 1e-6), ("v_conic", "conics", 1e-7), ("v_opacity", "opacities", 1e-7),
                         ("v_values", "values", 1e-6)):
        flat = ref[name].reshape(-1)
        scale = float(flat.abs().max())
        assert scale > 0
        for i in rng.choice(flat.numel(), 6, replace=False):
            fd = (loss(**{key: (int(i), h)}) - loss(**{key: (int(i), -h)})) / (2 * h)
            err = abs(fd - float(flat[i])) / scale
            worst = max(worst, err)
            print(f"{name}[{i}]: autograd {float(flat[i]):+.9e}, central difference {fd:+.9e}")
            assert err <= 1e-6, (name, i)
    print(f"worst |autograd - central difference| / max|gradient| = {worst:.2e}")


def test_median_rule_on_hand_built_rays():
    # crossing at the first entry: T_1 = 1 > 0.5, T_2 = 0.4: the first entry, whatever follows
    r = walk_ray([0.6, 0.3, 0.3], [1.0, 2.0, 3.0])
    assert float(r["median"][0, 0]) == 1.0 and int(r["final_idx"][0, 0]) == 2
    # never crossing: final T = 0.9^3 > 0.5: the last contributing entry
    r = walk_ray([0.1, 0.1, 0.1], [1.0, 2.0, 3.0])
    assert float(r["final_T"][0, 0]) > 0.5 and float(r["median"][0, 0]) == 3.0
    # crossing in the middle: T = 1, 0.7, 0.49: the second entry
    r = walk_ray([0.3, 0.3, 0.3], [1.0, 2.0, 3.0])
    assert float(r["median"][0, 0]) == 2.0
    # crossing exactly at the stop entry.  The stop entry itself never counts, and with alpha <= 0.999 it cannot be the
    # one with T_i > 0.5 (T_i 0.001 <= 1e-4 needs T_i <= 0.1).  What can happen: the crossing entry is the last
    # contributing one and the very next entry stops the walk -- T = 1, 0.08, then 0.08 * 0.001 <= 1e-4
    r = walk_ray([0.92, 0.9995, 0.5], [1.0, 2.0, 3.0])
    assert int(r["final_idx"][0, 0]) == 0 and float(r["median"][0, 0]) == 1.0
    assert abs(float(r["final_T"][0, 0]) - 0.08) < 1e-6 and not bool(r["decisions"][0][0, 1:].any())
    # ... and a stop entry right behind entries that never crossed: impossible for the same reason (T > 0.5 there)
    r = walk_ray([0.4, 0.9995, 0.5], [1.0, 2.0, 3.0])
    assert int(r["final_idx"][0, 0]) == 2 and float(r["median"][0, 0]) == 2.0  # (0.6 * 0.001 > 1e-4: it counts)
    # a skipped entry (alpha < 1/255) between two contributing ones is not the median
    r = walk_ray([0.3, 0.001, 0.3], [1.0, 2.0, 3.0])
    assert float(r["median"][0, 0]) == 3.0 and bool(r["decisions"][0][0, 1]) is False
    # nothing contributes
    r = walk_ray([0.001], [1.0])
    assert float(r["median"][0, 0]) == 0.0 and int(r["final_idx"][0, 0]) == -1 and float(r["distortion"][0, 0]) == 0.0


def test_the_clamp_passes_no_gradient_to_alpha():
    sc = D.build_case("clamp")
    ids, bins = D.oracle_lists(sc)
    v = np.zeros((16, 16), np.float32)
    v[8, 8] = 1.0  # the one pixel at which Gaussian 0 is clamped
    ref = D.distortion_reference(16, 16, ids, bins, sc["xys"], sc["conics"], sc["opacities"], sc["values"], v)
    assert not bool(ref["unstable"][8, 8])
    assert float(ref["v_opacity"][0]) == 0.0 and float(ref["v_xy"][0].abs().max()) == 0.0
    assert float(ref["v_values"][0]) != 0.0 and float(ref["v_opacity"][1:].abs().max()) > 0.0


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_every_gpu_case_meets_the_stability_cap(name):
    """At most 1 % of the pixels unstable and at most 1 % of the Gaussians with slack, on the reference alone."""
    sc = D.build_case(name)
    ids, bins = D.oracle_lists(sc)
    ref = D.distortion_reference(sc["H"], sc["W"], ids, bins, sc["xys"], sc["conics"], sc["opacities"], sc["values"],
                                 sc["v_distortion"])
    pixels, gaussians = D.stability(ref)
    lengths = (np.asarray(bins)[:, 1] - np.asarray(bins)[:, 0]).tolist()
    print(f"{name}: seed {D.CASES[name][1]}, lists {lengths}, unstable pixels {pixels:.4f}, Gaussians with slack "
          f"{gaussians:.4f}")
    assert pixels <= 0.01 and gaussians <= 0.01
    if name == "deep":
        assert lengths == [600]
    if name == "opaque":
        assert int(ref["final_idx"].max()) < 40 - 1 and float(ref["final_T"].max()) < 1e-2
    if name == "empty_tile":
        assert lengths[-1] == 0 and min(lengths[:-1]) > 0
    if name == "clamp":
        raw = float(sc["opacities"][0, 0]) * np.exp(-0.5 * float(sc["conics"][0, 0]) * 0.05 ** 2)
        assert raw > D.ALPHA_MAX * (1 + 1e-5)
