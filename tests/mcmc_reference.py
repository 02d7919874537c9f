"""NumPy float64 / Python-integer restatement of the MCMC densification kernels (include/gsraster.h "MCMC
densification", csrc/mcmc.hip): the oracle of tests/test_mcmc_host.py and tests/test_gpu_mcmc.py.

  relocation_values   o' = 1 - (1 - o)^(1/n), D = sum_i sum_k C(i-1,k) (-1)^k o'^(k+1) / sqrt(k+1), o / D -- float64
  weights / plan      integer weights floor(opac * 2^24), Python-integer prefix sums, dead rows in ascending order
  draw_targets        Philox4x32-10 (oracle.refine.philox4x32_10), r = c0 * 2^32 + c1, target = (r * total) >> 64
  sample              source = first index whose inclusive prefix is > target (bisect_right)
  phase               one relocate / add phase on the six tensors (and moments), fed the kernel's own `opac`
  noise_delta         Sigma (eps * gate * scaler) in float64
  regulariser         the loss and its closed-form gradients in float64
"""
import bisect
import math
from typing import Dict, Optional

import numpy as np

from oracle.refine import philox4x32_10, split_normals

PARAM_NAMES = ("means", "scales", "quats", "features_dc", "features_rest", "opacities")
MAX_RATIO = 51
RELOCATE, ADD = 0, 1
OPACITY_MAX = 1.0 - 2.0 ** -23


def relocation_values(o: float, n: int):
    """-> (o', o / D) in float64, the sum in the order it is written (i outer, k inner)."""
    n = min(max(int(n), 1), MAX_RATIO)
    o = float(o)
    o_new = 1.0 - (1.0 - o) ** (1.0 / n)
    D = 0.0
    for i in range(1, n + 1):
        p, sign = o_new, 1.0
        for k in range(i):
            D += math.comb(i - 1, k) * sign * p / math.sqrt(k + 1)
            p *= o_new
            sign = -sign
    return o_new, o / D


def relocation(opacities, scales, ratios, min_opacity: float = 0.0, raw: bool = False):
    """gs_fused.relocation in float64 (not yet rounded to float32)."""
    opacities, scales = np.asarray(opacities, np.float64), np.asarray(scales, np.float64)
    out_o, out_s = np.empty_like(opacities), np.empty_like(scales)
    for i, (o, n) in enumerate(zip(opacities, ratios)):
        o_new, ratio = relocation_values(o, n) if min(max(int(n), 1), MAX_RATIO) > 1 else (o, 1.0)
        oc = min(max(o_new, float(np.float32(min_opacity))), OPACITY_MAX)
        if raw:
            out_o[i] = math.log(oc / (1.0 - oc))
            out_s[i] = np.log(scales[i]) + math.log(ratio)
        else:
            out_o[i] = oc if int(n) > 1 else o
            out_s[i] = ratio * scales[i]
    return out_o, out_s


def new_raw_values(opac: float, log_scales, count: int, min_opacity: float):
    """What a source drawn `count` times becomes: (logit, log-scales) in float64."""
    o_new, ratio = relocation_values(float(opac), min(count + 1, MAX_RATIO))
    oc = min(max(o_new, float(np.float32(min_opacity))), OPACITY_MAX)
    return math.log(oc / (1.0 - oc)), np.asarray(log_scales, np.float64) + math.log(ratio)


def weights(opac: np.ndarray, min_opacity: float, phase: int):
    """-> (list of Python-integer weights, dead flags) from float32 opacities."""
    opac = np.asarray(opac, np.float32)
    dead = opac <= np.float32(min_opacity)
    w = [int(math.floor(float(o) * 16777216.0)) if o == o else 0 for o in opac]  # exact: a power of two
    if phase == RELOCATE:
        w = [0 if d else x for x, d in zip(w, dead)]
    return w, dead


def draw_targets(num: int, phase: int, step: int, seed: int, total: int):
    j = np.arange(num, dtype=np.uint32)
    ctr = np.stack([j, np.full_like(j, phase), np.full_like(j, step & 0xFFFFFFFF), np.zeros_like(j)], axis=-1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32), (num, 2))
    x = philox4x32_10(ctr, key) if num else np.zeros((0, 4), np.uint32)
    return [((int(a) << 32 | int(b)) * total) >> 64 for a, b in zip(x[:, 0], x[:, 1])]


def sample(prefix, targets):
    """The first index whose inclusive prefix is > target."""
    return [bisect.bisect_right(prefix, t) for t in targets]


def plan(opac: np.ndarray, min_opacity: float, phase: int, num_draws: int, step: int, seed: int) -> Dict:
    n = len(opac)
    w, dead = weights(opac, min_opacity, phase)
    prefix, acc = [], 0
    for x in w:
        acc += x
        prefix.append(acc)
    dead_index = [i for i in range(n) if dead[i]]
    total = acc
    nd = len(dead_index) if phase == RELOCATE else num_draws
    counts = [0] * n
    row_source = [-1] * n
    if total == 0:
        sources = [-1] * nd if phase == RELOCATE else [j % n for j in range(nd)]
    else:
        sources = sample(prefix, draw_targets(nd, phase, step, seed, total))
        for j, s in enumerate(sources):
            counts[s] += 1
            if phase == RELOCATE:
                row_source[dead_index[j]] = s
    return {"prefix": prefix, "dead_index": dead_index, "total": total, "n_dead": len(dead_index),
            "draw_source": sources, "row_source": row_source, "counts": counts}


def phase(params: Dict[str, np.ndarray], moments: Optional[Dict], opac: np.ndarray, min_opacity: float, ph: int,
          num_draws: int, step: int, seed: int):
    """One phase on float32 arrays -> (params, moments, plan, updated): sources take their new values (float64,
    rounded once), destinations copy their source afterwards, moments of both are zero.  `updated`: the float64 new
    (logit, log-scales) per source, for the neighbour comparison."""
    n = len(opac)
    pl = plan(opac, min_opacity, ph, num_draws, step, seed)
    n_out = n + (num_draws if ph == ADD else 0)
    p = {k: np.concatenate([v, np.zeros((n_out - n,) + v.shape[1:], v.dtype)]) for k, v in params.items()}
    mom = None if moments is None else {k: tuple(np.concatenate([m, np.zeros((n_out - n,) + m.shape[1:], m.dtype)])
                                                  for m in pair) for k, pair in moments.items()}
    updated = {}
    for i, c in enumerate(pl["counts"]):
        if c > 0:
            lg, ls = new_raw_values(opac[i], params["scales"][i], c, min_opacity)
            updated[i] = (lg, ls)
            p["opacities"][i] = np.float32(lg)
            p["scales"][i] = ls.astype(np.float32)
            if mom is not None:
                for pair in mom.values():
                    for m in pair:
                        m[i] = 0
    dest = [(r, s) for r, s in enumerate(pl["row_source"]) if s >= 0] if ph == RELOCATE else \
        [(n + j, s) for j, s in enumerate(pl["draw_source"])]
    for r, s in dest:
        for k in p:
            p[k][r] = p[k][s]
        if mom is not None:
            for pair in mom.values():
                for m in pair:
                    m[r] = 0
    pl["dest"] = dest
    return p, mom, pl, updated


def num_new(cap_max: int, grow_factor: float, n: int) -> int:
    return max(0, min(int(cap_max), int(grow_factor * n)) - n)


# ---- noise ---------------------------------------------------------------------------------------------------------
def rotation(q: np.ndarray) -> np.ndarray:
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=-1)
    return R.reshape(q.shape[:-1] + (3, 3))


def noise_gate(logits) -> np.ndarray:
    o = 1.0 / (1.0 + np.exp(-np.asarray(logits, np.float64).reshape(-1)))
    return 1.0 / (1.0 + np.exp(-100.0 * ((1.0 - o) - 0.995)))


def noise_delta(log_scales, raw_quats, logits, eps, scaler: float):
    """-> (delta [N,3], |Sigma| [N] (largest eigenvalue), |eps * gate * scaler| [N]) in float64."""
    R = rotation(raw_quats)
    s2 = np.exp(np.asarray(log_scales, np.float64)) ** 2
    v = np.asarray(eps, np.float64) * (noise_gate(logits) * float(np.float32(scaler)))[:, None]
    cov = np.einsum("nij,nj,nkj->nik", R, s2, R)
    return np.einsum("nij,nj->ni", cov, v), s2.max(-1), np.linalg.norm(v, axis=-1)


def noise_normals(seed: int, n: int, step: int) -> np.ndarray:
    """The kernel's eps without `noise=`: the three normals of the Philox block of counter (i, step, 0, 0)."""
    return split_normals(seed, np.arange(n), step)


# ---- regularisers --------------------------------------------------------------------------------------------------
def regulariser(logits, log_scales, opacity_reg: float, scale_reg: float):
    """-> (L, dL/dlogits [N], dL/dlog_scales [N,3]) in float64 (math.fsum for the means)."""
    x = np.asarray(logits, np.float64).reshape(-1)
    s = np.asarray(log_scales, np.float64)
    n = len(x)
    sg, e = 1.0 / (1.0 + np.exp(-x)), np.exp(s)
    L = opacity_reg * math.fsum(sg) / n + scale_reg * math.fsum(e.reshape(-1)) / (3 * n)
    return L, opacity_reg / n * sg * (1 - sg), scale_reg / (3 * n) * e
