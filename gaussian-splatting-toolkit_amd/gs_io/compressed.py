"""A compressed container for a trained model: the spherical-harmonics rows behind a k-means
codebook (gs_fused.kmeans, csrc/kmeans.hip), every other attribute as 8- or 16-bit codes on its own range.  The second
half of the LightGaussian / Compact3D recipe, the first being contribution pruning (section 4.21).

    compress_gaussians(params, sh_clusters=16384, iters=10, seed=0, weights=None) -> blob
    decompress_gaussians(blob)                                                   -> params (float32, the PLY's layout)
    write_compressed(path, blob) / read_compressed(path)                         -> one .npz

`params` are the six raw tensors `gs_io.write_gaussian_ply` takes: means [N,3], features_dc [N,3], features_rest
[N,B,3] (B = (degree + 1)^2 - 1), opacities [N,1] (logits), scales [N,3] (logs), quats [N,4].

The codec, for one column with range [lo, hi] and Q = 2^bits - 1, all in float64:

    inv  = Q / (hi - lo)    (0 when hi == lo)          step = (hi - lo) / Q         -- Python floats, on the host
    code = floor((float64(x) - lo) * inv + 0.5)        x'   = float32(lo + code * step)

so that |x - x'| <= (hi - lo) / (2 Q) up to rounding.  lo and hi come from the data (two floats per column, read back
once).  Every operation is a separate float64 torch op: the CPU, the GPU and tests/kmeans_reference.py's NumPy
restatement agree bit for bit.

    means            uint16 per axis                     19 bytes per Gaussian at SH degree 3 with a codebook
    scales (log)     uint8 per axis                      (6 + 3 + 1 + 3 + 4 + 2), against 236 in the PLY
    opacities        uint8
    features_dc      uint8 per channel
    quats            normalised in float64, uint8 on the fixed range [-1, 1]
    features_rest    rows [N,3B] clustered on the GPU: uint16 labels + a uint8 codebook [K,3B] with one range;
                     sh_clusters = 0: uint8 per column, no codebook; SH degree 0: nothing

The functions are plain torch and run on any device, but the clustering is HIP: a CPU `params` is refused unless
``sh_clusters=0`` (or the model has SH degree 0).
"""
import json
import time
from typing import Dict, Optional

import numpy as np
import torch
from torch import Tensor

FORMAT = "gs-compressed"
VERSION = 1
PARAM_NAMES = ("means", "features_dc", "features_rest", "opacities", "scales", "quats")
BITS = {"means": 16, "scales": 8, "opacities": 8, "features_dc": 8, "quats": 8, "features_rest": 8,
        "sh_labels": 16, "sh_codebook": 8}
MAX_SH_CLUSTERS = 65536  # uint16 labels; gs_fused.kmeans' own limit
_f64 = torch.float64
_COLUMNS = {"means": 3, "features_dc": 3, "opacities": 1, "scales": 3, "quats": 4}


# ---- the codec ------------------------------------------------------------------------------------------------------
def _scales_of(lo: float, hi: float, bits: int):
    q = float(2 ** bits - 1)
    return (q / (hi - lo) if hi > lo else 0.0), (hi - lo) / q


def quantize(x: Tensor, lo, hi, bits: int) -> Tensor:
    """x [N,C] (any float dtype) with per-column ranges ``lo``, ``hi`` (sequences of C Python floats) -> codes [N,C]
    as float64 holding integers in [0, 2^bits - 1]."""
    x = x.to(_f64)
    out = torch.empty_like(x)
    for c in range(x.shape[1]):
        inv, _ = _scales_of(float(lo[c]), float(hi[c]), bits)
        out[:, c] = torch.floor((x[:, c] - float(lo[c])) * inv + 0.5)
    return out


def dequantize(codes: Tensor, lo, hi, bits: int) -> Tensor:
    """codes [N,C] (any integer or float dtype) -> float32 [N,C]: ``float32(lo + code * step)``."""
    q = codes.to(_f64)
    out = torch.empty(q.shape, dtype=torch.float32, device=q.device)
    for c in range(q.shape[1]):
        _, step = _scales_of(float(lo[c]), float(hi[c]), bits)
        out[:, c] = (q[:, c] * step + float(lo[c])).to(torch.float32)
    return out


def _ranges(x: Tensor):
    """-> (lo, hi): per column of x [N,C], as lists of Python floats (the one read-back); zeros for an empty model."""
    if x.shape[0] == 0:
        return [0.0] * x.shape[1], [0.0] * x.shape[1]
    x = x.to(_f64)
    both = torch.stack([x.amin(dim=0), x.amax(dim=0)]).tolist()
    return both[0], both[1]


def _store(codes: Tensor, bits: int) -> np.ndarray:
    return codes.cpu().numpy().astype(np.uint16 if bits == 16 else np.uint8)


def _column_codes(blob: dict, name: str, x: Tensor, lo=None, hi=None) -> None:
    if lo is None:
        lo, hi = _ranges(x)
    blob[name] = _store(quantize(x, lo, hi, BITS[name]), BITS[name])
    blob[name + "_lo"], blob[name + "_hi"] = np.asarray(lo, np.float64), np.asarray(hi, np.float64)


# ---- compress / decompress --------------------------------------------------------------------------------------------
def _checked(params: Dict, op: str) -> Dict[str, Tensor]:
    out = {}
    for name in PARAM_NAMES:
        if name not in params:
            raise ValueError(f"{op}: params has no '{name}'")
        t = params[name]
        t = (t if isinstance(t, Tensor) else torch.as_tensor(np.asarray(t))).detach()
        if not t.is_floating_point():
            raise ValueError(f"{op}: {name} must be a floating-point tensor, got {t.dtype}")
        out[name] = t
    n = out["means"].shape[0]
    dev = out["means"].device
    for name, cols in _COLUMNS.items():
        if out[name].numel() != n * cols or out[name].shape[0] != n:
            raise ValueError(f"{op}: {name} must hold [{n},{cols}] values, got {tuple(out[name].shape)}")
        out[name] = out[name].reshape(n, cols)
    rest = out["features_rest"]
    if rest.dim() != 3 or rest.shape[0] != n or rest.shape[2] != 3:
        raise ValueError(f"{op}: features_rest must be [{n},B,3], got {tuple(rest.shape)}")
    degree = int(round((rest.shape[1] + 1) ** 0.5)) - 1
    if (degree + 1) ** 2 - 1 != rest.shape[1]:
        raise ValueError(f"{op}: features_rest has {rest.shape[1]} bands per channel: not (degree + 1)^2 - 1")
    for name, t in out.items():
        if t.device != dev:
            raise ValueError(f"{op}: {name} is on {t.device}, means on {dev}")
        if t.numel() and not bool(torch.isfinite(t).all()):
            raise ValueError(f"{op}: {name} holds values that are not finite")
    return out


@torch.no_grad()
def compress_gaussians(params: Dict, *, sh_clusters: int = 16384, iters: int = 10, seed: int = 0,
                       weights: Optional[Tensor] = None) -> dict:
    """-> blob: a dict of NumPy arrays (the integer codes, the float64 ``*_lo`` / ``*_hi`` ranges) and ``"meta"``
    (format, version, N, SH degree, K, bit widths) -- what `write_compressed` stores -- plus ``"kmeans"``, a report
    that is not stored (the float64 inertia after each assignment, the seconds the clustering took).

    ``sh_clusters``: rows of the SH codebook (cut to N; at most 65536); 0 keeps features_rest as uint8 per column.
    ``iters``, ``seed``: `gs_fused.kmeans`.  ``weights`` float32 [N], finite and >= 0, e.g.
    ``ContributionStats.weight_sum``: they weigh the codebook's means, not the assignment.

    ValueError: a missing or misshapen parameter, values that are not finite (by name), ``sh_clusters`` outside
    [0, 65536], and CPU parameters with a codebook asked for (the clustering has no CPU fallback)."""
    op = "compress_gaussians"
    p = _checked(params, op)
    if int(sh_clusters) != sh_clusters or not 0 <= sh_clusters <= MAX_SH_CLUSTERS:
        raise ValueError(f"{op}: sh_clusters = {sh_clusters}; 0 (no codebook) <= sh_clusters <= {MAX_SH_CLUSTERS}")
    n = p["means"].shape[0]
    bands = p["features_rest"].shape[1]
    rest = p["features_rest"].reshape(n, 3 * bands)
    clustered = int(sh_clusters) > 0 and bands > 0 and n > 0
    if clustered and not p["means"].is_cuda:
        raise ValueError(f"{op}: the parameters are CPU tensors; the SH codebook is clustered on the GPU (no CPU "
                         f"fallback): move them to a CUDA device, or pass sh_clusters=0")

    blob: dict = {}
    for name in ("means", "scales", "opacities", "features_dc"):
        _column_codes(blob, name, p[name])
    q = p["quats"].to(_f64)
    # (the sum written out: its order is part of the codec, a library reduction's is not)
    q = q / torch.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])[:, None]
    if n and not bool(torch.isfinite(q).all()):
        raise ValueError(f"{op}: quats holds a zero quaternion")
    _column_codes(blob, "quats", q, [-1.0] * 4, [1.0] * 4)

    k, report = 0, None
    if clustered:
        from gs_fused.kmeans import kmeans

        if weights is not None:
            weights = torch.as_tensor(weights).detach().to(device=rest.device)
        torch.cuda.synchronize(rest.device)
        t0 = time.perf_counter()
        res = kmeans(rest.to(torch.float32).contiguous(), int(sh_clusters), iters=iters, seed=seed, weights=weights)
        torch.cuda.synchronize(rest.device)
        report = {"seconds": time.perf_counter() - t0, "iters": int(iters), "inertia": res.inertia.tolist()}
        k = res.centroids.shape[0]
        lo, hi = (float(v) for v in torch.stack([res.centroids.amin(), res.centroids.amax()]).to(_f64).tolist())
        width = rest.shape[1]
        _column_codes(blob, "sh_codebook", res.centroids, [lo] * width, [hi] * width)
        blob["sh_codebook_lo"], blob["sh_codebook_hi"] = np.asarray([lo], np.float64), np.asarray([hi], np.float64)
        blob["sh_labels"] = res.labels.cpu().numpy().astype(np.uint16)
    elif bands > 0:
        _column_codes(blob, "features_rest", rest)
    kept = [name for name in BITS if name in blob]
    blob["meta"] = {"format": FORMAT, "version": VERSION, "num_gaussians": int(n),
                    "sh_degree": int(round((bands + 1) ** 0.5)) - 1, "sh_clusters": int(k),
                    "bits": {name: BITS[name] for name in kept}}
    blob["kmeans"] = report
    return blob


def bytes_per_gaussian(meta: dict) -> int:
    """The per-Gaussian payload in bytes, before zlib and without the codebook and the ranges: the sum of the widths."""
    bands = (meta["sh_degree"] + 1) ** 2 - 1
    cols = dict(_COLUMNS, features_rest=3 * bands, sh_labels=1)
    return sum(bits // 8 * cols[name] for name, bits in meta["bits"].items() if name != "sh_codebook")


def _check_meta(meta, op: str) -> dict:
    if not isinstance(meta, dict) or meta.get("format") != FORMAT:
        raise ValueError(f"{op}: not a {FORMAT} container")
    if meta.get("version") != VERSION:
        raise ValueError(f"{op}: container version {meta.get('version')}, this reader knows version {VERSION}")
    return meta


@torch.no_grad()
def decompress_gaussians(blob: dict, device="cpu") -> Dict[str, Tensor]:
    """-> the six raw parameters in float32 on ``device``, in the layout `gs_io.write_gaussian_ply` takes.  The
    quaternions come back normalised; features_rest is the decoded codebook's row of each label."""
    op = "decompress_gaussians"
    meta = _check_meta(blob.get("meta"), op)
    n, bits = meta["num_gaussians"], meta["bits"]
    bands = (meta["sh_degree"] + 1) ** 2 - 1

    def decode(name, lo=None, hi=None):
        codes = torch.from_numpy(blob[name].astype(np.int64)).to(device)
        lo = blob[name + "_lo"].tolist() if lo is None else lo
        hi = blob[name + "_hi"].tolist() if hi is None else hi
        return dequantize(codes, lo, hi, bits[name])

    out = {name: decode(name) for name in ("means", "features_dc", "opacities", "scales", "quats")}
    if "sh_codebook" in bits:
        width = 3 * bands
        book = decode("sh_codebook", blob["sh_codebook_lo"].tolist() * width, blob["sh_codebook_hi"].tolist() * width)
        labels = torch.from_numpy(blob["sh_labels"].astype(np.int64)).to(device)
        if labels.numel() and int(labels.max()) >= book.shape[0]:
            raise ValueError(f"{op}: a label points outside the codebook of {book.shape[0]} rows")
        rest = book[labels]
    elif "features_rest" in bits:
        rest = decode("features_rest")
    else:
        rest = torch.zeros((n, 0), dtype=torch.float32, device=device)
    out["features_rest"] = rest.reshape(n, bands, 3)
    for name, t in out.items():
        if t.shape[0] != n:
            raise ValueError(f"{op}: {name} holds {t.shape[0]} rows, the metadata says {n}")
    return {name: out[name] for name in PARAM_NAMES}


# ---- the file ---------------------------------------------------------------------------------------------------------
def _arrays(blob: dict) -> Dict[str, np.ndarray]:
    return {k: v for k, v in blob.items() if isinstance(v, np.ndarray)}


def write_compressed(path: str, blob: dict) -> None:
    """One ``.npz`` (`numpy.savez_compressed`: zlib): the integer arrays, the float64 ranges and the metadata as one
    JSON string.  ``path`` is written as given (no suffix is appended)."""
    meta = _check_meta(blob.get("meta"), "write_compressed")
    with open(path, "wb") as f:
        np.savez_compressed(f, meta=np.asarray(json.dumps(meta, sort_keys=True)), **_arrays(blob))


def read_compressed(path: str) -> dict:
    """Inverse of `write_compressed`.  ValueError for another format or version."""
    with np.load(path, allow_pickle=False) as z:
        if "meta" not in z.files:
            raise ValueError(f"read_compressed: not a {FORMAT} container")
        blob = {k: z[k] for k in z.files if k != "meta"}
        blob["meta"] = _check_meta(json.loads(str(z["meta"][()])), "read_compressed")
    return blob


__all__ = ["BITS", "FORMAT", "VERSION", "bytes_per_gaussian", "compress_gaussians", "decompress_gaussians",
           "dequantize", "quantize", "read_compressed", "write_compressed"]
