"""Case files for tools/standin/mono_depth_main.cpp: the golden cases of tests/golden/cogs_losses.npz and the edge cases
of the GPU tests at small sizes, with what the float64 restatement (tests/mono_depth_reference.py) returns for them.
    python tools/standin/mono_depth_cases.py DIR"""
import os
import sys

import numpy as np

OUT = sys.argv[1]
TESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests")
sys.path.insert(0, TESTS)
import mono_depth_reference as M


def put(name, pred, gt, img, box, rows, cols, scale=1.0, shift=0.0, mask=None, idx64=True):
    """header int32 [6]: H, W, box, n_corr, idx64, masked; float32 [2] scale, shift; pred, gt [H,W], img [H,W,3],
    mask [H,W] if masked; rows, cols; then float64: the three losses (local Pearson, log-depth, TV) and their three
    [H,W] gradients."""
    H, W = pred.shape
    scale, shift = float(np.float32(scale)), float(np.float32(shift))
    p, g = (pred.astype(np.float64), gt.astype(np.float64)) if mask is None else M.products(pred, gt, mask)
    want = [M.local_pearson(p, g, box, rows, cols, mask), M.log_depth(p, g, img, scale, shift, mask), M.tv(p, mask)]
    it = np.int64 if idx64 else np.int32
    with open(os.path.join(OUT, f"{name}.bin"), "wb") as f:
        f.write(np.array([H, W, box, len(rows), int(idx64), int(mask is not None)], np.int32).tobytes())
        f.write(np.array([scale, shift], np.float32).tobytes())
        for a in (pred, gt, img) + (() if mask is None else (mask,)):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
        f.write(np.asarray(rows, it).tobytes())
        f.write(np.asarray(cols, it).tobytes())
        f.write(np.array([w[0] for w in want], np.float64).tobytes())
        for w in want:
            f.write(np.ascontiguousarray(w[1], np.float64).tobytes())


z = np.load(os.path.join(TESTS, "golden", "cogs_losses.npz"))
for c in ("c0", "c1", "c2"):
    put(f"0_{c}", z[c + "_pred"], z[c + "_gt"], z[c + "_img"], int(z[c + "_box_pcorr"][0]), z[c + "_patch_rows"],
        z[c + "_patch_cols"], *z[c + "_scale_shift"])
rng = np.random.default_rng(1)
pred, gt, img = M.smooth_noise(33, 47, 2)
rows, cols = rng.integers(0, 33 - 17 + 1, 12), rng.integers(0, 47 - 17 + 1, 12)
put("1_box17_int32", pred, gt, img, 17, rows, cols, 0.9, 0.15, idx64=False)
put("1_box17_masked", pred, gt, img, 17, rows, cols, 0.9, 0.15, mask=rng.uniform(0, 1.5, (33, 47)).astype(np.float32))
put("1_box17_mask_zero", pred, gt, img, 17, rows, cols, mask=np.zeros((33, 47), np.float32))
put("2_out_of_range", pred, gt, img, 17, np.array([0, 17, -1, 2 ** 40, 3]), np.array([0, 5, 2, 1, 31]))
put("2_no_patches", pred, gt, img, 17, np.zeros(0, np.int64), np.zeros(0, np.int64))
flat = pred.copy()
flat[4:12, 6:14] = 2.5
put("2_constant_patch", flat, gt, img, 8, np.array([4, 20, 4]), np.array([6, 30, 7]))
put("2_box1", pred, gt, img, 1, np.array([3]), np.array([4]))
put("2_whole_image", pred[:30, :30], gt[:30, :30], img[:30, :30], 30, np.array([0]), np.array([0]))
pred, gt, img = M.smooth_noise(20, 70, 3)
put("3_600_patches", pred, gt, img, 3, rng.integers(0, 18, 600), rng.integers(0, 68, 600))
tie = pred.copy()
tie[5, 5] = tie[5, 6] = tie[6, 5]
gt2 = gt.copy()
gt2[7, 3] = tie[7, 3]
put("4_ties", tie, gt2, img, 3, np.array([4]), np.array([4]))
put("4_one_row", pred[:1], gt[:1], img[:1], 1, np.array([0]), np.array([2]))
put("4_one_column", pred[:, :1], gt[:, :1], img[:, :1], 1, np.array([2]), np.array([0]))
print(len(os.listdir(OUT)), "case files")
