"""Case files for tools/standin/knn_main.cpp: the small inputs of the GPU tests (n, m <= 300) and what the float32
restatement returns for them.    python tools/standin/knn_cases.py DIR"""
import os
import sys

import numpy as np

OUT = sys.argv[1]
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..', 'tests'))
import knn_reference as R
def put(name, P, Q, k, rc=0):
    self_mode = Q is None
    if rc == 0:
        d, i = R.brute32(P, Q, k)
    else:
        m = len(P) if self_mode else len(Q); d = np.zeros((m, k), np.float32); i = np.zeros((m, k), np.int32)
    Qa = np.zeros((0, 3), np.float32) if self_mode else Q
    m = len(P) if self_mode else len(Q)
    bad = int((~np.isfinite(P if self_mode else Q).all(1)).sum())
    with open(os.path.join(OUT, f'{name}.bin'), 'wb') as f:
        f.write(np.array([len(P), m, k, int(self_mode), rc, bad], np.int32).tobytes())
        if self_mode: Qa = np.zeros((m, 3), np.float32)
        f.write(P.astype(np.float32).tobytes()); f.write(Qa.astype(np.float32).tobytes()); f.write(d.astype(np.float32).tobytes()); f.write(i.astype(np.int32).tobytes())
c = 0
for case in R.small_cases():
    name, n, m, k = case
    if n > 300 or (m or 0) > 300: continue
    P, Q, k = R.case_inputs(case); put(f'{c:03d}_{name}_{n}_{m}_{k}', P, Q, k); c += 1
P = R.cloud('uniform', 65).copy(); P[[3, 40]] = [[np.nan, 0, 0], [0, np.inf, 0]]
Q = R.queries('uniform', 65, 63).copy(); Q[5, 2], Q[62, 0] = -np.inf, np.nan
put('900_nonfinite_q', P, Q, 3); put('901_nonfinite_self', P, None, 3)
P2 = R.cloud('uniform', 65).copy(); P2[4:] = np.nan
put('902_toofew_self', P2, None, 4, rc=-4); put('903_toofew_q', P2, P2[:2], 5, rc=-4); put('904_enough', P2, P2[:2], 4)
print(c + 5, 'case files')
