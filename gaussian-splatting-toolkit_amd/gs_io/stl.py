"""STL triangle soups (the ground-truth format of gs_toolkit/evaluation/surface_distance), binary and ASCII."""
import os

import numpy as np

_RECORD = np.dtype([("normal", "<f4", 3), ("vertices", "<f4", (3, 3)), ("attribute", "<u2")])  # 50 bytes


def read_stl(path: str) -> np.ndarray:
    """-> float32 [F,3,3]: the three vertices of every facet (normals and attribute words are dropped).

    The format is told by the file's size against the triangle count a binary file declares in bytes 80-83 -- not by
    a leading `solid`, which binary files often carry in their header too.  Anything else is parsed as ASCII and must
    hold complete facets up to `endsolid`; a truncated file of either kind raises ValueError."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(84)
        if len(head) == 84:
            count = int(np.frombuffer(head, "<u4", 1, 80)[0])
            if size == 84 + 50 * count:
                rec = np.frombuffer(f.read(50 * count), _RECORD, count)
                return np.ascontiguousarray(rec["vertices"], np.float32).reshape(-1, 3, 3)
        f.seek(0)
        data = f.read()
    try:
        tok = data.decode("ascii").split()
    except UnicodeDecodeError:
        raise ValueError(f"{path}: neither a binary STL of the size its header declares ({size} bytes) nor ASCII") from None
    if not tok or tok[0] != "solid":
        raise ValueError(f"{path}: not an STL file")
    if "endsolid" not in tok:
        raise ValueError(f"{path}: truncated ASCII STL (no endsolid)")
    tok = tok[:tok.index("endsolid")]
    at = [i for i, w in enumerate(tok) if w == "vertex"]
    loops, ends = tok.count("loop"), tok.count("endloop")
    if len(at) % 3 or loops != ends or 3 * loops != len(at) or (at and at[-1] + 3 >= len(tok)):
        raise ValueError(f"{path}: truncated or malformed ASCII STL")
    try:
        v = np.array([[float(tok[i + 1]), float(tok[i + 2]), float(tok[i + 3])] for i in at], np.float64)
    except ValueError:
        raise ValueError(f"{path}: malformed vertex in ASCII STL") from None
    return v.astype(np.float32).reshape(-1, 3, 3)
