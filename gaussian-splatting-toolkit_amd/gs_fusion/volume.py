"""`TSDFVolume`: the block-sparse volume and the ctypes wrappers of `gsr_tsdf_*`.

Rules (include/gsraster.h has the buffers, DESIGN.md section 4.5 the reasons): blocks of 8x8x8 voxels are opened
where depth points fall (within `sdf_trunc` per axis), slots are handed out in ascending block index, every voxel of
a touched block that projects onto a usable pixel with `sdf > -sdf_trunc` takes `min(1, sdf / sdf_trunc)` into a
running mean of weight + 1 per observation.  float32 throughout, structure-of-arrays.
"""
import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from rasterizer.cuda import _call, _check, _on, _stream, _typed

_f32 = torch.float32
# rows of the `state` tensor (csrc/tsdf.hip)
ST_ALLOCATED, ST_LIST, ST_OVERFLOW, ST_NEEDED, ST_PENDING, ST_POINTS, ST_VERTICES, ST_TRIANGLES = range(8)


class _Volume(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("voxel_length", C.c_float), ("sdf_trunc", C.c_float),
                ("blocks", C.c_int * 3), ("capacity", C.c_int), ("table", C.c_void_p), ("tsdf", C.c_void_p),
                ("weight", C.c_void_p), ("color", C.c_void_p), ("state", C.c_void_p)]


class _View(C.Structure):
    _fields_ = [("height", C.c_uint), ("width", C.c_uint), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("depth_trunc", C.c_float), ("viewmat", C.c_float * 12),
                ("cam2world", C.c_float * 12), ("depth", C.c_void_p), ("color", C.c_void_p), ("valid", C.c_void_p)]


def invert_viewmat(viewmat) -> np.ndarray:
    """world->camera [4,4] -> camera->world: inverted in fp64 on the host, rounded to fp32."""
    return np.linalg.inv(np.asarray(viewmat, np.float64)).astype(np.float32)


def _host_matrix(viewmat) -> np.ndarray:
    if isinstance(viewmat, Tensor):
        viewmat = viewmat.detach().cpu().numpy()  # (a CUDA tensor costs a read-back: hand in the host copy)
    m = np.asarray(viewmat, np.float32)
    if m.shape == (3, 4):
        m = np.concatenate([m, np.array([[0, 0, 0, 1]], np.float32)])
    if m.shape != (4, 4):
        raise ValueError("viewmat must be [4,4] or [3,4]")
    return m


class TSDFVolume:
    def __init__(self, voxel_length: float, sdf_trunc: float, origin: Sequence[float], blocks: Sequence[int],
                 capacity: int, device="cuda:0"):
        self.voxel_length, self.sdf_trunc = float(voxel_length), float(sdf_trunc)
        self.origin = tuple(float(o) for o in origin)
        self.blocks = tuple(int(b) for b in blocks)  # (Bx, By, Bz)
        self.capacity = int(capacity)
        self.device = torch.device(device)
        if len(self.origin) != 3 or len(self.blocks) != 3:
            raise ValueError("origin and blocks have three entries")
        if min(self.blocks) <= 0 or self.capacity <= 0 or self.voxel_length <= 0 or self.sdf_trunc <= 0:
            raise ValueError("blocks, capacity, voxel_length and sdf_trunc must be positive")
        if self.device.type != "cuda":
            raise RuntimeError("TSDFVolume lives on a CUDA device")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        Bx, By, Bz = self.blocks
        self.num_blocks = Bx * By * Bz
        L = _typed()
        ws_alloc = L.gsr_tsdf_allocate_workspace_bytes(self.num_blocks)
        if ws_alloc == 0 or L.gsr_tsdf_extract_mesh_workspace_bytes(self.num_blocks, self.capacity) == 0:
            raise ValueError("too many blocks or too large a pool")
        dev = self.device
        with _on(dev):
            self.table = torch.full((Bz, By, Bx), -1, dtype=torch.int32, device=dev)
            # the pool is initialised block by block as slots are handed out, not here
            self.tsdf = torch.empty((self.capacity, 512), dtype=_f32, device=dev)
            self.weight = torch.empty((self.capacity, 512), dtype=_f32, device=dev)
            self.color = torch.empty((self.capacity, 512, 3), dtype=_f32, device=dev)
            self._state = torch.zeros(8, dtype=torch.int32, device=dev)
            self._flags = torch.zeros(self.num_blocks, dtype=torch.uint8, device=dev)
            self._list = torch.empty(self.num_blocks, dtype=torch.int32, device=dev)
            self._ws_alloc = torch.empty(ws_alloc, dtype=torch.uint8, device=dev)

    @classmethod
    def from_bounds(cls, lo: Sequence[float], hi: Sequence[float], voxel_length: float, sdf_trunc: float,
                    capacity: Optional[int] = None, device="cuda:0") -> "TSDFVolume":
        """The smallest whole number of blocks that covers the box [lo, hi]; `capacity` None: every block."""
        lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        blocks = np.maximum(1, np.ceil((hi - lo) / (8.0 * voxel_length) - 1e-9)).astype(int)
        cap = int(np.prod(blocks)) if capacity is None else int(capacity)
        return cls(voxel_length, sdf_trunc, lo.tolist(), blocks.tolist(), cap, device)

    # ---- descriptors ------------------------------------------------------------------------------------------------
    def _desc(self) -> _Volume:
        return _Volume((C.c_float * 3)(*self.origin), self.voxel_length, self.sdf_trunc, (C.c_int * 3)(*self.blocks),
                       self.capacity, self.table.data_ptr(), self.tsdf.data_ptr(), self.weight.data_ptr(),
                       self.color.data_ptr(), self._state.data_ptr())

    # ---- integration ------------------------------------------------------------------------------------------------
    def integrate(self, depth: Tensor, color: Tensor, fx: float, fy: float, cx: float, cy: float, viewmat,
                  valid: Optional[Tensor] = None, depth_trunc: float = 10.0) -> None:
        """Fuse one view: `depth` [H,W] (or [H,W,1]) z-depth, `color` [H,W,3], `valid` [H,W] uint8 / bool or None,
        all CUDA; `viewmat` world->camera [4,4] as a HOST array (the convention of `harness.scene.Camera`).  Three
        native calls on the current stream; nothing is read back."""
        _check(depth, "depth", _f32)
        _check(color, "color", _f32)
        if depth.dim() == 3 and depth.size(2) == 1:
            depth = depth[..., 0]
        if depth.dim() != 2 or color.shape != (depth.size(0), depth.size(1), 3):
            raise RuntimeError("depth must be [H,W] and color [H,W,3]")
        if depth.device != self.device or color.device != self.device:
            raise RuntimeError(f"depth and color must be on {self.device}")
        vptr = None
        if valid is not None:
            _check(valid, "valid")
            if valid.dtype not in (torch.uint8, torch.bool) or valid.shape != depth.shape or valid.device != self.device:
                raise RuntimeError("valid must be a uint8 / bool [H,W] tensor on the volume's device")
            vptr = valid.data_ptr()
        view = self._view_desc(depth, color, fx, fy, cx, cy, viewmat, vptr, depth_trunc)
        vol = self._desc()
        dev = self.device
        with _on(dev):
            s = _stream(dev)
            self._touch_allocate(vol, view, s)
            self._integrate_listed(vol, view, s)

    @staticmethod
    def _view_desc(depth, color, fx, fy, cx, cy, viewmat, valid_ptr, depth_trunc) -> _View:
        V = _host_matrix(viewmat)
        inv = invert_viewmat(V)
        H, W = depth.shape[0], depth.shape[1]
        return _View(H, W, fx, fy, cx, cy, depth_trunc, (C.c_float * 12)(*V[:3].reshape(-1).tolist()),
                     (C.c_float * 12)(*inv[:3].reshape(-1).tolist()), depth.data_ptr(), color.data_ptr(), valid_ptr)

    # (the two halves of a view, apart: tools/fusion_bench.py times them separately)
    def _touch_allocate(self, vol: _Volume, view: _View, s) -> None:
        _call("gsr_tsdf_touch", C.byref(vol), C.byref(view), self._flags, s)
        _call("gsr_tsdf_allocate", C.byref(vol), self._flags, self._list, self._ws_alloc, self._ws_alloc.numel(), s)

    def _integrate_listed(self, vol: _Volume, view: _View, s) -> None:
        _call("gsr_tsdf_integrate", C.byref(vol), C.byref(view), self._list, s)

    # ---- extraction -------------------------------------------------------------------------------------------------
    def _read_state(self) -> np.ndarray:
        st = self._state.cpu().numpy()  # the one read-back of an extraction
        if st[ST_OVERFLOW]:
            raise RuntimeError(f"TSDF volume overflow: {int(st[ST_ALLOCATED])} blocks allocated, "
                               f"{int(st[ST_NEEDED])} needed (capacity {self.capacity})")
        return st

    def extract_point_cloud(self, return_axis: bool = False):
        """-> points [M,3], colors [M,3], normals [M,3] (and the axis [M] of each point's edge), ordered by
        (block, voxel, axis)."""
        dev = self.device
        vol = self._desc()
        with _on(dev):
            s = _stream(dev)
            n = _typed().gsr_tsdf_extract_points_workspace_bytes(self.num_blocks)
            ws = torch.empty(n, dtype=torch.uint8, device=dev)
            _call("gsr_tsdf_extract_points_count", C.byref(vol), ws, n, s)
            m = int(self._read_state()[ST_POINTS])
            points, colors, normals = (torch.empty((m, 3), dtype=_f32, device=dev) for _ in range(3))
            axis = torch.empty(m, dtype=torch.int32, device=dev)
            _call("gsr_tsdf_extract_points_emit", C.byref(vol), ws, n, m, points, colors, normals, axis, s)
        return (points, colors, normals, axis) if return_axis else (points, colors, normals)

    def extract_mesh(self) -> Tuple[Tensor, Tensor, Tensor]:
        """Surface nets -> vertices [V,3], vertex_colors [V,3], triangles [F,3] int32 (normals towards free space)."""
        dev = self.device
        vol = self._desc()
        with _on(dev):
            s = _stream(dev)
            n = _typed().gsr_tsdf_extract_mesh_workspace_bytes(self.num_blocks, self.capacity)
            ws = torch.empty(n, dtype=torch.uint8, device=dev)
            _call("gsr_tsdf_extract_mesh_count", C.byref(vol), ws, n, s)
            st = self._read_state()
            nv, nt = int(st[ST_VERTICES]), int(st[ST_TRIANGLES])
            vertices, vcolors = (torch.empty((nv, 3), dtype=_f32, device=dev) for _ in range(2))
            triangles = torch.empty((nt, 3), dtype=torch.int32, device=dev)
            _call("gsr_tsdf_extract_mesh_emit", C.byref(vol), ws, n, nv, nt, vertices, vcolors, triangles, s)
        return vertices, vcolors, triangles

    # ---- state ------------------------------------------------------------------------------------------------------
    @property
    def num_allocated_blocks(self) -> int:
        return int(self._state[ST_ALLOCATED].item())

    def state_dict(self) -> Dict:
        """Geometry, table and pool (rows of slots not handed out yet are zeroed) -- enough to resume a fusion."""
        st = self._state.cpu().numpy()
        n = int(st[ST_ALLOCATED])
        pool = {}
        for k in ("tsdf", "weight", "color"):
            t = getattr(self, k).clone()
            t[n:] = 0
            pool[k] = t
        return {"voxel_length": self.voxel_length, "sdf_trunc": self.sdf_trunc,
                "origin": np.asarray(self.origin, np.float32), "blocks": self.blocks, "capacity": self.capacity,
                "table": self.table.clone(), "num_allocated": n, "overflow": bool(st[ST_OVERFLOW]),
                "needed": int(st[ST_NEEDED]), **pool}

    def load_state_dict(self, sd: Dict) -> None:
        """Inverse of `state_dict`; numpy arrays or tensors.  Blocks and capacity must be this volume's."""
        if tuple(int(b) for b in sd["blocks"]) != self.blocks or int(sd["capacity"]) != self.capacity:
            raise ValueError("state_dict was taken from a volume with other blocks / capacity")
        self.voxel_length, self.sdf_trunc = float(sd["voxel_length"]), float(sd["sdf_trunc"])
        self.origin = tuple(float(o) for o in np.asarray(sd["origin"]).reshape(3))
        table = torch.as_tensor(sd["table"]).to(torch.int32)
        n = int(sd["num_allocated"])
        used = table[table >= 0]
        if table.shape != self.table.shape or n < 0 or n > self.capacity or int(table.max()) >= n \
                or used.numel() != n or torch.unique(used).numel() != n:
            raise ValueError("state_dict: table does not name each of num_allocated slots once")
        self.table.copy_(table)
        for k in ("tsdf", "weight", "color"):
            src = torch.as_tensor(sd[k]).to(_f32)
            if src.shape != getattr(self, k).shape:
                raise ValueError(f"state_dict: {k} has shape {tuple(src.shape)}")
            getattr(self, k).copy_(src)
        st = torch.zeros(8, dtype=torch.int32)
        st[ST_ALLOCATED], st[ST_OVERFLOW] = n, int(bool(sd.get("overflow", False)))
        st[ST_NEEDED] = int(sd.get("needed", n))
        self._state.copy_(st)
        self._flags.zero_()
