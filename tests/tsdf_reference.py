"""Float32 NumPy restatement of the TSDF fusion rules -- the oracle of test_tsdf_host.py and
test_gpu_tsdf.py -- plus the analytic scenes and the mesh checks those tests share.  A helper module, not a test.

Every operation is carried out on ``np.float32`` values in the order the rules give, so that the HIP kernels
(csrc/tsdf.hip, compiled without FMA contraction, correctly rounded division and square root) produce the same bits.

Orders that the rules leave to the implementation and that both sides follow:
  * a matrix row times a point is ``((m0*x + m1*y) + m2*z) + m3``;
  * voxel index in a block is ``(lz*8 + ly)*8 + lx``; linear block index is ``(bz*By + by)*Bx + bx``;
  * the sign of a mesh corner is ``f < 0``; a cell's crossing edges are visited axis x, y, z and, for axis ``a`` with
    ``(a, b, c)`` cyclic, offsets ``(db, dc)`` = (0,0), (1,0), (0,1), (1,1); the vertex is their running sum divided
    by their number;
  * faces are ordered by (block, voxel, axis) of the edge's lower voxel ``v0``; with ``q0 = v0-eb-ec, q1 = v0-ec,
    q2 = v0, q3 = v0-eb`` the two triangles are (q0,q1,q2),(q0,q2,q3) when ``f0 < 0`` and (q0,q2,q1),(q0,q3,q2)
    otherwise;
  * a blended normal is ``(g0*r1 + g1*r0)/(r0 + r1)`` divided by ``sqrt((nx*nx + ny*ny) + nz*nz)`` (zero if that is 0).
"""
import functools
import math

import numpy as np

F = np.float32
QUALIFY = F(0.98)
AMBIG_PIXEL = 1e-4
AMBIG_VALUE = 1e-6


def invert_viewmat(viewmat):
    """world->camera [4,4] -> camera->world: fp64 inverse rounded to fp32."""
    return np.linalg.inv(np.asarray(viewmat, np.float64)).astype(np.float32)


def _row(m, a, x, y, z):
    return ((m[a, 0] * x + m[a, 1] * y) + m[a, 2] * z) + m[a, 3]


class RefVolume:
    def __init__(self, voxel_length, sdf_trunc, origin, blocks, capacity):
        self.L = F(voxel_length)
        self.trunc = F(sdf_trunc)
        self.origin = np.asarray(origin, np.float32).copy()
        self.blocks = tuple(int(b) for b in blocks)  # (Bx, By, Bz)
        self.capacity = int(capacity)
        Bx, By, Bz = self.blocks
        self.table = np.full((Bz, By, Bx), -1, np.int32)
        self.tsdf = np.zeros((capacity, 512), np.float32)
        self.weight = np.zeros((capacity, 512), np.float32)
        self.color = np.zeros((capacity, 512, 3), np.float32)
        self.num_allocated = 0
        self.overflow = False
        self.needed = 0

    # ---- state shared with gs_fusion.TSDFVolume ---------------------------------------------------------------------
    def state_dict(self):
        return {"voxel_length": float(self.L), "sdf_trunc": float(self.trunc), "origin": self.origin.copy(),
                "blocks": self.blocks, "capacity": self.capacity, "table": self.table.copy(),
                "tsdf": self.tsdf.copy(), "weight": self.weight.copy(), "color": self.color.copy(),
                "num_allocated": self.num_allocated, "overflow": bool(self.overflow), "needed": int(self.needed)}

    # ---- integration ------------------------------------------------------------------------------------------------
    def flagged_blocks(self, depth, fx, fy, cx, cy, viewmat, valid=None, depth_trunc=10.0):
        """Step 1: ascending linear indices of the blocks this view touches."""
        depth = np.asarray(depth, np.float32)
        H, W = depth.shape
        fx, fy, cx, cy = F(fx), F(fy), F(cx), F(cy)
        c2w = invert_viewmat(viewmat)
        usable = (depth > 0) & (depth <= F(depth_trunc))
        if valid is not None:
            usable &= np.asarray(valid) != 0
        ii, jj = np.nonzero(usable)
        d = depth[ii, jj]
        xn = ((jj.astype(np.float32) + F(0.5)) - cx) / fx
        yn = ((ii.astype(np.float32) + F(0.5)) - cy) / fy
        x, y = xn * d, yn * d
        L8 = F(8) * self.L
        lo, hi = [], []
        for a in range(3):
            pw = _row(c2w, a, x, y, d)
            l = np.floor(((pw - self.trunc) - self.origin[a]) / L8)
            h = np.floor(((pw + self.trunc) - self.origin[a]) / L8)
            lo.append(np.maximum(l, F(0)).astype(np.int64))
            hi.append(np.minimum(h, F(self.blocks[a] - 1)).astype(np.int64))
        Bx, By, Bz = self.blocks
        flags = np.zeros((Bz, By, Bx), bool)
        if len(d):
            boxes = np.unique(np.stack(lo + hi, 1), axis=0)
            for x0, y0, z0, x1, y1, z1 in boxes:
                if x0 <= x1 and y0 <= y1 and z0 <= z1:
                    flags[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = True
        return np.nonzero(flags.reshape(-1))[0]

    def integrate(self, depth, color, fx, fy, cx, cy, viewmat, valid=None, depth_trunc=10.0):
        """One view.  -> dict: flagged (linear block indices), slots (of the integrated ones), updated / ambig / sdf
        [n_integrated, 512] (sdf is NaN where the voxel was skipped before its sdf was formed)."""
        depth = np.asarray(depth, np.float32)
        color = np.asarray(color, np.float32)
        H, W = depth.shape
        viewmat = np.asarray(viewmat, np.float32)
        flagged = self.flagged_blocks(depth, fx, fy, cx, cy, viewmat, valid, depth_trunc)
        fx, fy, cx, cy = F(fx), F(fy), F(cx), F(cy)
        dt = F(depth_trunc)
        # step 2: slots in ascending linear block index
        flat = self.table.reshape(-1)
        new = flagged[flat[flagged] < 0]
        self.needed = max(self.needed, self.num_allocated + len(new))
        room = self.capacity - self.num_allocated
        if len(new) > room:
            self.overflow = True
            new = new[:room]
        flat[new] = self.num_allocated + np.arange(len(new), dtype=np.int32)
        self.num_allocated += len(new)
        blocks = flagged[flat[flagged] >= 0]
        slots = flat[blocks]
        info = {"flagged": flagged, "blocks": blocks, "slots": slots}
        n = len(blocks)
        if n == 0:
            z = np.zeros((0, 512), bool)
            info.update(updated=z, ambig=z.copy(), sdf=np.zeros((0, 512), np.float32))
            return info
        # step 3
        Bx, By, Bz = self.blocks
        bx, by, bz = blocks % Bx, (blocks // Bx) % By, blocks // (Bx * By)
        v = np.arange(512)
        gx = (bx[:, None] * 8 + (v & 7)[None]).astype(np.float32)
        gy = (by[:, None] * 8 + ((v >> 3) & 7)[None]).astype(np.float32)
        gz = (bz[:, None] * 8 + (v >> 6)[None]).astype(np.float32)
        px = self.origin[0] + (gx + F(0.5)) * self.L
        py = self.origin[1] + (gy + F(0.5)) * self.L
        pz = self.origin[2] + (gz + F(0.5)) * self.L
        cxm = _row(viewmat, 0, px, py, pz)
        cym = _row(viewmat, 1, px, py, pz)
        czm = _row(viewmat, 2, px, py, pz)
        live = czm > 0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            czs = np.where(live, czm, F(1))
            u = fx * (cxm / czs) + cx
            w_ = fy * (cym / czs) + cy
            ju, iv = np.floor(u), np.floor(w_)
            ambig = live & ((np.abs(u - np.rint(u)) < AMBIG_PIXEL) | (np.abs(w_ - np.rint(w_)) < AMBIG_PIXEL))
            live &= (ju >= 0) & (ju < W) & (iv >= 0) & (iv < H)
            j = np.where(live, ju, 0).astype(np.int64)
            i = np.where(live, iv, 0).astype(np.int64)
            d = depth[i, j]
            ambig |= live & (np.abs(d.astype(np.float64) - float(dt)) < AMBIG_VALUE)
            usable = (d > 0) & (d <= dt)
            if valid is not None:
                usable &= np.asarray(valid)[i, j] != 0
            live &= usable
            xn = ((j.astype(np.float32) + F(0.5)) - cx) / fx
            yn = ((i.astype(np.float32) + F(0.5)) - cy) / fy
            m = np.sqrt((F(1) + xn * xn) + yn * yn)
            sdf = (d - czm) * m
            ambig |= live & (np.abs(sdf.astype(np.float64) + float(self.trunc)) < AMBIG_VALUE)
            upd = live & (sdf > -self.trunc)
            f = np.minimum(F(1), sdf / self.trunc)
        w = self.weight[slots]
        w1 = w + F(1)
        t_new = (self.tsdf[slots] * w + f) / w1
        self.tsdf[slots] = np.where(upd, t_new, self.tsdf[slots])
        c_pix = color[i, j]
        c_new = (self.color[slots] * w[..., None] + c_pix) / w1[..., None]
        self.color[slots] = np.where(upd[..., None], c_new, self.color[slots])
        self.weight[slots] = np.where(upd, w1, w)
        info.update(updated=upd, ambig=ambig, sdf=np.where(live, sdf, F(np.nan)))
        return info

    # ---- extraction -------------------------------------------------------------------------------------------------
    def _dense(self):
        Bx, By, Bz = self.blocks
        Fd = np.zeros((Bz * 8, By * 8, Bx * 8), np.float32)
        Wd = np.zeros_like(Fd)
        Cd = np.zeros(Fd.shape + (3,), np.float32)
        for b in np.nonzero(self.table.reshape(-1) >= 0)[0]:
            s = self.table.reshape(-1)[b]
            x0, y0, z0 = (b % Bx) * 8, ((b // Bx) % By) * 8, (b // (Bx * By)) * 8
            Fd[z0:z0 + 8, y0:y0 + 8, x0:x0 + 8] = self.tsdf[s].reshape(8, 8, 8)
            Wd[z0:z0 + 8, y0:y0 + 8, x0:x0 + 8] = self.weight[s].reshape(8, 8, 8)
            Cd[z0:z0 + 8, y0:y0 + 8, x0:x0 + 8] = self.color[s].reshape(8, 8, 8, 3)
        return Fd, Wd, Cd

    def _key(self, z, y, x):
        Bx, By, _ = self.blocks
        b = ((z >> 3) * By + (y >> 3)) * Bx + (x >> 3)
        return b * 512 + (((z & 7) * 8 + (y & 7)) * 8 + (x & 7))

    def _centre(self, idx, a):
        return self.origin[a] + (idx.astype(np.float32) + F(0.5)) * self.L

    def _check_overflow(self):
        if self.overflow:
            raise RuntimeError(f"TSDF volume overflow: {self.num_allocated} blocks allocated, {self.needed} needed")

    def extract_point_cloud(self):
        """-> points [M,3], colors [M,3], normals [M,3], axis [M]"""
        self._check_overflow()
        Fd, Wd, Cd = self._dense()
        Q = (Wd > 0) & (np.abs(Fd) < QUALIFY)
        # gradients: central differences over observed neighbours, the centre value where one is missing
        Fp = np.pad(Fd, 1)
        Wp = np.pad(Wd, 1)
        G = np.zeros(Fd.shape + (3,), np.float32)
        core = (slice(1, -1),) * 3
        for a in range(3):
            ax = 2 - a
            hi = tuple(slice(2, None) if k == ax else slice(1, -1) for k in range(3))
            lo = tuple(slice(0, -2) if k == ax else slice(1, -1) for k in range(3))
            fp = np.where(Wp[hi] > 0, Fp[hi], Fp[core])
            fm = np.where(Wp[lo] > 0, Fp[lo], Fp[core])
            G[..., a] = fp - fm
        rows = []
        for a in range(3):
            ax = 2 - a
            s0 = tuple(slice(0, -1) if k == ax else slice(None) for k in range(3))
            s1 = tuple(slice(1, None) if k == ax else slice(None) for k in range(3))
            cond = Q[s0] & Q[s1] & (Fd[s0] * Fd[s1] < 0)
            z, y, x = np.nonzero(cond)
            idx0 = (z, y, x)
            idx1 = tuple(c + (1 if k == ax else 0) for k, c in enumerate(idx0))
            r0, r1 = np.abs(Fd[idx0]), np.abs(Fd[idx1])
            den = r0 + r1
            p = np.stack([self._centre(x, 0), self._centre(y, 1), self._centre(z, 2)], 1)
            g = (x, y, z)[a]
            p[:, a] = (self._centre(g, a) * r1 + self._centre(g + 1, a) * r0) / den
            c = (Cd[idx0] * r1[:, None] + Cd[idx1] * r0[:, None]) / den[:, None]
            nrm = (G[idx0] * r1[:, None] + G[idx1] * r0[:, None]) / den[:, None]
            ln = np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])
            nrm = np.where(ln[:, None] > 0, nrm / np.where(ln > 0, ln, F(1))[:, None], F(0))
            rows.append((self._key(z, y, x) * 3 + a, p, c, nrm.astype(np.float32), np.full(len(z), a, np.int32)))
        key = np.concatenate([r[0] for r in rows])
        order = np.argsort(key, kind="stable")
        cat = lambda k: np.concatenate([r[k] for r in rows])[order]  # noqa: E731
        return cat(1), cat(2), cat(3), cat(4)

    def extract_mesh(self):
        """-> vertices [V,3], vertex_colors [V,3], triangles [F,3] int32 (surface nets)"""
        self._check_overflow()
        Fd, Wd, Cd = self._dense()
        Z, Y, X = Fd.shape
        Q = (Wd > 0) & (np.abs(Fd) < QUALIFY)
        N = Fd < 0
        cs = lambda dz, dy, dx: (slice(dz, Z - 1 + dz), slice(dy, Y - 1 + dy), slice(dx, X - 1 + dx))  # noqa: E731
        allq = np.ones((Z - 1, Y - 1, X - 1), bool)
        anyn = np.zeros_like(allq)
        alln = np.ones_like(allq)
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    allq &= Q[cs(dz, dy, dx)]
                    anyn |= N[cs(dz, dy, dx)]
                    alln &= N[cs(dz, dy, dx)]
        active = np.zeros((Z, Y, X), bool)
        active[:Z - 1, :Y - 1, :X - 1] = allq & anyn & ~alln
        z, y, x = np.nonzero(active)
        order = np.argsort(self._key(z, y, x), kind="stable")
        z, y, x = z[order], y[order], x[order]
        V = len(z)
        vidx = np.full((Z, Y, X), -1, np.int64)
        vidx[z, y, x] = np.arange(V)
        base = (x, y, z)
        psum = np.zeros((V, 3), np.float32)
        csum = np.zeros((V, 3), np.float32)
        cnt = np.zeros(V, np.float32)
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            for dc in (0, 1):
                for db in (0, 1):
                    g0 = [base[0].copy(), base[1].copy(), base[2].copy()]
                    g0[b] = g0[b] + db
                    g0[c] = g0[c] + dc
                    g1 = [g.copy() for g in g0]
                    g1[a] = g1[a] + 1
                    i0, i1 = (g0[2], g0[1], g0[0]), (g1[2], g1[1], g1[0])
                    cross = N[i0] != N[i1]
                    r0, r1 = np.abs(Fd[i0]), np.abs(Fd[i1])
                    den = np.where(cross, r0 + r1, F(1))
                    p = np.stack([self._centre(g0[k], k) for k in range(3)], 1)
                    p[:, a] = (self._centre(g0[a], a) * r1 + self._centre(g1[a], a) * r0) / den
                    col = (Cd[i0] * r1[:, None] + Cd[i1] * r0[:, None]) / den[:, None]
                    psum = np.where(cross[:, None], psum + p, psum)
                    csum = np.where(cross[:, None], csum + col, csum)
                    cnt = np.where(cross, cnt + F(1), cnt)
        verts = psum / cnt[:, None]
        cols = csum / cnt[:, None]
        # faces
        tris, keys = [], []
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            ax = 2 - a
            s0 = tuple(slice(0, -1) if k == ax else slice(None) for k in range(3))
            s1 = tuple(slice(1, None) if k == ax else slice(None) for k in range(3))
            zz, yy, xx = np.nonzero(N[s0] != N[s1])
            g = [xx, yy, zz]
            ok = (g[b] >= 1) & (g[c] >= 1)
            g = [k[ok] for k in g]

            def cell(db, dc):
                h = [k.copy() for k in g]
                h[b] = h[b] - db
                h[c] = h[c] - dc
                return vidx[h[2], h[1], h[0]]

            q0, q1, q2, q3 = cell(1, 1), cell(0, 1), cell(0, 0), cell(1, 0)
            ok = (q0 >= 0) & (q1 >= 0) & (q2 >= 0) & (q3 >= 0)
            q0, q1, q2, q3 = q0[ok], q1[ok], q2[ok], q3[ok]
            g = [k[ok] for k in g]
            neg0 = N[g[2], g[1], g[0]]
            t_pos = np.stack([q0, q1, q2, q0, q2, q3], 1)
            t_neg = np.stack([q0, q2, q1, q0, q3, q2], 1)
            tris.append(np.where(neg0[:, None], t_pos, t_neg))
            keys.append(self._key(g[2], g[1], g[0]) * 3 + a)
        key = np.concatenate(keys)
        order = np.argsort(key, kind="stable")
        tri = np.concatenate(tris)[order].reshape(-1, 3).astype(np.int32)
        return verts.astype(np.float32), cols.astype(np.float32), tri


# ---- mesh checks -----------------------------------------------------------------------------------------------------
def mesh_report(vertices, triangles):
    """-> dict: closed (every undirected edge in exactly two triangles), oriented (every directed edge once),
    euler (V - E + F over the vertices the triangles use), volume (signed, positive for outward normals)."""
    t = np.asarray(triangles, np.int64)
    v = np.asarray(vertices, np.float64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    nv = int(t.max()) + 1 if len(t) else 0
    directed = e[:, 0] * nv + e[:, 1]
    _, dcount = np.unique(directed, return_counts=True)
    lo, hi = e.min(1), e.max(1)
    _, ucount = np.unique(lo * nv + hi, return_counts=True)
    used = len(np.unique(t))
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    vol = float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
    return {"closed": bool(len(t) and (ucount == 2).all()), "oriented": bool((dcount == 1).all()),
            "euler": used - len(ucount) + len(t), "volume": vol, "used_vertices": used}


# ---- scenes ----------------------------------------------------------------------------------------------------------
def look_at(campos, target=(0.0, 0.0, 0.0)):
    """world->camera [4,4] fp32 of a camera at `campos` looking at `target` (x right, y down, z forward)."""
    campos = np.asarray(campos, np.float64)
    fwd = np.asarray(target, np.float64) - campos
    fwd /= np.linalg.norm(fwd)
    up = np.array([0.0, 0.0, 1.0]) if abs(fwd[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])
    V = np.eye(4)
    V[:3, :3] = R
    V[:3, 3] = -R @ campos
    return V.astype(np.float32)


def _rays(H, W, fx, fy, cx, cy, viewmat):
    V = viewmat.astype(np.float64)
    R, t = V[:3, :3], V[:3, 3]
    o = -R.T @ t
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    dc = np.stack([(jj + 0.5 - cx) / fx, (ii + 0.5 - cy) / fy, np.ones((H, W))], -1)
    return o, dc @ R  # world directions with unit camera-z component: the ray parameter is the z-depth


SPHERE_RADIUS = 0.5
SPHERE_L = 1.0 / 64
SPHERE_SIZE = 160
SPHERE_GRAZING = 0.35


def sphere_cameras(distance=1.5):
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    dirs += [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    out = []
    for d in dirs:
        d = np.asarray(d, np.float64)
        out.append(look_at(distance * d / np.linalg.norm(d)))
    return out


def sphere_intrinsics(size=SPHERE_SIZE, fov_deg=50.0):
    f = 0.5 * size / math.tan(math.radians(fov_deg) / 2)
    # (principal point off the pixel lattice: with cx = size/2 the voxel centres on the symmetry planes of the eight
    #  corner cameras project exactly onto pixel borders, 4.7 % of all updates -- measured on the oracle)
    return float(np.float32(f)), float(np.float32(f)), size / 2.0 + 0.37, size / 2.0 - 0.21


def sphere_view(viewmat, size=SPHERE_SIZE, radius=SPHERE_RADIUS, grazing=SPHERE_GRAZING):
    """-> depth [H,W] f32 (0 = background), color [H,W,3] f32, valid [H,W] u8"""
    fx, fy, cx, cy = sphere_intrinsics(size)
    o, D = _rays(size, size, fx, fy, cx, cy, viewmat)
    a = (D * D).sum(-1)
    b = 2 * (D @ o)
    c = o @ o - radius * radius
    disc = b * b - 4 * a * c
    hit = disc > 0
    t = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0))) / (2 * a), 0.0)
    p = o + t[..., None] * D
    n = p / radius
    cosv = -(n * D).sum(-1) / np.sqrt(a)
    valid = hit & (cosv >= grazing)
    color = np.where(hit[..., None], 0.5 + 0.5 * n, 0.0)
    return t.astype(np.float32), color.astype(np.float32), valid.astype(np.uint8)


def sphere_volume_args(capacity=1000):
    L = SPHERE_L
    return dict(voxel_length=L, sdf_trunc=4 * L, origin=(-0.625, -0.625, -0.625), blocks=(10, 10, 10),
                capacity=capacity)


ROOM_HALF = (1.0, 0.75, 1.25)
ROOM_L = 1.0 / 32
ROOM_W, ROOM_H = 320, 240
ROOM_DEPTH_TRUNC = 1.6


def room_cameras():
    out = []
    for k in range(8):
        yaw = k * math.pi / 4 + 0.1
        pos = np.array([0.2 * math.cos(1.7 * k), 0.1 * math.sin(2.3 * k), 0.25 * math.sin(0.9 * k)])
        tgt = pos + np.array([math.cos(yaw), 0.35 * math.sin(1.3 * k), math.sin(yaw)])
        out.append(look_at(pos, tgt))
    return out


def room_intrinsics():
    f = float(np.float32(0.5 * ROOM_W / math.tan(math.radians(80.0) / 2)))
    return f, f, ROOM_W / 2.0, ROOM_H / 2.0


def room_view(viewmat):
    """Inward-facing planes of the box |x| <= 1, |y| <= 0.75, |z| <= 1.25 seen from inside.  No valid mask."""
    fx, fy, cx, cy = room_intrinsics()
    o, D = _rays(ROOM_H, ROOM_W, fx, fy, cx, cy, viewmat)
    half = np.asarray(ROOM_HALF)
    with np.errstate(divide="ignore"):
        tt = np.where(D > 0, (half - o) / D, np.where(D < 0, (-half - o) / D, np.inf))
    t = tt.min(-1)
    p = o + t[..., None] * D
    color = 0.5 + 0.5 * np.sin(3.0 * p + np.array([0.0, 1.0, 2.0]))
    return t.astype(np.float32), color.astype(np.float32)


def room_volume_args(capacity=960):
    L = ROOM_L
    return dict(voxel_length=L, sdf_trunc=4 * L, origin=(-1.25, -1.0, -1.5), blocks=(10, 8, 12), capacity=capacity)


def fuse_sphere(vol, n_views=None):
    """Integrate the sphere scene into `vol` (a RefVolume or a gs_fusion.TSDFVolume wrapper with the same
    `integrate` signature taking numpy arrays).  -> list of the per-view returns."""
    fx, fy, cx, cy = sphere_intrinsics()
    out = []
    for V in sphere_cameras()[:n_views]:
        d, c, m = sphere_view(V)
        out.append(vol.integrate(d, c, fx, fy, cx, cy, V, valid=m, depth_trunc=10.0))
    return out


def fuse_room(vol):
    fx, fy, cx, cy = room_intrinsics()
    out = []
    for V in room_cameras():
        d, c = room_view(V)
        out.append(vol.integrate(d, c, fx, fy, cx, cy, V, valid=None, depth_trunc=ROOM_DEPTH_TRUNC))
    return out


def dense_view_sdf(volume_args, depth, color, fx, fy, cx, cy, viewmat, valid=None, depth_trunc=10.0):
    """sdf of one view over EVERY voxel of the volume (not only the touched blocks): [num_blocks, 512], NaN where the
    voxel sees no usable pixel.  What step 1 has to cover: every voxel with |sdf| < sdf_trunc."""
    vol = RefVolume(**{**volume_args, "capacity": int(np.prod(volume_args["blocks"]))})
    every = np.arange(int(np.prod(vol.blocks)))
    vol.flagged_blocks = lambda *a, **k: every
    return vol.integrate(depth, color, fx, fy, cx, cy, viewmat, valid=valid, depth_trunc=depth_trunc)["sdf"]


# ---- noise scene: per-pixel random depth over a volume of more than 2048 blocks ---------------------------------------
# Nothing here is a surface: every pixel is a depth point of its own, so nearly every block of the volume is opened by
# nearly every view (lists longer than the 2048 workgroups of the looping kernels), and the fused values have no
# smoothness for an error to hide in -- a voxel that takes the wrong pixel takes an unrelated depth and colour.
NOISE_L = 1.0 / 64
NOISE_W, NOISE_H = 317, 203
NOISE_DEPTH_TRUNC = 3.0
NOISE_BLOCKS = (16, 12, 16)
NOISE_ORIGIN = (-1.0, -0.75, -1.0)
NOISE_OVERFLOW_CAPACITY = 2500


def noise_volume_args(capacity=3072):
    L = NOISE_L
    return dict(voxel_length=L, sdf_trunc=4 * L, origin=NOISE_ORIGIN, blocks=NOISE_BLOCKS, capacity=capacity)


def noise_intrinsics():
    fx = float(np.float32(0.5 * NOISE_W / math.tan(math.radians(100.0) / 2)))
    return fx, float(np.float32(1.07 * fx)), NOISE_W / 2.0 + 0.37, NOISE_H / 2.0 - 0.21


def noise_cameras():
    """One camera inside the volume, three near its corners, one outside it (its frustum clips the volume)."""
    return [look_at((-0.93, -0.68, -0.9), (0.35, 0.2, 0.3)),
            look_at((0.92, 0.66, -0.88), (-0.3, -0.25, 0.35)),
            look_at((0.1, -0.05, 0.2), (0.6, 0.3, -0.5)),
            look_at((-0.9, 0.68, 0.93), (0.3, -0.2, -0.35)),
            look_at((1.6, -1.2, 1.45), (0.1, 0.0, 0.05))]


def noise_view(k, poison=False):
    """-> depth [H,W] f32 uniform in [0.15, 3.2] with 5 % zeros, color [H,W,3] f32 uniform, valid [H,W] u8 (90 % set).
    `poison`: a fixed 1 % of the pixels hold NaN, +inf, -1 and 1.5 * depth_trunc in turn; their `valid` stays 1."""
    rng = np.random.default_rng(4100 + k)
    depth = rng.uniform(0.15, 3.2, (NOISE_H, NOISE_W)).astype(np.float32)
    depth[rng.random((NOISE_H, NOISE_W)) < 0.05] = 0.0
    color = rng.random((NOISE_H, NOISE_W, 3)).astype(np.float32)
    valid = (rng.random((NOISE_H, NOISE_W)) < 0.9).astype(np.uint8)
    bad = rng.permutation(NOISE_H * NOISE_W)[:NOISE_H * NOISE_W // 100]
    if poison:
        values = np.array([np.nan, np.inf, -1.0, NOISE_DEPTH_TRUNC * 1.5], np.float32)
        depth.reshape(-1)[bad] = values[np.arange(len(bad)) % 4]
    valid.reshape(-1)[bad] = 1
    return depth, color, valid


def sphere_views(n_views=None):
    """The scenes as lists of views: dicts of the keyword arguments of `integrate`."""
    fx, fy, cx, cy = sphere_intrinsics()
    out = []
    for V in sphere_cameras()[:n_views]:
        d, c, m = sphere_view(V)
        out.append(dict(depth=d, color=c, fx=fx, fy=fy, cx=cx, cy=cy, viewmat=V, valid=m, depth_trunc=10.0))
    return out


def room_views():
    fx, fy, cx, cy = room_intrinsics()
    out = []
    for V in room_cameras():
        d, c = room_view(V)
        out.append(dict(depth=d, color=c, fx=fx, fy=fy, cx=cx, cy=cy, viewmat=V, valid=None,
                        depth_trunc=ROOM_DEPTH_TRUNC))
    return out


def noise_views(poison=False, masked=False):
    fx, fy, cx, cy = noise_intrinsics()
    out = []
    for k, V in enumerate(noise_cameras()):
        d, c, m = noise_view(k, poison)
        out.append(dict(depth=d, color=c, fx=fx, fy=fy, cx=cx, cy=cy, viewmat=V, valid=m if masked else None,
                        depth_trunc=NOISE_DEPTH_TRUNC))
    return out


def fuse_views(vol, views):
    """Integrate `views` (dicts as above) into a RefVolume, or a wrapper with the same `integrate`, in order."""
    return [vol.integrate(v["depth"], v["color"], v["fx"], v["fy"], v["cx"], v["cy"], v["viewmat"], valid=v["valid"],
                          depth_trunc=v["depth_trunc"]) for v in views]


def blocked(a, blocks):
    """dense [Bz*8, By*8, Bx*8(, C)] -> [num_blocks, 512(, C)] in the pool's block and voxel order."""
    Bx, By, Bz = blocks
    tail = a.shape[3:]
    a = a.reshape((Bz, 8, By, 8, Bx, 8) + tail)
    a = a.transpose((0, 2, 4, 1, 3, 5) + tuple(range(6, 6 + len(tail))))
    return np.ascontiguousarray(a).reshape((Bx * By * Bz, 512) + tail)


def dense_fusion_f64(volume_args, views, lists=None):
    """The fusion rule in plain float64 over EVERY voxel of the volume: no blocks, no touch step, no slot table.

    The parameters are the float32 numbers the kernels receive (voxel length, truncation, origin, intrinsics, the
    world->camera matrix), widened; every operation on them is float64.  -> dict of tsdf [num_blocks,512], weight,
    color [num_blocks,512,3] and
      unstable [num_blocks,512]: true where, in any view, a float32 evaluation may decide otherwise than this one -- a
        projected coordinate within AMBIG_PIXEL of an integer (voxels in front of the camera), the fetched depth within
        AMBIG_VALUE of depth_trunc, or the sdf within AMBIG_VALUE of -sdf_trunc;
      band [num_blocks,512] int64: bit k set where view k updates the voxel with sdf < sdf_trunc -- what the touch step
        of view k has to cover (an update with sdf >= sdf_trunc is free space: it stores 1, and only blocks that a
        depth point opened receive it).

    A block-sparse volume applies a view to the blocks that view opened, this function to every voxel: the two agree
    where every block is opened by every view that sees it (the noise scene).  For a scene of surfaces, `lists[k]`
    (linear block indices) confines view k to those blocks; `band` does not depend on it, and says whether the lists
    hold what they must."""
    w32 = lambda x: float(np.float32(x))  # noqa: E731
    L, trunc = w32(volume_args["voxel_length"]), w32(volume_args["sdf_trunc"])
    origin = np.asarray(volume_args["origin"], np.float32).astype(np.float64)
    Bx, By, Bz = (int(b) for b in volume_args["blocks"])
    X = origin[0] + (np.arange(Bx * 8) + 0.5) * L
    Y = origin[1] + (np.arange(By * 8) + 0.5) * L
    Z = origin[2] + (np.arange(Bz * 8) + 0.5) * L
    pz, py, px = np.meshgrid(Z, Y, X, indexing="ij")
    shape = px.shape
    tsdf = np.zeros(shape)
    weight = np.zeros(shape)
    color = np.zeros(shape + (3,))
    unstable = np.zeros(shape, bool)
    band = np.zeros(shape, np.int64)
    for k, view in enumerate(views):
        depth = np.asarray(view["depth"], np.float32).astype(np.float64)
        image = np.asarray(view["color"], np.float32).astype(np.float64)
        H, W = depth.shape
        fx, fy, cx, cy = (w32(view[k]) for k in ("fx", "fy", "cx", "cy"))
        dt = w32(view["depth_trunc"])
        M = np.asarray(view["viewmat"], np.float32).astype(np.float64)
        xc = M[0, 0] * px + M[0, 1] * py + M[0, 2] * pz + M[0, 3]
        yc = M[1, 0] * px + M[1, 1] * py + M[1, 2] * pz + M[1, 3]
        zc = M[2, 0] * px + M[2, 1] * py + M[2, 2] * pz + M[2, 3]
        front = zc > 0
        zs = np.where(front, zc, 1.0)
        u = fx * xc / zs + cx
        v = fy * yc / zs + cy
        unstable |= front & ((np.abs(u - np.rint(u)) < AMBIG_PIXEL) | (np.abs(v - np.rint(v)) < AMBIG_PIXEL))
        ju, iv = np.floor(u), np.floor(v)
        inside = front & (ju >= 0) & (ju < W) & (iv >= 0) & (iv < H)
        j = np.where(inside, ju, 0).astype(np.int64)
        i = np.where(inside, iv, 0).astype(np.int64)
        d = depth[i, j]
        finite = np.isfinite(d)
        dz = np.where(finite, d, 0.0)  # (a NaN or inf pixel is unusable; kept out of the arithmetic below)
        unstable |= inside & finite & (np.abs(dz - dt) < AMBIG_VALUE)
        usable = inside & finite & (dz > 0) & (dz <= dt)
        if view["valid"] is not None:
            usable &= np.asarray(view["valid"])[i, j] != 0
        xn = (j + 0.5 - cx) / fx
        yn = (i + 0.5 - cy) / fy
        sdf = (dz - zc) * np.sqrt(1.0 + xn * xn + yn * yn)
        unstable |= usable & (np.abs(sdf + trunc) < AMBIG_VALUE)
        upd = usable & (sdf > -trunc)
        band |= (upd & (sdf < trunc)).astype(np.int64) << k
        if lists is not None:
            member = np.zeros(Bx * By * Bz, bool)
            member[np.asarray(lists[k], np.int64)] = True
            upd &= member.reshape(Bz, By, Bx).repeat(8, 0).repeat(8, 1).repeat(8, 2)
        f = np.minimum(1.0, sdf / trunc)
        w1 = weight + 1.0
        tsdf = np.where(upd, (tsdf * weight + f) / w1, tsdf)
        color = np.where(upd[..., None], (color * weight[..., None] + image[i, j]) / w1[..., None], color)
        weight = np.where(upd, w1, weight)
    blocks = (Bx, By, Bz)
    return {"tsdf": blocked(tsdf, blocks), "weight": blocked(weight, blocks), "color": blocked(color, blocks),
            "unstable": blocked(unstable, blocks), "band": blocked(band, blocks)}


def pool_by_block(vol_table, pool):
    """pool rows [capacity, 512(,C)] -> [num_blocks, 512(,C)] through the slot table (zeros where there is no slot)."""
    table = np.asarray(vol_table).reshape(-1)
    out = np.zeros((len(table),) + pool.shape[1:], pool.dtype)
    held = table >= 0
    out[held] = pool[table[held]]
    return out


def f64_distance(table, tsdf, weight, color, dense, what=""):
    """A fused float32 volume (table and pool arrays) against `dense` = dense_fusion_f64(...).  -> dict: stable (mask
    [num_blocks,512]), unstable_share, uncovered (stable voxels float64 updated that lie in no allocated block),
    weight_mismatches, d_tsdf / d_color (largest distances), all over stable voxels."""
    t64, w64, c64, unstable = (dense[k] for k in ("tsdf", "weight", "color", "unstable"))
    stable = ~unstable
    t, w, c = (pool_by_block(table, a) for a in (tsdf, weight, color))
    held = (np.asarray(table).reshape(-1) >= 0)[:, None]
    rep = {"stable": stable, "unstable_share": float(unstable.mean()),
           "uncovered": int((stable & (w64 > 0) & ~held).sum()),
           "weight_mismatches": int((w.astype(np.float64) != w64)[stable].sum()),
           "d_tsdf": float(np.abs(t - t64)[stable].max()), "d_color": float(np.abs(c - c64)[stable].max())}
    if what:
        print(f"{what}: {int(stable.sum())} stable voxels ({rep['unstable_share']:.3%} unstable), "
              f"{int((w64 > 0)[stable].sum())} updated in float64, {rep['uncovered']} of them in no allocated block, "
              f"{rep['weight_mismatches']} weights differ, max |tsdf - f64| {rep['d_tsdf']:.3e}, "
              f"max |colour - f64| {rep['d_color']:.3e}")
    return rep


# ---- random volumes for the extraction ---------------------------------------------------------------------------------
RANDOM_SHAPES = [(2100, 1, 1), (1, 1, 2100), (13, 17, 11), (1, 1, 1)]
RANDOM_KINDS = ["smooth", "noise"]
RANDOM_L = 1.0 / 64
SMOOTH_WAVES, SMOOTH_WAVELENGTHS = 3, (16.0, 40.0)
PLANTED = (np.float32(0.0), np.float32(-0.0), QUALIFY, -QUALIFY, np.nextafter(QUALIFY, F(0)))


def random_fill(blocks):
    """Share of allocated blocks per shape: the oracle stays within a few seconds on each."""
    return 1.0 if int(np.prod(blocks)) == 1 else 0.8


def random_volume_state(blocks, capacity=None, fill=0.8, seed=0, kind="noise", plant=0.002):
    """A `state_dict` that no fusion produced.  A random `fill` share of the blocks holds a slot, the slot numbers are a
    random permutation (slot order unrelated to block order), `capacity` None leaves three spare slots.  tsdf:
    "smooth" = 0.6 times a sum of three random sinusoids over the voxel position (wavelengths of 16 to 40 voxels),
    clipped to [-1, 1]; "noise" = clip(0.6 N(0,1), -1, 1) per voxel.  Then weight = 0 on a random 10 % of the voxels
    (weights are 1..6 elsewhere), and each of the values of PLANTED on a random `plant` share of them.

    Surface nets lists a directed edge twice wherever a cell face has the signs of a checkerboard (the four grid edges
    of that face all cross, and each of their quads joins the same two cells), so a mesh is consistently oriented in
    the sense of `mesh_report` only if the field has no such face.  The smooth kind is meant to have none: its
    wavelengths are long, and the planted values that count as positive (0.0, -0.0, just below 0.98) go only where the
    field is not negative, so that no planted voxel flips a sign next to the surface (the noise kind plants them
    everywhere).  Whether a given seed gives such a field is pinned on the oracle (test_tsdf_host.py)."""
    rng = np.random.default_rng(seed)
    Bx, By, Bz = (int(b) for b in blocks)
    nb = Bx * By * Bz
    n = max(1, min(nb, int(round(fill * nb))))
    capacity = n + 3 if capacity is None else int(capacity)
    assert capacity >= n
    held = np.sort(rng.permutation(nb)[:n])
    table = np.full(nb, -1, np.int32)
    table[held] = rng.permutation(n).astype(np.int32)
    L = np.float32(RANDOM_L)
    origin = np.array([-0.3, 0.2, 0.1], np.float32)
    v = np.arange(512)
    g = np.stack([(held % Bx)[:, None] * 8 + (v & 7)[None], ((held // Bx) % By)[:, None] * 8 + ((v >> 3) & 7)[None],
                  (held // (Bx * By))[:, None] * 8 + (v >> 6)[None]], -1).astype(np.float64)  # [n,512,3]
    if kind == "smooth":
        f = np.zeros((n, 512))
        for _ in range(SMOOTH_WAVES):
            k = rng.standard_normal(3)
            k *= 2 * math.pi / (rng.uniform(*SMOOTH_WAVELENGTHS) * np.linalg.norm(k))
            f += np.sin(g @ k + rng.uniform(0, 2 * math.pi))
        f = np.clip(0.6 * f, -1.0, 1.0)
    elif kind == "noise":
        f = np.clip(0.6 * rng.standard_normal((n, 512)), -1.0, 1.0)
    else:
        raise ValueError(kind)
    f = f.astype(np.float32)
    w = rng.integers(1, 7, (n, 512)).astype(np.float32)
    w[rng.random((n, 512)) < 0.1] = 0.0
    where = rng.random((n, 512))
    for k, value in enumerate(PLANTED):
        here = (where >= k * plant) & (where < (k + 1) * plant)
        if kind == "smooth" and abs(value) < QUALIFY:
            here &= f >= 0
        f[here] = value
    col = rng.random((n, 512, 3)).astype(np.float32)
    tsdf = np.zeros((capacity, 512), np.float32)
    weight = np.zeros((capacity, 512), np.float32)
    color = np.zeros((capacity, 512, 3), np.float32)
    tsdf[table[held]], weight[table[held]], color[table[held]] = f, w, col
    return {"voxel_length": float(L), "sdf_trunc": float(4 * L), "origin": origin, "blocks": (Bx, By, Bz),
            "capacity": capacity, "table": table.reshape(Bz, By, Bx), "tsdf": tsdf, "weight": weight, "color": color,
            "num_allocated": n, "overflow": False, "needed": n}


def ref_from_state(sd):
    """A RefVolume holding the state `sd` (its arrays are copied)."""
    vol = RefVolume(sd["voxel_length"], sd["sdf_trunc"], sd["origin"], sd["blocks"], sd["capacity"])
    vol.table = np.array(sd["table"], np.int32)
    vol.tsdf, vol.weight, vol.color = (np.array(sd[k], np.float32) for k in ("tsdf", "weight", "color"))
    vol.num_allocated, vol.overflow, vol.needed = int(sd["num_allocated"]), bool(sd["overflow"]), int(sd["needed"])
    return vol


def band_uncovered(dense, lists):
    """Per view: stable voxels that the view updates with sdf < sdf_trunc (float64) in a block missing from the
    view's list."""
    out = []
    for k, blocks in enumerate(lists):
        need = ((dense["band"] >> k) & 1).astype(bool) & ~dense["unstable"]
        need[np.asarray(blocks, np.int64)] = False
        out.append(int(need.sum()))
    return out


# ---- cases shared by the CPU and the GPU tests --------------------------------------------------------------------------
def f64_case(scene):
    """-> volume args, views, and `lists(infos)`: what dense_fusion_f64 takes as `lists` for this scene -- None on the
    noise scene (the plain rule), the oracle's per-view blocks on the scenes of surfaces."""
    if scene == "noise":
        return noise_volume_args(), noise_views(), lambda infos: None
    args, views = (sphere_volume_args(), sphere_views()) if scene == "sphere" else (room_volume_args(), room_views())
    return args, views, lambda infos: [i["blocks"] for i in infos]


@functools.lru_cache(maxsize=None)
def fused_oracle(scene, capacity=None, poison=False, masked=False):
    """-> (RefVolume, infos) of a whole scene, computed once per process; callers leave it unchanged."""
    if scene == "noise":
        args, views = noise_volume_args(), noise_views(poison, masked)
    else:
        args, views, _ = f64_case(scene)
    if capacity is not None:
        args = {**args, "capacity": capacity}
    vol = RefVolume(**args)
    return vol, fuse_views(vol, views)


RANDOM_SEED = 8  # (with it the smooth fields have no ambiguous face: test_oracle_extraction_of_random_volumes)


@functools.lru_cache(maxsize=None)
def random_state(blocks, kind):
    return random_volume_state(blocks, fill=random_fill(blocks), seed=RANDOM_SEED, kind=kind)
