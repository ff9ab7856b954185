"""The geometric odometry restated in numpy, written from the contract (include/dpm_hip.h: dpm_local_map_*):
a dict-of-voxels map with the owner-word rule, the search with its geometric tie-break, the weighted Gauss-Newton step and
the odometry loop around them.  The reference has no such module, so this restatement is the yardstick of
tests/test_gpu_local_map.py and tests/test_gpu_lidar_odometry.py.

`dtype` float32 mirrors the kernels' operation order (transform by the rounded map-frame pose, fp32 division, floor,
sub-cell, distances); float64 is the independent form: nothing is rounded to fp32 on the way.  The solve and the pose are
float64 in both, as on the GPU; the Gauss-Newton part is icp_restated's: it is the same csrc/gn_solve.h.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restated as I  # noqa: E402

CONVERGED, MAX_ITER, NO_MATCH, SINGULAR = I.CONVERGED, I.MAX_ITER, I.NO_MATCH, I.SINGULAR
BIAS = 1 << 20
M21 = (1 << 21) - 1
M64 = (1 << 64) - 1


def mix64(k):
    """splitmix64 finaliser on Python ints: the slot a key starts probing from is mix64(key) & (cap_vox - 1)"""
    k ^= k >> 30
    k = (k * 0xbf58476d1ce4e5b9) & M64
    k ^= k >> 27
    k = (k * 0x94d049bb133111eb) & M64
    return k ^ (k >> 31)


def pack_key(v):
    """voxel coordinates (..., 3) int64 -> keys (uint64 bits in int64; the top bit is never set)"""
    v = np.asarray(v, np.int64) + BIAS
    return v[..., 0] | (v[..., 1] << 21) | (v[..., 2] << 42)


def unpack_key(key):
    key = np.asarray(key, np.int64)
    return np.stack([key & M21, (key >> 21) & M21, (key >> 42) & M21], axis=-1) - BIAS


def map_pose(pose, origin):
    """the pose in the map frame, float64: the translation minus the origin (rounded to dtype by I.transform, once)"""
    P = np.array(pose, np.float64)
    P[:3, 3] -= np.asarray(origin, np.float64)
    return P


def cells(q, voxel, s, dtype):
    """q (n,3) dtype -> voxel coordinates (n,3) int64, sub-cell number (n,), inside (n,) bool"""
    v = dtype(voxel) if dtype == np.float32 else np.float64(voxel)
    with np.errstate(invalid="ignore", over="ignore"):
        f = (q.astype(dtype) / v).astype(dtype)
        fl = np.floor(f)
        inside = np.all((fl >= -BIAS) & (fl < BIAS), axis=1)
        fl_ok = np.where(inside[:, None], fl, 0)
        frac = np.where(inside[:, None], f - fl, 0).astype(dtype)
        sc = np.minimum((frac * dtype(s)).astype(dtype).astype(np.int64), s - 1)
    return fl_ok.astype(np.int64), (sc[:, 2] * s + sc[:, 1]) * s + sc[:, 0], inside


class Map:
    """{key: {sub-cell: (owner word, xyz)}} with the rule: the smallest owner word ever offered keeps the sub-cell"""

    def __init__(self, voxel=1.0, subdiv=3, origin=(0, 0, 0), min_range=0.0, max_range=100.0, dtype=np.float32):
        self.voxel = float(np.float32(voxel)) if dtype == np.float32 else float(voxel)
        self.s, self.origin, self.dtype = int(subdiv), np.asarray(origin, np.float64), dtype
        self.min_range, self.max_range = float(min_range), float(max_range)
        self.vox = {}
        self.outside = 0

    def gate(self, xyz):
        p = xyz.astype(self.dtype)
        with np.errstate(invalid="ignore", over="ignore"):
            r2 = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
            lo, hi = self.min_range * self.min_range, self.max_range * self.max_range
            if self.dtype == np.float32:
                lo, hi = np.float32(lo), np.float32(hi)
            return (r2 >= lo) & (r2 <= hi)

    def insert(self, xyz, idx, pose, stamp):
        """xyz (n,3) float32 valid rows, idx (n,) the rows' numbers, pose (4,4) float64"""
        xyz = np.asarray(xyz, np.float32)
        keep = self.gate(xyz)
        q = I.transform(map_pose(pose, self.origin), xyz, self.dtype)
        vox, sub, inside = cells(q, self.voxel, self.s, self.dtype)
        self.outside += int((keep & ~inside).sum())
        key = pack_key(vox)
        for i in np.nonzero(keep & inside)[0]:
            word = (int(stamp) << 32) | int(idx[i])
            cell = self.vox.setdefault(int(key[i]), {})
            if int(sub[i]) not in cell or word < cell[int(sub[i])][0]:
                cell[int(sub[i])] = (word, q[i].copy())

    def prune(self, pose, radius):
        dt = self.dtype
        t = map_pose(pose, self.origin)[:3, 3].astype(dt)
        r2 = dt(radius * radius)
        keep = {}
        for key, cell in self.vox.items():
            c = ((unpack_key(key).astype(dt) + dt(0.5)) * dt(self.voxel)).astype(dt)
            d = (c - t).astype(dt)
            if (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= r2:
                keep[key] = cell
        self.vox = keep

    def export(self):
        """sorted by (key, sub-cell): keys (n,) int64, sub (n,) int32, owner (n,) int64, xyz (n,3) dtype"""
        rows = sorted((key, sub, w, p) for key, cell in self.vox.items() for sub, (w, p) in cell.items())
        if not rows:
            return np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros((0, 3), self.dtype)
        return (np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], np.int32),
                np.array([r[2] for r in rows], np.int64), np.stack([r[3] for r in rows]).astype(self.dtype))

    def points_world(self):
        return self.export()[3].astype(np.float64) + self.origin


# ------------------------------------------------------------------------------------------------------------------- search
def _d2(q, p, dtype):
    d = q.astype(dtype) - p.astype(dtype)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _tie(qv, pv, sub):
    """neighbour number * 32 + sub-cell from the voxel offset point - query; offsets outside -1..1 sort last"""
    dv = pv - qv
    near = np.all(np.abs(dv) <= 1, axis=-1)
    n = ((dv[..., 2] + 1) * 3 + (dv[..., 1] + 1)) * 3 + (dv[..., 0] + 1)
    return np.where(near, n * 32 + sub, 1 << 40), near


def _pick(d2, tie, r2):
    """per row the column with the smallest (d2, tie); -1 when that d2 > r2 or the row is empty"""
    if d2.shape[1] == 0:
        return np.full(d2.shape[0], -1, np.int64)
    with np.errstate(invalid="ignore"):
        d2 = np.where(np.isnan(d2), np.inf, d2)
        best = d2.min(axis=1, keepdims=True)
        t = np.where(d2 == best, tie, 1 << 41)
        j = np.argmin(t, axis=1)
        ok = best[:, 0] <= r2
    return np.where(ok, j, -1)


def search_exhaustive(q, exported, voxel, s, max_dist, dtype, chunk=256):
    """q (n,3) map-frame queries against EVERY exported point: winner row of the export or -1, and whether the winner lay
    inside the 27 voxels around the query (it always does when max_dist <= voxel, in exact arithmetic)"""
    keys, sub, _, xyz = exported
    qv, _, inside = cells(q, voxel, s, dtype)
    pv = unpack_key(keys)
    r2 = np.float32(max_dist * max_dist).astype(dtype)
    win = np.full(len(q), -1, np.int64)
    near = np.ones(len(q), bool)
    for a in range(0, len(q), chunk):
        b = slice(a, a + chunk)
        tie, nr = _tie(qv[b, None, :], pv[None, :, :], sub[None, :].astype(np.int64))
        w = _pick(_d2(q[b, None, :], xyz[None, :, :], dtype), tie, r2)
        w = np.where(inside[b], w, -1)
        win[b] = w
        near[b] = np.where(w >= 0, nr[np.arange(len(w)), np.maximum(w, 0)], True) if len(keys) else True
    return win, near


def search27(q, exported, voxel, s, max_dist, dtype):
    """the kernel's search: only the 3 x 3 x 3 voxels around the query's own, looked up by key"""
    keys, sub, _, xyz = exported
    n, S = len(q), s ** 3
    win = np.full(n, -1, np.int64)
    if len(keys) == 0 or n == 0:
        return win
    qv, _, inside = cells(q, voxel, s, dtype)
    ukeys, start = np.unique(keys, return_index=True)   # the export is sorted by (key, sub)
    slot = np.full((len(ukeys), S), -1, np.int64)       # row of the export per (voxel, sub-cell)
    slot[np.searchsorted(ukeys, keys), sub] = np.arange(len(keys))
    r2 = np.float32(max_dist * max_dist).astype(dtype)
    best_d = np.full(n, np.inf, dtype)
    best_t = np.full(n, 1 << 41, np.int64)
    for nb in range(27):
        off = np.array([nb % 3 - 1, (nb // 3) % 3 - 1, nb // 9 - 1])
        v = qv + off
        ok = inside & np.all((v >= -BIAS) & (v < BIAS), axis=1)
        k = pack_key(np.where(ok[:, None], v, 0))
        pos = np.minimum(np.searchsorted(ukeys, k), len(ukeys) - 1)
        ok &= ukeys[pos] == k
        rows = np.where(ok[:, None], slot[pos], -1)     # (n,S)
        with np.errstate(invalid="ignore"):
            d = np.where(rows >= 0, _d2(q[:, None, :], xyz[np.maximum(rows, 0)], dtype), np.inf)
            d = np.where(np.isnan(d), np.inf, d)
        t = nb * 32 + np.arange(S)[None, :]
        j = np.argmin(d, axis=1)                         # first minimum = smaller sub-cell
        dj, tj, rj = d[np.arange(n), j], t[0, j], rows[np.arange(n), j]
        better = (dj < best_d) | ((dj == best_d) & (tj < best_t) & (rj >= 0))
        best_d, best_t = np.where(better, dj, best_d), np.where(better, tj, best_t)
        win = np.where(better & (rj >= 0), rj, win)
    return np.where(best_d <= r2, win, -1)


def search_fast(q, exported, voxel, s, max_dist, dtype, tree=None, k=8):
    """the same answer over the k candidates a cKDTree finds nearest in float64 (another point wins in dtype only if k + 1
    lie within rounding of the best): what the odometry loop below uses"""
    from scipy.spatial import cKDTree
    keys, sub, _, xyz = exported
    if len(keys) == 0 or len(q) == 0:
        return np.full(len(q), -1, np.int64)
    k = min(k, len(keys))
    tree = tree or cKDTree(xyz.astype(np.float64))
    qq = np.where(np.isfinite(q), q, 1e30).astype(np.float64)
    _, cand = tree.query(qq, k=k)
    cand = cand.reshape(len(q), k)
    qv, _, inside = cells(q, voxel, s, dtype)
    tie, near = _tie(qv[:, None, :], unpack_key(keys)[cand], sub[cand].astype(np.int64))
    d = np.where(near, _d2(q[:, None, :], xyz[cand], dtype), np.inf)
    j = _pick(d, tie, np.float32(max_dist * max_dist).astype(dtype))
    return np.where((j >= 0) & inside, cand[np.arange(len(q)), np.maximum(j, 0)], -1)


# --------------------------------------------------------------------------------------------------------------- Gauss-Newton
def system(q, win, xyz, kernel_scale, dtype):
    """the 29 sums of the point rows on given matches, weighted by the match's e.e; also J, e, w for the bounds"""
    m = int((win >= 0).sum())
    J, e = I.rows(q, win, xyz, None, I.POINT, dtype)
    e3 = e.reshape(3, m).T
    w3 = np.tile(I.weights((e3[:, 0] * e3[:, 0] + e3[:, 1] * e3[:, 1]) + e3[:, 2] * e3[:, 2], kernel_scale, dtype), 3)
    return I.system(J, e, m, dtype, w3), J, e, w3


def system_floor(J, e, w3, kernel_scale, delta):
    """icp_restated.system_floor with the weights of point rows: with E = e.e of the match, |dE| <= sum_a 2 |e_a| 2 delta and
    dw = 2 sqrt(w) k / (k + E)^2 dE <= 2 w / (k + E) dE."""
    ae, w3 = np.abs(e).astype(np.float64), w3.astype(np.float64)
    m = len(e) // 3
    dw = np.zeros(len(e))
    if kernel_scale > 0:
        k = kernel_scale * kernel_scale
        E = (ae.reshape(3, m) ** 2).sum(axis=0)
        dE = (2 * ae.reshape(3, m) * 2 * delta).sum(axis=0)
        dw = np.tile(2 * w3[:m] / (k + E) * dE, 3)
    return I.system_floor(J, e, delta, w3, dw)


def register(src, exported, voxel, s, origin, init, schedule, kernel_scale=0.0, tol_rot=1e-7, tol_trans=1e-6,
             dtype=np.float64, search=search_fast):
    """-> dict(pose, fitness, rmse, iterations, status) of the valid rows src (n,3) float32 against an exported map; the step
    acts in the map frame, where the rows were formed"""
    from scipy.spatial import cKDTree
    xyz = exported[3]
    extra = dict(tree=cKDTree(xyz.astype(np.float64))) if search is search_fast and len(xyz) else {}

    def system_of(pose, max_dist):
        q = I.transform(pose, src, dtype)
        return system(q, search(q, exported, voxel, s, max_dist, dtype, **extra), xyz, kernel_scale, dtype)[0]
    return I.iterate(system_of, len(src), init, schedule, tol_rot, tol_trans, origin)


# ------------------------------------------------------------------------------------------------------------------- odometry
def odometry(frames, voxel=1.0, subdiv=3, max_range=100.0, min_range=0.0, schedule=((1.0, 30),), kernel_scale=0.0,
             first_pose=None, dtype=np.float64, tol_rot=1e-7, tol_trans=1e-6, initial_motion=None):
    """frames: [(n_k,3) float32] neither thinned nor deskewed -> (poses (F,4,4) float64, statuses).  Constant-velocity
    prediction, registration against the map, insert under the refined pose (rows numbered 0..n_k-1, stamp = frame number),
    prune to max_range; a frame whose registration fails keeps its prediction and is not inserted."""
    poses, statuses = [], []
    m = None
    for k, xyz in enumerate(frames):
        xyz = np.asarray(xyz, np.float32)
        if k == 0:
            P = np.eye(4) if first_pose is None else np.array(first_pose, np.float64)
            m = Map(voxel, subdiv, P[:3, 3].copy(), min_range, max_range, dtype)
            status = CONVERGED
        else:
            motion = np.linalg.inv(poses[-2]) @ poses[-1] if k >= 2 else (np.eye(4) if initial_motion is None else initial_motion)
            pred = poses[-1] @ motion
            r = register(xyz, m.export(), m.voxel, m.s, m.origin, pred, schedule, kernel_scale, tol_rot, tol_trans, dtype)
            status = r["status"]
            P = r["pose"] if status in (CONVERGED, MAX_ITER) else pred
        if status in (CONVERGED, MAX_ITER):
            m.insert(xyz, np.arange(len(xyz)), P, k)
            m.prune(P, max_range)
        poses.append(P)
        statuses.append(status)
    return np.stack(poses), statuses, m


# --------------------------------------------------------------------------------------------------------------------- scenes
def three_planes(n_side=18, spacing=1.0, wall=-9.0):
    """3 n_side^2 lattice points on the planes x = wall, y = wall, z = wall (a room's corner seen from inside), float64"""
    a = (np.arange(n_side) - (n_side - 1) / 2) * spacing
    u, v = [g.ravel() for g in np.meshgrid(a, a, indexing="ij")]
    z = np.full_like(u, wall)
    return np.concatenate([np.stack([z, u, v], 1), np.stack([u, z, v], 1), np.stack([u, v, z], 1)])
