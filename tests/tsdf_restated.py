"""The TSDF surface map restated in numpy, written from the contract (include/dpm_hip.h: dpm_tsdf_*).  The
reference has no such module, so this restatement is the yardstick of tests/test_gpu_tsdf.py.

Two forms:
  Fused      float32, operation for operation what csrc/tsdf_map.hip does: the range gate, the fma chain of the transform
             (icp_restated.transform), u = (q - o) / r, the samples t = r + (float)k * h, the voxel of o + u * t, the skip of a
             repeated key, s clamped, rintf(s * 2^24) into an integer sum.  `surface` and `mesh` read its export.
             skip / clamp / rint = False give the three MUTANTS tests/test_tsdf_host.py needs: they must differ from the true
             form on the inputs the GPU tests use, or those inputs could not tell a kernel that forgot the step.
  fused64    float64 in WORLD coordinates, independent: no map-frame pose, no fixed point, the sum a float64 mean.  It also
             says which voxels are AMBIGUOUS: touched by a sample whose float64 position lies within 1e-5 m of a voxel face,
             or whose t lies within 1e-5 m of 0 -- either voxel such a sample might fall into.  They may be left out of a
             comparison between the two forms, at most 1 % of a test's voxels (the simulator's cap).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restated as I  # noqa: E402
import lidar_odometry_restated as L  # noqa: E402

FIX_ONE = 16777216.0
AMBIGUOUS = 1e-5
F32 = np.float32


def steps(tau, h):
    return int(np.ceil(float(tau) / float(h)))


class Fused:
    """{key: [sum, count]} under the kernel's rule, float32"""

    def __init__(self, voxel, origin=(0, 0, 0), truncation=None, step=None, min_range=0.0, max_range=100.0, skip=True,
                 clamp=True, rint=True):
        self.voxel, self.origin = float(voxel), np.asarray(origin, np.float64)
        self.tau = 3.0 * self.voxel if truncation is None else float(truncation)
        self.h = self.voxel / 2.0 if step is None else float(step)
        self.lo2, self.hi2 = F32(float(min_range) ** 2), F32(float(max_range) ** 2)
        self.skip, self.clamp, self.rint = skip, clamp, rint
        self.sum, self.count, self.outside = {}, {}, 0

    def integrate(self, xyz, pose):
        """xyz (n,3) float32 valid rows, pose (4,4) float64"""
        xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
        if len(xyz) == 0:
            return self
        v, tau, h = F32(self.voxel), F32(self.tau), F32(self.h)
        with np.errstate(all="ignore"):
            x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
            r2 = (x * x + y * y) + z * z
            keep = (r2 >= self.lo2) & (r2 <= self.hi2)
            r = np.sqrt(r2)
            P = L.map_pose(pose, self.origin)
            q = I.transform(P, xyz, F32)
            o = P[:3, 3].astype(F32)
            u = (q - o[None, :]) / r[:, None]
            prev = np.full(len(xyz), -1, np.int64)
            keys, fixed = [], []
            n = steps(self.tau, self.h)
            for k in range(-n, n + 1):
                t = r + F32(k) * h
                live = keep & (t > 0)
                p = o[None, :] + u * t[:, None]
                fl = np.floor(p / v)
                inside = np.all((fl >= -L.BIAS) & (fl < L.BIAS), axis=1)
                self.outside += int((live & ~inside).sum())
                live &= inside
                fl = np.where(live[:, None], fl, 0)
                key = L.pack_key(fl.astype(np.int64))
                new = live & (key != prev) if self.skip else live
                prev = np.where(live, key, prev)
                c = (fl + F32(0.5)) * v
                e = q - c
                s = (u[:, 0] * e[:, 0] + u[:, 1] * e[:, 1]) + u[:, 2] * e[:, 2]
                if self.clamp:
                    s = np.minimum(np.maximum(s, -tau), tau)
                w = s[new] * F32(FIX_ONE)
                keys.append(key[new])
                fixed.append((np.rint(w) if self.rint else np.trunc(w)).astype(np.int64))
        keys, fixed = np.concatenate(keys), np.concatenate(fixed)
        uk, inv = np.unique(keys, return_inverse=True)
        total, number = np.zeros(len(uk), np.int64), np.zeros(len(uk), np.int64)
        np.add.at(total, inv, fixed)
        np.add.at(number, inv, 1)
        for kk, a, b in zip(uk.tolist(), total.tolist(), number.tolist()):
            self.sum[kk] = self.sum.get(kk, 0) + a
            self.count[kk] = self.count.get(kk, 0) + b
        return self

    def integrate_frames(self, store, lengths, frames, poses):
        store = np.asarray(store, F32)
        for row, pose in zip(frames, np.asarray(poses, np.float64).reshape(-1, 4, 4)):
            if not 0 <= int(row) < store.shape[0]:
                continue
            n = min(max(int(lengths[row]), 0), store.shape[2])
            self.integrate(store[row, :, :n].T, pose)
        return self

    def export(self):
        """sorted by key: keys (n,) int64, sums (n,) int64, counts (n,) uint32"""
        keys = np.array(sorted(self.sum), np.int64)
        return (keys, np.array([self.sum[k] for k in keys.tolist()], np.int64),
                np.array([self.count[k] for k in keys.tolist()], np.uint32))


def field(exported, min_count=1, dtype=F32):
    """-> (keys, D) of the qualified voxels; D = (float)((double)sum / ((double)count * 2^24))"""
    keys, sums, counts = exported
    ok = counts >= min_count
    return keys[ok], (sums[ok].astype(np.float64) / (counts[ok].astype(np.float64) * FIX_ONE)).astype(dtype)


# ----------------------------------------------------------------------------------------------------------- the float64 form
def fused64(frames, voxel, origin=(0, 0, 0), truncation=None, step=None, min_range=0.0, max_range=100.0):
    """frames: [(xyz (n,3) float32, pose (4,4) float64)] -> (keys (m,) int64 sorted, D (m,) float64 = the mean of s, counts
    (m,), ambiguous keys as a set).  World coordinates; the lattice hangs at `origin`."""
    v, org = float(voxel), np.asarray(origin, np.float64)
    tau = 3.0 * v if truncation is None else float(truncation)
    h = v / 2.0 if step is None else float(step)
    total, number, doubt = {}, {}, set()
    shifts = np.array([[a, b, c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], np.float64) * AMBIGUOUS
    for xyz, pose in frames:
        x = np.asarray(xyz, F32).astype(np.float64).reshape(-1, 3)
        pose = np.asarray(pose, np.float64)
        with np.errstate(all="ignore"):
            r = np.sqrt((x * x).sum(axis=1))
            keep = (r >= min_range) & (r <= max_range) & (r > 0)
            x, r = x[keep], r[keep]
            o = pose[:3, 3]
            q = x @ pose[:3, :3].T + o
            u = (q - o) / r[:, None]
            prev = np.full((len(x), 3), np.iinfo(np.int64).min)
            for k in range(-steps(tau, h), steps(tau, h) + 1):
                t = r + k * h
                p = o + u * t[:, None]
                g = (p - org) / v
                idx = np.floor(g).astype(np.int64)
                off = (g - np.floor(g)) * v
                near = (np.minimum(off, v - off) < AMBIGUOUS).any(axis=1) | (np.abs(t) < AMBIGUOUS)
                for pp in p[near]:
                    for cell in np.floor((pp + shifts - org) / v).astype(np.int64):
                        doubt.add(int(L.pack_key(cell)))
                live = t > 0
                new = live & (idx != prev).any(axis=1)
                prev = np.where(live[:, None], idx, prev)
                c = org + (idx + 0.5) * v
                s = np.clip(((q - c) * u).sum(axis=1), -tau, tau)
                for kk, ss in zip(L.pack_key(idx[new]).tolist(), s[new].tolist()):
                    total[kk] = total.get(kk, 0.0) + ss
                    number[kk] = number.get(kk, 0) + 1
    keys = np.array(sorted(total), np.int64)
    return (keys, np.array([total[k] / number[k] for k in keys.tolist()]), np.array([number[k] for k in keys.tolist()], np.int64),
            doubt)


def compare_fields(got, want64):
    """the float32 field (keys, D) against fused64's result -> (largest |D - D64| over the unambiguous voxels both hold, the
    unambiguous voxels only one of them holds, the ambiguous share of all voxels)"""
    k32, d32 = got
    k64, d64, _, doubt = want64
    every = np.union1d(k32, k64)
    clear = np.array([k not in doubt for k in every.tolist()], bool)
    both = np.intersect1d(k32, k64)
    both = both[np.isin(both, every[clear])]
    err = np.abs(d32[np.searchsorted(k32, both)].astype(np.float64) - d64[np.searchsorted(k64, both)])
    lonely = np.setxor1d(k32, k64)
    lonely = lonely[np.isin(lonely, every[clear])]
    return (float(err.max()) if len(err) else 0.0), len(lonely), 1.0 - float(clear.mean()) if len(every) else 0.0


# -------------------------------------------------------------------------------------------------------- surface and mesh
class Grid:
    """the qualified voxels of a field by coordinates"""

    def __init__(self, keys, D):
        self.keys, self.D = np.asarray(keys, np.int64), np.asarray(D)
        self.at = {k: i for i, k in enumerate(self.keys.tolist())}

    def value(self, xyz):
        """D of the voxel with (unbiased) coordinates xyz, or None"""
        if any(not -L.BIAS <= int(c) < L.BIAS for c in xyz):
            return None
        i = self.at.get(int(L.pack_key(np.asarray(xyz, np.int64))))
        return None if i is None else self.D[i]


def _grad(G, x, D, dt):
    g = []
    for b in range(3):
        e = np.eye(3, dtype=np.int64)[b]
        Dp, Dm = G.value(x + e), G.value(x - e)
        g.append(Dp - Dm if Dp is not None and Dm is not None else dt(2) * (Dp - D) if Dp is not None
                 else dt(2) * (D - Dm) if Dm is not None else dt(0))
    return g


def surface(fld, voxel, dtype=F32):
    """fld = (keys, D) -> (keys (M,) int64, axes (M,) int32, xyz (M,3), normals (M,3)) sorted by (key, axis)"""
    dt = dtype
    G, v = Grid(*fld), dt(voxel)
    out = []
    with np.errstate(all="ignore"):
        for key, D0 in zip(G.keys.tolist(), G.D):
            x0 = L.unpack_key(key)
            c = (x0.astype(dt) + dt(0.5)) * v
            for a in range(3):
                x1 = x0 + np.eye(3, dtype=np.int64)[a]
                D1 = G.value(x1)
                if D1 is None or (D0 < 0) == (D1 < 0):
                    continue
                f = dt(D0 / (D0 - D1))
                g0, g1 = _grad(G, x0, D0, dt), _grad(G, x1, D1, dt)
                g = [dt(g0[b] + g1[b]) for b in range(3)]
                ln = np.sqrt(dt(dt(g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]))
                nrm = [dt(gb / ln) if ln > 0 else dt(0) for gb in g]
                pos = [dt(c[b] + dt(f * v)) if b == a else c[b] for b in range(3)]
                out.append((key, a, pos, nrm))
    out.sort(key=lambda t: (t[0], t[1]))
    return (np.array([t[0] for t in out], np.int64), np.array([t[1] for t in out], np.int32),
            np.array([t[2] for t in out], dt).reshape(-1, 3), np.array([t[3] for t in out], dt).reshape(-1, 3))


PERMUTATIONS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
DIRECTION = {1: 0, 2: 1, 4: 2, 3: 3, 5: 4, 6: 5, 7: 6}


def _parity(seq):
    return sum(1 for i in range(len(seq)) for j in range(i + 1, len(seq)) if seq[i] > seq[j]) & 1


def mesh(fld, voxel, dtype=F32):
    """fld = (keys, D) -> triangles (vertex_keys (n,3) int64, vertex_dirs (n,3) int32, xyz (n,3,3)), unsorted.  Written from
    the geometry: for a right-handed tetrahedron (A, B, C, D) the triangle on the edges AB, AC, AD has its normal pointing
    away from A; an odd ordering, a left-handed tetrahedron (an odd permutation of the axes) and a lone POSITIVE corner each
    turn it round."""
    dt = dtype
    G, v = Grid(*fld), dt(voxel)
    tk, td, tp = [], [], []
    with np.errstate(all="ignore"):
        for key in G.keys.tolist():
            x0 = L.unpack_key(key)
            corner = [x0 + np.array([m & 1, (m >> 1) & 1, m >> 2]) for m in range(8)]
            D = [G.value(c) for c in corner]
            if any(d is None for d in D) or len({bool(d < 0) for d in D}) == 1:
                continue

            def vertex(p, q):
                p, q = min(p, q), max(p, q)
                f = dt(D[p] / (D[p] - D[q]))
                c = (corner[p].astype(dt) + dt(0.5)) * v
                return (int(L.pack_key(corner[p])), DIRECTION[p ^ q],
                        [dt(c[b] + dt(f * v)) if ((p ^ q) >> b) & 1 else c[b] for b in range(3)])

            for perm in PERMUTATIONS:
                m = [0, 1 << perm[0], (1 << perm[0]) | (1 << perm[1]), 7]
                neg = [i for i in range(4) if D[m[i]] < 0]
                pos = [i for i in range(4) if not D[m[i]] < 0]
                tris = []
                if len(neg) in (1, 3):
                    A = (neg if len(neg) == 1 else pos)[0]
                    rest = [i for i in range(4) if i != A]
                    flip = _parity([A] + rest) ^ _parity(perm) ^ (len(neg) == 3)
                    tri = [(A, rest[0]), (A, rest[1]), (A, rest[2])]
                    tris.append([tri[0], tri[2], tri[1]] if flip else tri)
                elif len(neg) == 2:
                    (A, B), (C, E) = neg, pos
                    if _parity([A, B, C, E]) ^ _parity(perm):
                        C, E = E, C
                    tris += [[(A, C), (A, E), (B, E)], [(A, C), (B, E), (B, C)]]
                for tri in tris:
                    vs = [vertex(m[i], m[j]) for i, j in tri]
                    tk.append([t[0] for t in vs]), td.append([t[1] for t in vs]), tp.append([t[2] for t in vs])
    return (np.array(tk, np.int64).reshape(-1, 3), np.array(td, np.int32).reshape(-1, 3), np.array(tp, dt).reshape(-1, 3, 3))


def sort_triangles(vertex_keys, vertex_dirs, xyz):
    """triangles in a canonical order: by the names of their vertices, in the order given (the winding is part of the result)"""
    k, d, p = np.asarray(vertex_keys, np.int64).reshape(-1, 3), np.asarray(vertex_dirs, np.int32).reshape(-1, 3), np.asarray(xyz)
    order = np.lexsort((d[:, 2], k[:, 2], d[:, 1], k[:, 1], d[:, 0], k[:, 0])) if len(k) else np.zeros(0, np.int64)
    return k[order], d[order], p.reshape(-1, 3, 3)[order]


# --------------------------------------------------------------------------------------------------------------- mesh topology
def topology(faces):
    """faces (F,3) -> dict(V, E, F, closed: every undirected edge in exactly two triangles, oriented: every directed edge
    once, euler = V - E + F)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    und = np.sort(directed, axis=1)
    _, n_und = np.unique(und, axis=0, return_counts=True)
    _, n_dir = np.unique(directed, axis=0, return_counts=True)
    V, E, F = len(np.unique(f)), len(n_und), len(f)
    return dict(V=V, E=E, F=F, closed=bool((n_und == 2).all()), oriented=bool((n_dir == 1).all()), euler=V - E + F)


def signed_volume(vertices, faces):
    """of a closed mesh: positive when the faces' normals point outwards"""
    p = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)
