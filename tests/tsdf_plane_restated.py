"""The plane-distance fusion and the free-space carving of the TSDF map restated in numpy, written from the contract
(include/dpm_hip.h: dpm_tsdf_integrate_planes, dpm_tsdf_carve).  The yardstick of tests/test_gpu_tsdf_plane.py,
beside tests/tsdf_restated.py, whose field, surface and mesh read what these forms export.

Two forms:
  FusedPlane  float32, operation for operation what csrc/tsdf_map.hip does.  integrate: the ray rule of tsdf_restated.Fused
              (range gate, fma chain, u, the samples, the voxel, the skip of a repeated key) with the normal turned by the
              pose's rotation in the same fma chain, a0 = n_m . u, the flip m = +-n_m away from the sensor, a = |a0|, wq =
              rint(256 a), the row gate (wq >= 1 and a >= cos_min; header word 2 counts the rows it stops), s = m . (q - c)
              clamped, sum += wq rint(s 2^24), count += wq.  `carve` (a function: it serves ray maps too): lookups only, t =
              (float)k h < r - margin, sum += weight rint(tau 2^24), count += weight.
              MUTANTS: flip=False (no orientation flip), weigh_sum=False (the weight not applied to the sum), use_m=False (u
              instead of m in s), carve(..., claims=True) (a carve that claims slots).
  Fused64     float64 in WORLD coordinates, independent: no map-frame pose, no fixed point, float sums.  Beside
              tsdf_restated.fused64's ambiguous voxels (a sample within 1e-5 m of a voxel face or of t = 0; for a carve also of
              t = r - margin) it marks every voxel touched by a row whose 256 a lies within 5e-4 of a half-integer (the weight
              may round the other way) or whose a lies within 1e-6 of cos_min or of 0 (the row gate may fall the other way).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restated as I  # noqa: E402
import lidar_odometry_restated as L  # noqa: E402
import tsdf_restated as R  # noqa: E402

F32 = np.float32
FIX_ONE = R.FIX_ONE
WEIGHT_ONE = 256
HALF_BAND = 5e-4      # of 256 a round a half-integer
GATE_BAND = 1e-6      # of a round cos_min and round 0


def rotate32(P, n):
    """n (k,3) float32 turned by the (float) rotation of P (4,4 float64) in the kernel's chain fma(R2, z, fma(R1, y, R0 * x)):
    a float32 product is exact in float64, so rounding product + addend from float64 is the fused operation"""
    M = P[:3, :3].astype(F32)
    M64, n64 = M.astype(np.float64), n.astype(np.float64)
    a = (M[None, :, 0] * n[:, 0:1]).astype(F32)
    a = (M64[None, :, 1] * n64[:, 1:2] + a.astype(np.float64)).astype(F32)
    return (M64[None, :, 2] * n64[:, 2:3] + a.astype(np.float64)).astype(F32)


def _ray32(m, xyz, pose):
    """what every form starts from: (keep, r, q, o, u) in float32 under the map's range gate"""
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    r2 = (x * x + y * y) + z * z
    keep = (r2 >= m.lo2) & (r2 <= m.hi2)
    r = np.sqrt(r2)
    P = L.map_pose(pose, m.origin)
    q = I.transform(P, xyz, F32)
    o = P[:3, 3].astype(F32)
    return keep, r, q, o, (q - o[None, :]) / r[:, None], P


def _cells32(p, v):
    fl = np.floor(p / v)
    return fl, np.all((fl >= -L.BIAS) & (fl < L.BIAS), axis=1)


class FusedPlane(R.Fused):
    """{key: [sum, count]} under the plane-distance rule, float32; `unusable` is header word 2"""

    def __init__(self, voxel, origin=(0, 0, 0), truncation=None, step=None, min_range=0.0, max_range=100.0, cos_min=0.0, flip=True,
                 weigh_sum=True, use_m=True):
        super().__init__(voxel, origin, truncation, step, min_range, max_range)
        self.cos_min, self.flip, self.weigh_sum, self.use_m = float(cos_min), flip, weigh_sum, use_m
        self.unusable = 0

    def integrate(self, xyz, pose, normals):
        """xyz, normals (n,3) float32 valid rows (sensor frame), pose (4,4) float64"""
        xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
        nrm = np.ascontiguousarray(normals, F32).reshape(-1, 3)
        assert nrm.shape == xyz.shape
        if len(xyz) == 0:
            return self
        v, tau, h = F32(self.voxel), F32(self.tau), F32(self.h)
        with np.errstate(all="ignore"):
            keep, r, q, o, u, P = _ray32(self, xyz, pose)
            nm = rotate32(P, nrm)
            a0 = (nm[:, 0] * u[:, 0] + nm[:, 1] * u[:, 1]) + nm[:, 2] * u[:, 2]
            a = np.abs(a0)
            wf = np.rint(a * F32(256))
            usable = (wf >= 1) & (a >= F32(self.cos_min))          # a NaN fails both
            self.unusable += int((keep & ~usable).sum())
            keep = keep & usable
            wq = np.where(keep, wf, 0).astype(np.int64)
            m = np.where((a0 >= 0)[:, None], nm, -nm) if self.flip else nm
            d = m if self.use_m else u
            prev = np.full(len(xyz), -1, np.int64)
            keys, fixed, weight = [], [], []
            n = R.steps(self.tau, self.h)
            for k in range(-n, n + 1):
                t = r + F32(k) * h
                live = keep & (t > 0)
                fl, inside = _cells32(o[None, :] + u * t[:, None], v)
                self.outside += int((live & ~inside).sum())
                live &= inside
                fl = np.where(live[:, None], fl, 0)
                key = L.pack_key(fl.astype(np.int64))
                new = live & (key != prev)
                prev = np.where(live, key, prev)
                e = q - (fl + F32(0.5)) * v
                s = (d[:, 0] * e[:, 0] + d[:, 1] * e[:, 1]) + d[:, 2] * e[:, 2]
                s = np.minimum(np.maximum(s, -tau), tau)
                keys.append(key[new])
                fixed.append(np.rint(s[new] * F32(FIX_ONE)).astype(np.int64))
                weight.append(wq[new])
        keys, fixed, weight = np.concatenate(keys), np.concatenate(fixed), np.concatenate(weight)
        uk, inv = np.unique(keys, return_inverse=True)
        total, number = np.zeros(len(uk), np.int64), np.zeros(len(uk), np.int64)
        np.add.at(total, inv, fixed * weight if self.weigh_sum else fixed)
        np.add.at(number, inv, weight)
        for kk, a_, b_ in zip(uk.tolist(), total.tolist(), number.tolist()):
            self.sum[kk] = self.sum.get(kk, 0) + a_
            self.count[kk] = self.count.get(kk, 0) + b_
        return self

    def integrate_frames(self, store, lengths, frames, poses, normals):
        """store (capacity,3,P), normals (capacity,P,3)"""
        store, normals = np.asarray(store, F32), np.asarray(normals, F32)
        for row, pose in zip(frames, np.asarray(poses, np.float64).reshape(-1, 4, 4)):
            if not 0 <= int(row) < store.shape[0]:
                continue
            n = min(max(int(lengths[row]), 0), store.shape[2])
            self.integrate(store[row, :, :n].T, pose, normals[row, :n])
        return self


def carve(m, xyz, pose, weight, margin, claims=False):
    """the free space of one frame into the map m (a tsdf_restated.Fused or a FusedPlane): lookups only.  weight in count
    units.  claims=True: the mutant that adds the voxels it does not find.  -> m"""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    if len(xyz) == 0:
        return m
    v, h = F32(m.voxel), F32(m.h)
    add = int(weight) * int(np.rint(F32(m.tau) * F32(FIX_ONE)))
    held = set(m.sum)                      # the key set before the call: a carve never looks at what it wrote
    hits = []
    with np.errstate(all="ignore"):
        keep, r, q, o, u, _ = _ray32(m, xyz, pose)
        lim = r - F32(margin)
        prev = np.full(len(xyz), -1, np.int64)
        k = 1
        while True:
            t = F32(k) * h
            live = keep & (t < lim)
            if not live.any():
                break                      # t grows with k: no later sample of any row is live
            fl, inside = _cells32(o[None, :] + u * t, v)
            live &= inside
            key = L.pack_key(np.where(live[:, None], fl, 0).astype(np.int64))
            new = live & (key != prev)
            prev = np.where(live, key, prev)
            hits.append(key[new])
            k += 1
    if hits:
        uk, times = np.unique(np.concatenate(hits), return_counts=True)
        for kk, n in zip(uk.tolist(), times.tolist()):
            if kk in held or claims:
                m.sum[kk] = m.sum.get(kk, 0) + n * add
                m.count[kk] = m.count.get(kk, 0) + n * int(weight)
    return m


def carve_frames(m, store, lengths, frames, poses, weight, margin):
    store = np.asarray(store, F32)
    for row, pose in zip(frames, np.asarray(poses, np.float64).reshape(-1, 4, 4)):
        if 0 <= int(row) < store.shape[0]:
            carve(m, store[row, :, :min(max(int(lengths[row]), 0), store.shape[2])].T, pose, weight, margin)
    return m


# ----------------------------------------------------------------------------------------------------------- the float64 form
class Fused64:
    """float64, world coordinates; the lattice hangs at `origin`.  total / number: {key: sum of w s, sum of w}; doubt: the
    ambiguous keys"""

    def __init__(self, voxel, origin=(0, 0, 0), truncation=None, step=None, min_range=0.0, max_range=100.0, cos_min=0.0):
        self.v, self.org = float(voxel), np.asarray(origin, np.float64)
        self.tau = 3.0 * self.v if truncation is None else float(truncation)
        self.h = self.v / 2.0 if step is None else float(step)
        self.lo, self.hi, self.cos_min = float(min_range), float(max_range), float(cos_min)
        self.total, self.number, self.doubt = {}, {}, set()
        self.shifts = np.array([[a, b, c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], np.float64) * R.AMBIGUOUS

    def _rays(self, xyz, pose):
        x = np.asarray(xyz, F32).astype(np.float64).reshape(-1, 3)
        pose = np.asarray(pose, np.float64)
        r = np.sqrt((x * x).sum(axis=1))
        keep = (r >= self.lo) & (r <= self.hi) & (r > 0)
        o = pose[:3, 3]
        q = x @ pose[:3, :3].T + o
        with np.errstate(all="ignore"):
            u = (q - o) / r[:, None]
        return keep, r, q, o, u, pose

    def _cells(self, p, extra):
        """-> (idx, the rows whose sample is ambiguous); their neighbouring voxels go to `doubt`"""
        g = (p - self.org) / self.v
        off = (g - np.floor(g)) * self.v
        near = (np.minimum(off, self.v - off) < R.AMBIGUOUS).any(axis=1) | extra
        for pp in p[near]:
            for cell in np.floor((pp + self.shifts - self.org) / self.v).astype(np.int64):
                self.doubt.add(int(L.pack_key(cell)))
        return np.floor(g).astype(np.int64)

    def integrate(self, xyz, pose, normals):
        keep, r, q, o, u, pose = self._rays(xyz, pose)
        nrm = np.asarray(normals, F32).astype(np.float64).reshape(-1, 3) @ pose[:3, :3].T
        with np.errstate(all="ignore"):
            a0 = (nrm * u).sum(axis=1)
            a = np.abs(a0)
            w = np.rint(256.0 * a)
            frac = 256.0 * a - np.floor(256.0 * a)
            shaky = keep & np.isfinite(a) & ((np.abs(frac - 0.5) < HALF_BAND) | (np.abs(a - self.cos_min) < GATE_BAND) | (a < GATE_BAND))
            usable = keep & (w >= 1) & (a >= self.cos_min)
        m = np.where((a0 >= 0)[:, None], nrm, -nrm)
        prev = np.full((len(r), 3), np.iinfo(np.int64).min)
        n = R.steps(self.tau, self.h)
        for k in range(-n, n + 1):
            t = r + k * self.h
            on = (usable | shaky) & (t > -R.AMBIGUOUS)
            idx = np.zeros((len(r), 3), np.int64)
            if on.any():
                idx[on] = self._cells(o + u[on] * t[on, None], np.abs(t[on]) < R.AMBIGUOUS)
            for cell in idx[on & shaky]:                           # every voxel a shaky row touches
                self.doubt.add(int(L.pack_key(cell)))
            live = usable & (t > 0)
            new = live & (idx != prev).any(axis=1)
            prev = np.where(live[:, None], idx, prev)
            c = self.org + (idx + 0.5) * self.v
            s = np.clip(((q - c) * m).sum(axis=1), -self.tau, self.tau)
            for kk, ss, ww in zip(L.pack_key(idx[new]).tolist(), s[new].tolist(), w[new].tolist()):
                self.total[kk] = self.total.get(kk, 0.0) + ww * ss
                self.number[kk] = self.number.get(kk, 0.0) + ww
        return self

    def integrate_ray(self, xyz, pose):
        """the along-ray rule with weight 1 a sample (a ray-distance map to carve)"""
        keep, r, q, o, u, pose = self._rays(xyz, pose)
        prev = np.full((len(r), 3), np.iinfo(np.int64).min)
        n = R.steps(self.tau, self.h)
        for k in range(-n, n + 1):
            t = r + k * self.h
            on = keep & (t > -R.AMBIGUOUS)
            idx = np.zeros((len(r), 3), np.int64)
            if on.any():
                idx[on] = self._cells(o + u[on] * t[on, None], np.abs(t[on]) < R.AMBIGUOUS)
            live = keep & (t > 0)
            new = live & (idx != prev).any(axis=1)
            prev = np.where(live[:, None], idx, prev)
            s = np.clip(((q - (self.org + (idx + 0.5) * self.v)) * u).sum(axis=1), -self.tau, self.tau)
            for kk, ss in zip(L.pack_key(idx[new]).tolist(), s[new].tolist()):
                self.total[kk] = self.total.get(kk, 0.0) + ss
                self.number[kk] = self.number.get(kk, 0.0) + 1.0
        return self

    def carve(self, xyz, pose, weight, margin):
        keep, r, q, o, u, _ = self._rays(xyz, pose)
        lim = r - float(margin)
        held = set(self.total)
        prev = np.full((len(r), 3), np.iinfo(np.int64).min)
        times = {}
        k = 1
        while True:
            t = k * self.h
            on = keep & (t < lim + R.AMBIGUOUS)
            if not on.any():
                break
            idx = np.zeros((len(r), 3), np.int64)
            idx[on] = self._cells(o + u[on] * t, np.abs(t - lim[on]) < R.AMBIGUOUS)
            live = keep & (t < lim)
            new = live & (idx != prev).any(axis=1)
            prev = np.where(live[:, None], idx, prev)
            for kk in L.pack_key(idx[new]).tolist():
                times[kk] = times.get(kk, 0) + 1
            k += 1
        for kk, n in times.items():
            if kk in held:
                self.total[kk] += n * weight * self.tau
                self.number[kk] += n * weight
        return self

    def result(self):
        """-> (keys sorted, D, counts, ambiguous keys): what tsdf_restated.compare_fields takes"""
        keys = np.array(sorted(self.total), np.int64)
        return (keys, np.array([self.total[k] / self.number[k] for k in keys.tolist()]),
                np.array([self.number[k] for k in keys.tolist()]), self.doubt)
