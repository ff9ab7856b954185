"""The ray-cast of the TSDF map restated in numpy, written from the contract (include/dpm_hip.h: dpm_tsdf_raycast; DESIGN §7l,
"Ray-casting the field").  The yardstick of tests/test_gpu_tsdf_raycast.py, beside tests/tsdf_register_restated.py, whose
float32 `sample` is the field at a point bit for bit.

  cast32   float32, operation for operation what the kernel does, from an exported field (keys sorted, D float32): u by the
           transform's fma chain without the translation, t_k = t0 + (float)k * h, p_k = o + u * t_k, the field at p_k, the first
           sign change between two valued samples in a row, f, range, the interpolated gradient, its unit, R^T.  It looks up
           every sample: nothing is skipped.  MUTANTS, as arguments: across_gap (a crossing accepted across samples without a
           value), sign_ge (s(d) = d >= 0), back_as_hit, map_normal (the normal left in the map frame), accumulate_t (t += h).
  cast64   float64 in WORLD coordinates, independent: no map-frame pose, its own trilinear code (the sum over the 8 corners of
           the product of the one-dimensional weights).  It also says which rays are AMBIGUOUS: up to the sample the ray ends
           at, a valued sample with |d| <= SIGN_EPS (a sign decision within rounding of zero), or a sample within NEAR_FACE
           voxels of a cell face whose neighbouring cell answers "has a value" differently.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lidar_odometry_restated as L  # noqa: E402
import tsdf_register_restated as RR  # noqa: E402

F32 = np.float32
MISS, HIT, BACK = 0, 1, 2
SIGN_EPS = 1e-5      # metres: what fp32 positions within ~100 m of the origin can move a field value of unit slope by
NEAR_FACE = 1e-5     # voxels
EYE = np.eye(4)


def samples(min_range, max_range, step):
    """K = floor((max_range - min_range) / step) + 1, in double as on the host"""
    return int(np.floor((float(max_range) - float(min_range)) / float(step))) + 1


def turn32(R, d):
    """fma(R2, z, fma(R1, y, R0 * x)) per axis in float32 (icp_restated.transform's chain without the translation)"""
    M = np.asarray(R, np.float64).astype(F32)
    s = np.asarray(d, F32)
    M64, s64 = M.astype(np.float64), s.astype(np.float64)
    a = (M[None, :, 0] * s[:, 0:1]).astype(F32)
    a = (M64[None, :, 1] * s64[:, 1:2] + a.astype(np.float64)).astype(F32)
    return (M64[None, :, 2] * s64[:, 2:3] + a.astype(np.float64)).astype(F32)


def cast32(fld, voxel, origin, poses, dirs, min_range, max_range, step, across_gap=False, sign_ge=False, back_as_hit=False,
           map_normal=False, accumulate_t=False):
    """fld = (keys sorted, D float32) of the qualified voxels; poses (F,4,4) float64 world; dirs (R,3) float32 sensor frame ->
    (range (F,R) float32, normals (F,R,3) float32, flag (F,R) int32)"""
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    dirs = np.ascontiguousarray(dirs, F32).reshape(-1, 3)
    origin = np.asarray(origin, np.float64)
    Fn, Rn = len(poses), len(dirs)
    K, t0, h = samples(min_range, max_range, step), F32(min_range), F32(step)
    rng, nrm, flag = np.zeros((Fn, Rn), F32), np.zeros((Fn, Rn, 3), F32), np.zeros((Fn, Rn), np.int32)
    sign = (lambda d: d >= 0) if sign_ge else (lambda d: d > 0)
    with np.errstate(all="ignore"):
        for f in range(Fn):
            if Rn == 0:
                continue
            M = poses[f, :3, :3].astype(F32)
            o = (poses[f, :3, 3] - origin).astype(F32)
            u = turn32(poses[f, :3, :3], dirs)
            prev, dp, gp = np.zeros(Rn, bool), np.zeros(Rn, F32), np.zeros((Rn, 3), F32)
            live = np.ones(Rn, bool)
            t_run = t0
            for k in range(K):
                if not live.any():
                    break
                t = t_run if accumulate_t else t0 + F32(k) * h
                t_before = (t_run - h if accumulate_t else t0 + F32(k - 1) * h)
                t_run = t_run + h
                ix = np.flatnonzero(live)
                p = o[None, :] + u[ix] * t
                s = RR.sample(fld, voxel, p, EYE, (0.0, 0.0, 0.0), F32)      # the identity's chain leaves p as it is
                has, d, g = s.flag == 1, s.d, s.grad
                cross = has & prev[ix] & (sign(dp[ix]) != sign(d))
                c = ix[cross]
                if len(c):
                    d0, d1, g0, g1 = dp[c], d[cross], gp[c], g[cross]
                    fr = d0 / (d0 - d1)
                    rng[f, c] = t_before + fr * h
                    flag[f, c] = HIT if back_as_hit else np.where(sign(d0), HIT, BACK)
                    gm = g0 + fr[:, None] * (g1 - g0)
                    ln = np.sqrt((gm[:, 0] * gm[:, 0] + gm[:, 1] * gm[:, 1]) + gm[:, 2] * gm[:, 2])
                    ok = (ln > 0) & np.isfinite(ln)
                    m = gm / ln[:, None]
                    n = m if map_normal else np.stack([(M[0, j] * m[:, 0] + M[1, j] * m[:, 1]) + M[2, j] * m[:, 2] for j in range(3)], axis=1)
                    nrm[f, c] = np.where(ok[:, None], n, F32(0)).astype(F32)
                    live[c] = False
                prev[ix] = (prev[ix] | has) if across_gap else has
                dp[ix] = np.where(has, d, dp[ix])
                gp[ix] = np.where(has[:, None], g, gp[ix])
    return rng, nrm, flag


# --------------------------------------------------------------------------------------------------------------- the float64 form
def _field64(table, g):
    """g (n,3) float64 in voxels, already shifted by -0.5 -> (has (n,), d (n,), grad in voxels^-1 (n,3), f (n,3)): the sum over
    the 8 corners of the product of the one-dimensional weights"""
    fl = np.floor(g)
    ok = np.isfinite(g).all(axis=1) & np.all((fl >= RR.CELL_LO) & (fl < RR.CELL_HI), axis=1)
    f = g - fl
    base = np.where(ok[:, None], fl, 0).astype(np.int64)
    n = len(g)
    d, grad, has = np.zeros(n), np.zeros((n, 3)), ok.copy()
    for cx in range(2):
        for cy in range(2):
            for cz in range(2):
                c = (cx, cy, cz)
                key = L.pack_key(base + np.array(c))
                val = np.array([table.get(int(kk), np.nan) for kk in key.tolist()]) if n else np.zeros(0)
                has &= ~np.isnan(val)
                w = [np.where(c[a] == 1, f[:, a], 1.0 - f[:, a]) for a in range(3)]
                sg = [1.0 if c[a] == 1 else -1.0 for a in range(3)]
                d += val * w[0] * w[1] * w[2]
                grad[:, 0] += val * sg[0] * w[1] * w[2]
                grad[:, 1] += val * w[0] * sg[1] * w[2]
                grad[:, 2] += val * w[0] * w[1] * sg[2]
    return has, d, grad, f


def cast64(fld64, voxel, origin, poses, dirs, min_range, max_range, step):
    """fld64 = (keys sorted, D float64) -> namespace(range, normals (sensor frame), flag, ambiguous (F,R) bool)"""
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    dirs = np.ascontiguousarray(dirs, F32).reshape(-1, 3).astype(np.float64)
    origin, v = np.asarray(origin, np.float64), float(voxel)
    table = dict(zip(np.asarray(fld64[0]).tolist(), np.asarray(fld64[1], np.float64).tolist()))
    Fn, Rn = len(poses), len(dirs)
    K = samples(min_range, max_range, step)
    rng, nrm, flag = np.zeros((Fn, Rn)), np.zeros((Fn, Rn, 3)), np.zeros((Fn, Rn), np.int32)
    doubt = np.zeros((Fn, Rn), bool)
    shifts = np.array([[a, b, c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], np.float64) * 2 * NEAR_FACE
    with np.errstate(all="ignore"):
        for fi in range(Fn):
            if Rn == 0:
                continue
            Rm, o = poses[fi, :3, :3], poses[fi, :3, 3]
            u = dirs @ Rm.T
            prev, dp, gp = np.zeros(Rn, bool), np.zeros(Rn), np.zeros((Rn, 3))
            live = np.ones(Rn, bool)
            for k in range(K):
                if not live.any():
                    break
                ix = np.flatnonzero(live)
                t = float(min_range) + k * float(step)
                g = ((o + u[ix] * t) - origin) / v - 0.5
                has, d, gr, fr3 = _field64(table, g)
                doubt[fi, ix] |= has & (np.abs(d) <= SIGN_EPS)
                near = np.flatnonzero((np.minimum(fr3, 1.0 - fr3) < NEAR_FACE).any(axis=1))
                for j in near.tolist():
                    other = _field64(table, g[j][None, :] + shifts)[0]
                    if (other != has[j]).any():
                        doubt[fi, ix[j]] = True
                cross = has & prev[ix] & ((dp[ix] > 0) != (d > 0))
                c = ix[cross]
                if len(c):
                    d0, d1, g0, g1 = dp[c], d[cross], gp[c], gr[cross]
                    fr = d0 / (d0 - d1)
                    rng[fi, c] = (float(min_range) + (k - 1) * float(step)) + fr * float(step)
                    flag[fi, c] = np.where(d0 > 0, HIT, BACK)
                    gm = (g0 + fr[:, None] * (g1 - g0)) / v
                    ln = np.linalg.norm(gm, axis=1)
                    ok = (ln > 0) & np.isfinite(ln)
                    nrm[fi, c] = np.where(ok[:, None], (gm / ln[:, None]) @ Rm, 0.0)     # R^T m
                    live[c] = False
                prev[ix] = has
                dp[ix] = np.where(has, d, dp[ix])
                gp[ix] = np.where(has[:, None], gr, gp[ix])
    return SimpleNamespace(range=rng, normals=nrm, flag=flag, ambiguous=doubt)


def compare(c32, c64):
    """(range32, normals32, flag32) against cast64's result on the unambiguous rays -> (rays whose flags differ, largest
    |range32 - range64| over the rays that end in both, largest |normal32 - normal64| there, the ambiguous share)"""
    r32, n32, f32 = c32
    clear = ~c64.ambiguous
    differ = int(((f32 != c64.flag) & clear).sum())
    both = clear & (f32 != MISS) & (c64.flag != MISS)
    dr = np.abs(r32.astype(np.float64) - c64.range)[both]
    dn = np.abs(n32.astype(np.float64) - c64.normals)[both]
    share = float(c64.ambiguous.mean()) if c64.ambiguous.size else 0.0
    return differ, (float(dr.max()) if dr.size else 0.0), (float(dn.max()) if dn.size else 0.0), share
