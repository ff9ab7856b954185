"""The map-evaluation kernels in numpy, written from the contract (include/dpm_hip.h: dpm_scene_distance / dpm_cloud_nn /
dpm_distance_stats and csrc/map_eval.hip's header comments).  Two forms:

* float32 in the header comment's order of operations (`records`, `scene_distance32`, `cloud_nn32`): numpy rounds each
  float32 operation once and fuses nothing, so the kernels' outputs are expected bit for bit;
* INDEPENDENT float64 in world coordinates with no origin shift (`scene_distance64`): case analysis per primitive (inside:
  the nearest face; outside: the distance to the clamped point) instead of the max / min form, a cylinder from its base and
  height as the scene stores it -- this one answers "is the float32 path right".

`stats` is the statistics table in exact arithmetic (math.fsum over the float32 values taken as float64).
"""
import math

import numpy as np

f32 = np.float32
INF32 = f32(np.inf)
REC = 12


# ------------------------------------------------------------------------------------------------------------
# float32, the kernels' order
# ------------------------------------------------------------------------------------------------------------
def shift(points, origin):
    """(3,M) float32 -> shifted (3,M) float32: q = (float)((double)p - origin)"""
    p = np.asarray(points)
    assert p.dtype == f32 and p.shape[0] == 3
    with np.errstate(all="ignore"):
        return (p.astype(np.float64) - np.asarray(origin, np.float64).reshape(3, 1)).astype(f32)


def records(params, kind, origin):
    """Scene.params (P,7), kind (P,) -> (P,12) float32: float64 arithmetic, rounded once; the kind as bits"""
    q = np.asarray(params, np.float64).reshape(-1, 7)
    o = np.asarray(origin, np.float64).reshape(3)
    rec = np.zeros((len(q), REC), f32)
    for p, (row, k) in enumerate(zip(q, kind)):
        if k == 0:
            vals = [row[0] - o[0], row[1] - o[1], row[2] - o[2], math.cos(row[6]), math.sin(row[6]), row[3], row[4], row[5]]
        else:
            vals = [row[0] - o[0], row[1] - o[1], (row[2] + 0.5 * row[4]) - o[2], 1.0, 0.0, row[3], 0.5 * row[4], 0.0]
        rec[p, :8] = np.asarray(vals, np.float64).astype(f32)
        rec[p, 8:9].view(np.int32)[0] = int(k)
    return rec


def scene_distance32(points, rec, ground, origin):
    """points (3,M) float32, rec (P,12) float32, ground = z0 - origin_z (float64) or None -> dist (M,) float32, surf (M,) int32"""
    q = shift(points, origin)
    qx, qy, qz = q[0], q[1], q[2]
    M = q.shape[1]
    best, bid = np.full(M, INF32, f32), np.full(M, -1, np.int32)
    zero = f32(0)
    with np.errstate(all="ignore"):
        for p, r in enumerate(rec):
            dx, dy, dz = qx - r[0], qy - r[1], qz - r[2]
            if r[8:9].view(np.int32)[0] == 0:
                lx, ly = r[3] * dx + r[4] * dy, r[3] * dy - r[4] * dx
                ax, ay, az = np.abs(lx) - r[5], np.abs(ly) - r[6], np.abs(dz) - r[7]
                ox, oy, oz = np.where(ax > zero, ax, zero), np.where(ay > zero, ay, zero), np.where(az > zero, az, zero)
                myz = np.where(ay > az, ay, az)
                m = np.where(ax > myz, ax, myz)
                d = np.abs(np.sqrt((ox * ox + oy * oy) + oz * oz) + np.where(m < zero, m, zero))
            else:
                a0, a1 = np.sqrt(dx * dx + dy * dy) - r[5], np.abs(dz) - r[6]
                o0, o1 = np.where(a0 > zero, a0, zero), np.where(a1 > zero, a1, zero)
                m = np.where(a0 > a1, a0, a1)
                d = np.abs(np.sqrt(o0 * o0 + o1 * o1) + np.where(m < zero, m, zero))
            assert d.dtype == f32
            upd = d < best
            best, bid = np.where(upd, d, best), np.where(upd, np.int32(p), bid)
        if ground is not None:
            d = np.abs(qz - f32(ground))
            upd = d < best
            best, bid = np.where(upd, d, best), np.where(upd, np.int32(len(rec)), bid)
    ok = np.isfinite(qx) & np.isfinite(qy) & np.isfinite(qz)
    return np.where(ok, best, INF32).astype(f32), np.where(ok, bid, -1).astype(np.int32)


def cloud_nn32(query, target, max_dist, origin, block=512):
    """exhaustive: every query against every target.  -> dist (Nq,) float32, idx (Nq,) int32"""
    q, t = shift(query, origin), shift(target, origin)
    Nq, Nt = q.shape[1], t.shape[1]
    r2 = f32(float(max_dist) * float(max_dist))
    dist, idx = np.full(Nq, INF32, f32), np.full(Nq, -1, np.int32)
    if Nt == 0:
        return dist, idx
    usable = np.isfinite(t).all(axis=0)
    with np.errstate(all="ignore"):
        for a in range(0, Nq, block):
            b = min(a + block, Nq)
            dx, dy, dz = (q[k, a:b, None] - t[k][None, :] for k in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == f32
            d2 = np.where(usable[None, :] & ~np.isnan(d2), d2, INF32)
            win = np.argmin(d2, axis=1)                         # the first of equal minima = the smallest index
            best = d2[np.arange(b - a), win]
            hit = best <= r2
            dist[a:b] = np.where(hit, np.sqrt(best), INF32)
            idx[a:b] = np.where(hit, win, -1)
    return dist, idx


# ------------------------------------------------------------------------------------------------------------
# float64, world coordinates, independent formulas
# ------------------------------------------------------------------------------------------------------------
def primitive_distance64(row, k, X):
    """row = Scene.params[p] (x, y, z, e0, e1, e2, yaw), k its kind, X (3,M) float64 world points -> (M,) float64"""
    if k == 0:
        c, s = math.cos(row[6]), math.sin(row[6])
        rx, ry = X[0] - row[0], X[1] - row[1]
        L = np.stack([c * rx + s * ry, -s * rx + c * ry, X[2] - row[2]])
        h = np.asarray(row[3:6]).reshape(3, 1)
        nearest = np.clip(L, -h, h)                           # the nearest point of the solid box
        outside = np.sqrt(((L - nearest) ** 2).sum(axis=0))
        inside = (h - np.abs(L)).min(axis=0)                  # depth below the nearest face
        return np.where((np.abs(L) <= h).all(axis=0), inside, outside)
    r, H = row[3], row[4]
    rho = np.hypot(X[0] - row[0], X[1] - row[1])
    z = X[2] - row[2]                                         # above the base
    zc, rc = np.clip(z, 0.0, H), np.minimum(rho, r)           # the nearest point of the solid cylinder
    outside = np.hypot(rho - rc, z - zc)
    inside = np.minimum(r - rho, np.minimum(z, H - z))
    return np.where((rho <= r) & (z >= 0) & (z <= H), inside, outside)


def scene_distance64(params, kind, z0, X):
    """-> dist (M,), surf (M,), gap (M,) = the distance of the SECOND nearest surface minus the nearest's (inf with one
    surface): small gaps are the points where float32 and float64 may legitimately name different surfaces"""
    X = np.asarray(X, np.float64)
    rows = [primitive_distance64(row, k, X) for row, k in zip(np.asarray(params, np.float64).reshape(-1, 7), kind)]
    if z0 is not None:
        rows.append(np.abs(X[2] - z0))
    M = X.shape[1]
    if not rows:
        return np.full(M, np.inf), np.full(M, -1), np.full(M, np.inf)
    D = np.stack(rows)
    surf = np.argmin(D, axis=0)
    dist = D[surf, np.arange(M)]
    if len(rows) > 1:
        second = np.partition(D, 1, axis=0)[1]
    else:
        second = np.full(M, np.inf)
    return dist, surf, second - dist


# ------------------------------------------------------------------------------------------------------------
# statistics, exact
# ------------------------------------------------------------------------------------------------------------
def stats(dist, thresholds, max_dist, surf=None, class_id=None, C=0):
    """-> (C+1, 5+T) float64 with math.fsum sums over the float32 values; thresholds and max_dist rounded to float32"""
    d = np.asarray(dist)
    assert d.dtype == f32
    thr = [f32(t) for t in thresholds]
    md = f32(max_dist)
    matched = np.isfinite(d) & (d <= md)
    out = np.zeros((C + 1, 5 + len(thr)), np.float64)
    cls = None
    if C:
        s = np.asarray(surf)
        ok = (s >= 0) & (s < len(class_id))
        cls = np.where(ok, np.asarray(class_id)[np.where(ok, s, 0)], -1)
    for row in range(C + 1):
        sel = np.ones(len(d), bool) if row == C else cls == row
        m = sel & matched
        v = d[m].astype(np.float64)
        out[row, 0], out[row, 1] = m.sum(), (sel & ~matched).sum()
        out[row, 2], out[row, 3] = math.fsum(v.tolist()), math.fsum((v * v).tolist())      # v * v is exact in float64
        out[row, 4] = v.max() if len(v) else 0.0
        for k, t in enumerate(thr):
            out[row, 5 + k] = (m & (d <= t)).sum()
    return out
