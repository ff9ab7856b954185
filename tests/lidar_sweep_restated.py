"""Sweep motion in numpy, written from the contract (deeppointmap_amd/lidar_sim.py's docstring, DESIGN §7i, include/dpm_hip.h:
dpm_lidar_cull_sweep / dpm_lidar_cast_sweep / dpm_points_deskew).  The reference has no counterpart.

* `delta64`, `log64`, `exp64`, `motion64`: the model D = P0^-1 P1, D(s) = (Exp(s Log R_D), s t_D) in float64;
* `table64`: the column table of the sweep cull in float64 (the kernel's float32 entries are expected within one ulp);
* `cast32_sweep`: the sweep cast in float32 in the kernel's order of operations, FED a table (the device's own), so the
  kernel's outputs are expected bit for bit;
* `cast64_sweep`: an INDEPENDENT float64 cast -- no table, no sensor frame: every column gets its own world pose
  P0 D(s_c) and its rays go through `cast64_rays`, which is lidar_sim_restated.cast64_dirs with one origin per ray (the
  host test checks the two equal on whole columns; cast64_dirs itself would take one call per column, frame and tilt);
* `deskew64`: D(s_ref)^-1 D(s) p in float64.
"""
import numpy as np

import lidar_sim_restated as RS

f32 = np.float32
INF32 = f32(np.inf)


# ------------------------------------------------------------------------------------------------------------
# the model, float64
# ------------------------------------------------------------------------------------------------------------
def delta64(P0, P1):
    D = np.eye(4)
    D[:3, :3] = P0[:3, :3].T @ P1[:3, :3]
    D[:3, 3] = P0[:3, :3].T @ (P1[:3, 3] - P0[:3, 3])
    return D


def log64(R):
    """rotation vector, angle below pi"""
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    n = np.linalg.norm(v)
    return np.zeros(3) if n == 0 else v / n * np.arctan2(n, 0.5 * (np.trace(R) - 1.0))


def exp64(w, s=1.0):
    """Exp(s w) for s a number -> (3,3), or an array (n,) -> (n,3,3)"""
    s = np.asarray(s, np.float64)
    angle = np.linalg.norm(w)
    if angle == 0:
        return np.broadcast_to(np.eye(3), s.shape + (3, 3)).copy()
    k = w / angle
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    a = (s * angle)[..., None, None]
    return np.eye(3) + np.sin(a) * K + 2.0 * np.sin(0.5 * a) ** 2 * (K @ K)


def motion64(D, s):
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = exp64(log64(D[:3, :3]), s), s * D[:3, 3]
    return out


def table64(P0, P1, A):
    """(A,12) float64: Exp(s_c w) row-major and s_c t_D, s_c = c / A"""
    D = delta64(P0, P1)
    s = np.arange(A, dtype=np.float64) / A
    return np.concatenate([exp64(log64(D[:3, :3]), s).reshape(A, 9), s[:, None] * D[:3, 3][None, :]], axis=1)


def travel64(P0, P1):
    return float(np.linalg.norm(delta64(P0, P1)[:3, 3]))


# ------------------------------------------------------------------------------------------------------------
# cast, float32, the kernel's order of operations; the origin differs from ray to ray
# ------------------------------------------------------------------------------------------------------------
def _slab32(o, dd, lo, hi):
    with np.errstate(all="ignore"):
        t1, t2 = (lo - o) / dd, (hi - o) / dd
    zero = dd == 0
    first = t1 < t2
    tn = np.where(zero, -INF32, np.where(first, t1, t2))
    tf = np.where(zero, INF32, np.where(first, t2, t1))
    return np.where(zero, ~((o < lo) | (o > hi)), True), tn, tf


def cast32_sweep(rec, ids, kinds, plane, P, dirs, table, min_range, max_range):
    """one frame: rec / ids / kinds / plane from lidar_sim_restated.cull about the START pose (max_range enlarged by the
    travel), dirs (rays,3) float32, table (A,12) float32 with rays a multiple of A -> range, prim, cos_inc (rays,)"""
    dirs, table = np.asarray(dirs), np.asarray(table)
    assert dirs.dtype == f32 and rec.dtype == f32 and table.dtype == f32 and plane.dtype == f32
    n, A = dirs.shape[0], table.shape[0]
    assert n % A == 0
    e = table[np.arange(n) % A]
    x, y, z = dirs[:, 0], dirs[:, 1], dirs[:, 2]
    d0 = (e[:, 0] * x + e[:, 1] * y) + e[:, 2] * z
    d1 = (e[:, 3] * x + e[:, 4] * y) + e[:, 5] * z
    d2 = (e[:, 6] * x + e[:, 7] * y) + e[:, 8] * z
    o0, o1, o2 = e[:, 9], e[:, 10], e[:, 11]
    best, bcos, bid = np.full(n, INF32, f32), np.zeros(n, f32), np.full(n, -1, np.int32)
    zero = f32(0)
    for q, pid, k in zip(rec, ids, kinds):
        ox = q[0] + ((q[3] * o0 + q[4] * o1) + q[5] * o2)
        oy = q[1] + ((q[6] * o0 + q[7] * o1) + q[8] * o2)
        oz = q[2] + ((q[9] * o0 + q[10] * o1) + q[11] * o2)
        dx = (q[3] * d0 + q[4] * d1) + q[5] * d2
        dy = (q[6] * d0 + q[7] * d1) + q[8] * d2
        dz = (q[9] * d0 + q[10] * d1) + q[11] * d2
        if k == 0:
            okx, nx, fx = _slab32(ox, dx, -q[12], q[12])
            oky, ny, fy = _slab32(oy, dy, -q[13], q[13])
            okz, nz, fz = _slab32(oz, dz, -q[14], q[14])
            hit = okx & oky & okz
            enter, cen = nx, np.abs(dx)
            m = ny > enter
            enter, cen = np.where(m, ny, enter), np.where(m, np.abs(dy), cen)
            m = nz > enter
            enter, cen = np.where(m, nz, enter), np.where(m, np.abs(dz), cen)
            exit_, cex = fx, np.abs(dx)
            m = fy < exit_
            exit_, cex = np.where(m, fy, exit_), np.where(m, np.abs(dy), cex)
            m = fz < exit_
            exit_, cex = np.where(m, fz, exit_), np.where(m, np.abs(dz), cex)
        else:
            rad = q[12]
            a = dx * dx + dy * dy
            with np.errstate(all="ignore"):
                cr = np.abs(ox * dy - oy * dx)
                qa = rad * np.sqrt(a)
                disc = (qa - cr) * (qa + cr)
                ok = disc >= 0
                sd = np.sqrt(np.where(ok, disc, zero))
                half = sd / a
                tm = (zero - (ox * dx + oy * dy)) / a
                ns, fs, cs = tm - half, tm + half, sd / rad
            az = a == 0
            hit = np.where(az, ox * ox + oy * oy <= rad * rad, ok)
            ns, fs, cs = np.where(az, -INF32, ns), np.where(az, INF32, fs), np.where(az, zero, cs)
            okz, nz, fz = _slab32(oz, dz, zero, q[13])
            hit = hit & okz
            enter, cen = ns, cs
            m = nz > enter
            enter, cen = np.where(m, nz, enter), np.where(m, np.abs(dz), cen)
            exit_, cex = fs, cs
            m = fz < exit_
            exit_, cex = np.where(m, fz, exit_), np.where(m, np.abs(dz), cex)
        hit = hit & (enter <= exit_) & (exit_ > 0)
        front = enter > 0
        t, c = np.where(front, enter, exit_), np.where(front, cen, cex)
        upd = hit & (t < best)
        best, bcos, bid = np.where(upd, t, best), np.where(upd, c, bcos), np.where(upd, np.int32(pid), bid)
    den = (plane[0] * d0 + plane[1] * d1) + plane[2] * d2
    with np.errstate(all="ignore"):
        t = (plane[3] - ((plane[0] * o0 + plane[1] * o1) + plane[2] * o2)) / den
    upd = (den != 0) & (t > 0) & (t < best)
    best, bcos, bid = np.where(upd, t, best), np.where(upd, np.abs(den), bcos), np.where(upd, np.int32(P), bid)
    ret = (bid >= 0) & ~(best < f32(min_range)) & ~(best > f32(max_range))
    return (np.where(ret, best, zero).astype(f32), np.where(ret, bid, -1).astype(np.int32),
            np.where(ret, bcos, zero).astype(f32))


def cull_sweep(prims, kind, ground, P0, P1, max_range):
    """the records of the sweep cull: lidar_sim_restated.cull about the start pose with the reach enlarged by |t_D|"""
    return RS.cull(prims, kind, ground, P0, max_range + travel64(P0, P1))


# ------------------------------------------------------------------------------------------------------------
# cast, float64, world coordinates, one origin per ray
# ------------------------------------------------------------------------------------------------------------
def _slab64(o, dd, lo, hi):
    with np.errstate(all="ignore"):
        t1, t2 = (lo - o) / dd, (hi - o) / dd
    zero = dd == 0
    tn = np.where(zero, -np.inf, np.minimum(t1, t2))
    tf = np.where(zero, np.inf, np.maximum(t1, t2))
    return np.where(zero, (lo <= o) & (o <= hi), True), tn, tf


def cast64_rays(params, kind, z0, origins, D, min_range, max_range):
    """lidar_sim_restated.cast64_dirs with origins (n,3): params (P,7), kind (P,), z0 or None, D (n,3) float64 unit
    directions in the WORLD -> range, prim, cos_inc (n,)"""
    n = D.shape[0]
    best, bcos, bid = np.full(n, np.inf), np.zeros(n), np.full(n, -1, np.int64)
    for pid, (q, k) in enumerate(zip(params, kind)):
        rel = origins - q[:3]
        if k == 0:
            c, s = np.cos(q[6]), np.sin(q[6])
            o = np.stack([c * rel[:, 0] + s * rel[:, 1], -s * rel[:, 0] + c * rel[:, 1], rel[:, 2]], axis=1)
            d = np.stack([c * D[:, 0] + s * D[:, 1], -s * D[:, 0] + c * D[:, 1], D[:, 2]], axis=1)
            slabs = [_slab64(o[:, a], d[:, a], -q[3 + a], q[3 + a]) for a in range(3)]
            hit = slabs[0][0] & slabs[1][0] & slabs[2][0]
            tn, tf = np.stack([s_[1] for s_ in slabs]), np.stack([s_[2] for s_ in slabs])
            ia, ix = np.argmax(tn, axis=0), np.argmin(tf, axis=0)
            enter, exit_ = tn.max(axis=0), tf.min(axis=0)
            ad = np.abs(d)
            cen, cex = ad[np.arange(n), ia], ad[np.arange(n), ix]
        else:
            r, H = q[3], q[4]
            A = D[:, 0] ** 2 + D[:, 1] ** 2
            B = rel[:, 0] * D[:, 0] + rel[:, 1] * D[:, 1]
            C = rel[:, 0] ** 2 + rel[:, 1] ** 2 - r * r
            with np.errstate(all="ignore"):
                disc = B * B - A * C
                ok = disc >= 0
                root = np.sqrt(np.where(ok, disc, 0.0))
                ns, fs = (-B - root) / A, (-B + root) / A
            vertical = A == 0
            hit = np.where(vertical, C <= 0, ok)
            ns, fs = np.where(vertical, -np.inf, ns), np.where(vertical, np.inf, fs)
            okz, nz, fz = _slab64(rel[:, 2], D[:, 2], 0.0, H)
            hit = hit & okz
            enter, exit_ = np.maximum(ns, nz), np.minimum(fs, fz)
            side_in, side_out = ns >= nz, fs <= fz

            def side_cos(t):
                with np.errstate(all="ignore"):
                    px, py = rel[:, 0] + t * D[:, 0], rel[:, 1] + t * D[:, 1]
                    return np.abs(px * D[:, 0] + py * D[:, 1]) / r
            cen = np.where(side_in, side_cos(ns), np.abs(D[:, 2]))
            cex = np.where(side_out, side_cos(fs), np.abs(D[:, 2]))
        hit = hit & (enter <= exit_) & (exit_ > 0)
        front = enter > 0
        t, c = np.where(front, enter, exit_), np.where(front, cen, cex)
        upd = hit & (t < best)
        best, bcos, bid = np.where(upd, t, best), np.where(upd, c, bcos), np.where(upd, pid, bid)
    if z0 is not None:
        with np.errstate(all="ignore"):
            t = (z0 - origins[:, 2]) / D[:, 2]
        upd = (D[:, 2] != 0) & (t > 0) & (t < best)
        best, bcos, bid = np.where(upd, t, best), np.where(upd, np.abs(D[:, 2]), bcos), np.where(upd, len(kind), bid)
    ret = (bid >= 0) & (best >= min_range) & (best <= max_range)
    return np.where(ret, best, 0.0), np.where(ret, bid, -1), np.where(ret, bcos, 0.0)


def column_poses64(P0, P1, A):
    """(A,4,4): the world pose P0 D(s_c) of every column"""
    D = delta64(P0, P1)
    w = log64(D[:3, :3])
    out = np.zeros((A, 4, 4))
    for c in range(A):
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = exp64(w, c / A), (c / A) * D[:3, 3]
        out[c] = P0 @ M
    return out


def cast64_sweep(params, kind, z0, P0, P1, dirs, A, min_range, max_range, sensor_dirs=None):
    """every ray from the world pose of its column (ray r: column r % A).  sensor_dirs: float64 directions in the sensor
    frame to cast instead of the table's (the tilted ones of `ambiguous_sweep`)"""
    d = np.asarray(dirs).astype(np.float64) if sensor_dirs is None else sensor_dirs
    poses = column_poses64(P0, P1, A)
    world = np.empty_like(d)
    for c in range(A):                               # as cast64 turns a frame's rays: d @ R^T
        world[c::A] = d[c::A] @ poses[c, :3, :3].T
    return cast64_rays(params, kind, z0, poses[np.arange(d.shape[0]) % A, :3, 3], world, min_range, max_range)


def ambiguous_sweep(params, kind, z0, P0, P1, dirs, A, min_range, max_range, prim64):
    """lidar_sim_restated.ambiguous's tilt rule applied at every column's pose"""
    out = np.zeros(len(prim64), bool)
    for d in RS.tilted(dirs):
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        out |= cast64_sweep(params, kind, z0, P0, P1, dirs, A, min_range, max_range, sensor_dirs=d)[1] != prim64
    return out


# ------------------------------------------------------------------------------------------------------------
# deskew, float64
# ------------------------------------------------------------------------------------------------------------
def deskew64(xyz, s, D, s_ref):
    """xyz (n,3), s (n,) sweep fractions, D (4,4) -> D(s_ref)^-1 D(s) p, (n,3) float64"""
    p = np.asarray(xyz, np.float64)
    s = np.asarray(s, np.float64)
    w = log64(D[:3, :3])
    at_s = np.einsum("nij,nj->ni", exp64(w, s), p) + s[:, None] * D[:3, 3][None, :]
    ref = motion64(D, float(s_ref))
    return (at_s - ref[:3, 3]) @ ref[:3, :3]          # R_ref^T (q - t_ref), row vectors


def column_fraction(idx, A):
    return (np.asarray(idx) % A).astype(np.float64) / A


def azimuth_column32(xyz, A):
    """the kernel's time_mode 1 with azimuth_steps = A in float32: the nearest column of every point's azimuth"""
    p = np.asarray(xyz)
    assert p.dtype == f32
    u = np.arctan2(p[:, 1], p[:, 0]).astype(f32) * f32(0.15915494309189535)
    u = np.where(u < 0, u + f32(1), u).astype(f32)
    c = np.rint(u * f32(A))
    return np.where(c >= A, 0, c).astype(np.int64)
