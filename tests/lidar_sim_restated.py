"""The LiDAR simulator in numpy, written from the contract (include/dpm_hip.h: dpm_lidar_cull / _cast / _emit and
deeppointmap_amd/lidar_sim.py's docstring).  Two forms:

* `simulate32`: the cull in float64 rounded to float32 and the cast in float32, every operation in the kernels' order
  (numpy rounds each float32 operation once and fuses nothing), so the kernels' outputs are expected bit for bit;
* `cast64`: an INDEPENDENT float64 cast in world coordinates over all primitives -- no cull, no sensor frame, the
  textbook quadratic for the cylinder (float64 has the headroom) -- that answers "is the float32 path right".

Both take the float32 direction table, converted exactly, so they cast the very same rays.

`ambiguous` marks the rays whose float64 primitive id changes under a tilt of 1e-5 rad in azimuth or elevation: rays
through an edge or a silhouette, where float32 and float64 may legitimately disagree about WHICH surface is hit.
"""
import numpy as np

f32 = np.float32
INF32 = f32(np.inf)
TILT = 1e-5
REC = 16


# ------------------------------------------------------------------------------------------------------------
# cull (float64 -> float32 records)
# ------------------------------------------------------------------------------------------------------------
def cull(prims, kind, ground, pose, max_range):
    """-> (rec (K,15) float32, ids (K,) int, kinds (K,) int, plane (4,) float32): the kept records of one frame in ascending
    primitive index"""
    prims = np.asarray(prims, np.float64).reshape(-1, 10)
    R, t = pose[:3, :3], pose[:3, 3]
    ex, ey, ez = t[0] - prims[:, 0], t[1] - prims[:, 1], t[2] - prims[:, 2]
    sz, reach = ez - prims[:, 8], max_range + prims[:, 9]
    keep = (ex * ex + ey * ey) + sz * sz <= reach * reach
    c, s = prims[:, 6], prims[:, 7]
    one = np.ones_like(c)
    cols = [c * ex + s * ey, c * ey - s * ex, ez,
            c * R[0, 0] + s * R[1, 0], c * R[0, 1] + s * R[1, 1], c * R[0, 2] + s * R[1, 2],
            c * R[1, 0] - s * R[0, 0], c * R[1, 1] - s * R[0, 1], c * R[1, 2] - s * R[0, 2],
            one * R[2, 0], one * R[2, 1], one * R[2, 2], prims[:, 3], prims[:, 4], prims[:, 5]]
    rec = np.stack(cols, axis=1).astype(f32)[keep] if len(prims) else np.zeros((0, 15), f32)
    ids = np.nonzero(keep)[0]
    if ground[1] != 0.0:
        plane = np.array([R[2, 0], R[2, 1], R[2, 2], ground[0] - t[2]], np.float64).astype(f32)
    else:
        plane = np.zeros(4, f32)
    return rec, ids, np.asarray(kind)[ids], plane


def kept_counts(prims, kind, ground, poses, max_range):
    return [len(cull(prims, kind, ground, p, max_range)[1]) for p in poses]


# ------------------------------------------------------------------------------------------------------------
# cast, float32, the kernel's order of operations
# ------------------------------------------------------------------------------------------------------------
def _slab32(o, dd, lo, hi):
    with np.errstate(all="ignore"):
        t1, t2 = (lo - o) / dd, (hi - o) / dd
    zero = dd == 0
    first = t1 < t2
    tn = np.where(zero, -INF32, np.where(first, t1, t2))
    tf = np.where(zero, INF32, np.where(first, t2, t1))
    ok = np.where(zero, not (o < lo or o > hi), True)
    return ok, tn, tf


def cast32(rec, ids, kinds, plane, P, dirs, min_range, max_range):
    """one frame: rec / ids / kinds / plane from cull, dirs (rays,3) float32 -> range, prim, cos_inc (rays,)"""
    dirs = np.asarray(dirs)
    assert dirs.dtype == f32 and rec.dtype == f32
    d0, d1, d2 = dirs[:, 0], dirs[:, 1], dirs[:, 2]
    n = dirs.shape[0]
    best, bcos, bid = np.full(n, INF32, f32), np.zeros(n, f32), np.full(n, -1, np.int32)
    zero = f32(0)
    for q, pid, k in zip(rec, ids, kinds):
        ox, oy, oz = q[0], q[1], q[2]
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
            inside = bool(ox * ox + oy * oy <= rad * rad)
            hit = np.where(az, inside, ok)
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
        t = plane[3] / den
    upd = (den != 0) & (t > 0) & (t < best)
    best, bcos, bid = np.where(upd, t, best), np.where(upd, np.abs(den), bcos), np.where(upd, np.int32(P), bid)
    ret = (bid >= 0) & ~(best < f32(min_range)) & ~(best > f32(max_range))
    return (np.where(ret, best, zero).astype(f32), np.where(ret, bid, -1).astype(np.int32),
            np.where(ret, bcos, zero).astype(f32))


def simulate32(prims, kind, ground, poses, dirs, min_range, max_range, rays=None):
    """every frame: (range, prim, cos_inc) each (F,rays); rays: indices of a subsample of the rays to cast (default all)"""
    P = len(kind)
    d = np.asarray(dirs) if rays is None else np.asarray(dirs)[rays]
    out = [cast32(*cull(prims, kind, ground, p, max_range), P, d, min_range, max_range) for p in poses]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


# ------------------------------------------------------------------------------------------------------------
# cast, float64, world coordinates, independent formulas
# ------------------------------------------------------------------------------------------------------------
def _slab64(o, dd, lo, hi):
    with np.errstate(all="ignore"):
        t1, t2 = (lo - o) / dd, (hi - o) / dd
    zero = dd == 0
    tn = np.where(zero, -np.inf, np.minimum(t1, t2))
    tf = np.where(zero, np.inf, np.maximum(t1, t2))
    return np.where(zero, lo <= o <= hi, True), tn, tf


def cast64_dirs(params, kind, z0, origin, D, min_range, max_range):
    """params (P,7) float64 (Scene.params), kind (P,), z0 or None; origin (3,) and D (n,3) float64 unit directions in the
    WORLD -> range, prim, cos_inc (n,) float64 / int"""
    n = D.shape[0]
    best, bcos, bid = np.full(n, np.inf), np.zeros(n), np.full(n, -1, np.int64)
    for pid, (q, k) in enumerate(zip(params, kind)):
        rel = origin - q[:3]
        if k == 0:
            c, s = np.cos(q[6]), np.sin(q[6])
            o = np.array([c * rel[0] + s * rel[1], -s * rel[0] + c * rel[1], rel[2]])
            d = np.stack([c * D[:, 0] + s * D[:, 1], -s * D[:, 0] + c * D[:, 1], D[:, 2]], axis=1)
            slabs = [_slab64(o[a], d[:, a], -q[3 + a], q[3 + a]) for a in range(3)]
            hit = slabs[0][0] & slabs[1][0] & slabs[2][0]
            tn, tf = np.stack([s_[1] for s_ in slabs]), np.stack([s_[2] for s_ in slabs])
            ia, ix = np.argmax(tn, axis=0), np.argmin(tf, axis=0)
            enter, exit_ = tn.max(axis=0), tf.min(axis=0)
            ad = np.abs(d)
            cen, cex = ad[np.arange(n), ia], ad[np.arange(n), ix]
        else:
            r, H = q[3], q[4]
            A = D[:, 0] ** 2 + D[:, 1] ** 2
            B = rel[0] * D[:, 0] + rel[1] * D[:, 1]
            C = rel[0] ** 2 + rel[1] ** 2 - r * r
            with np.errstate(all="ignore"):
                disc = B * B - A * C
                ok = disc >= 0
                root = np.sqrt(np.where(ok, disc, 0.0))
                ns, fs = (-B - root) / A, (-B + root) / A
            vertical = A == 0
            hit = np.where(vertical, C <= 0, ok)
            ns, fs = np.where(vertical, -np.inf, ns), np.where(vertical, np.inf, fs)
            okz, nz, fz = _slab64(rel[2], D[:, 2], 0.0, H)
            hit = hit & okz
            enter, exit_ = np.maximum(ns, nz), np.minimum(fs, fz)
            side_in, side_out = ns >= nz, fs <= fz

            def side_cos(t):   # |normal . direction| from the hit point itself
                with np.errstate(all="ignore"):
                    px, py = rel[0] + t * D[:, 0], rel[1] + t * D[:, 1]
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
            t = (z0 - origin[2]) / D[:, 2]
        upd = (D[:, 2] != 0) & (t > 0) & (t < best)
        best, bcos, bid = np.where(upd, t, best), np.where(upd, np.abs(D[:, 2]), bcos), np.where(upd, len(kind), bid)
    ret = (bid >= 0) & (best >= min_range) & (best <= max_range)
    return np.where(ret, best, 0.0), np.where(ret, bid, -1), np.where(ret, bcos, 0.0)


def cast64(params, kind, z0, pose, dirs, min_range, max_range):
    d = np.asarray(dirs).astype(np.float64)        # exact
    return cast64_dirs(params, kind, z0, pose[:3, 3], d @ pose[:3, :3].T, min_range, max_range)


def tilted(dirs):
    """the four directions TILT rad off every ray: azimuth +-, elevation +- (float64, sensor frame, unit length)"""
    d = np.asarray(dirs).astype(np.float64)
    c, s = np.cos(TILT), np.sin(TILT)
    h = np.hypot(d[:, 0], d[:, 1])
    out = []
    for sg in (1.0, -1.0):      # a turn about the sensor's z axis
        out.append(np.stack([c * d[:, 0] - sg * s * d[:, 1], sg * s * d[:, 0] + c * d[:, 1], d[:, 2]], axis=1))
    for sg in (1.0, -1.0):      # a turn in the vertical plane through the ray
        h2, z2 = c * h - sg * s * d[:, 2], c * d[:, 2] + sg * s * h
        scale = np.where(h > 0, h2 / np.where(h > 0, h, 1.0), 0.0)
        x = np.where(h > 0, scale * d[:, 0], h2)        # a vertical ray tilts towards x
        out.append(np.stack([x, scale * d[:, 1], z2], axis=1))
    return out


def ambiguous(params, kind, z0, pose, dirs, min_range, max_range, prim64=None):
    """(rays,) bool: the float64 primitive id differs for one of the four tilted directions"""
    if prim64 is None:
        prim64 = cast64(params, kind, z0, pose, dirs, min_range, max_range)[1]
    out = np.zeros(len(prim64), bool)
    for d in tilted(dirs):
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        out |= cast64_dirs(params, kind, z0, pose[:3, 3], d @ pose[:3, :3].T, min_range, max_range)[1] != prim64
    return out


# ------------------------------------------------------------------------------------------------------------
# emit
# ------------------------------------------------------------------------------------------------------------
def emit(rng, prim, cos_inc, dirs, albedo, class_id, noise=None, u=None, drop_prob=0.0):
    """one frame: -> xyz (rays,3) float32 with the returns first in ray order and zeros after, idx (rays,) int32, count,
    intensity (rays,) float32, label (rays,) int32"""
    dirs = np.asarray(dirs)
    rays = dirs.shape[0]
    keep = prim >= 0
    if u is not None:
        keep &= u >= f32(drop_prob)
    t = rng if noise is None else rng + noise
    pts = (t[:, None] * dirs).astype(f32)
    xyz, idx = np.zeros((rays, 3), f32), np.zeros(rays, np.int32)
    n = int(keep.sum())
    xyz[:n], idx[:n] = pts[keep], np.nonzero(keep)[0]
    hit = prim >= 0
    safe = np.where(hit, prim, 0)
    intensity = np.where(hit, albedo[safe] * cos_inc, f32(0)).astype(f32)
    label = np.where(hit, class_id[safe], -1).astype(np.int32)
    return xyz, idx, n, intensity, label
