"""The voxel planes, the point-to-plane rows and the adaptive gate of the geometric odometry restated in numpy, written from
the contract (include/dpm_hip.h: dpm_local_map_planes, dpm_local_map_register_planes).  It extends
tests/lidar_odometry_restated.py, whose map, search and solve it uses, and is the yardstick of
tests/test_gpu_local_map_planes.py and tests/test_gpu_lidar_odometry_plane.py.

`planes(..., np.float32)` mirrors the kernel: the fp32 centre, difference and membership test, the fp64 cumulants of the fp32
differences, the scatter matrix n S_ab - S_a S_b and the same cyclic Jacobi.  `planes(..., np.float64)` is the independent
form: nothing is rounded to fp32 before the normal, the covariance is formed about the mean in a second pass, and the
eigenvectors come from numpy.linalg.eigh.  Both end alike: the normal rounded to fp32, the sign rule on the fp32 values,
w = max(l0, 0) / l1 rounded to fp32.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restated as I  # noqa: E402
import lidar_odometry_restated as L  # noqa: E402

CONVERGED, MAX_ITER, NO_MATCH, SINGULAR = L.CONVERGED, L.MAX_ITER, L.NO_MATCH, L.SINGULAR
LINE_RATIO = 1e-8   # l1 <= LINE_RATIO l2: a line to the precision fp32 coordinates have -- no plane (include/dpm_hip.h)


# --------------------------------------------------------------------------------------------------------------------- planes
def members(exported, voxel, plane_radius, dtype):
    """-> (ukeys (V,) the held voxels ascending, vi, pi, d): point pi of the export is a member of voxel vi with d = p - c in
    dtype, ordered by (voxel, neighbour number, sub-cell) -- the kernel's order of summation up to its four-lane tree"""
    keys, sub, _, xyz = exported
    ukeys = np.unique(keys)
    if len(ukeys) == 0:
        return ukeys, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 3), dtype)
    pv = L.unpack_key(keys)
    vi, pi, nn = [], [], []
    for nb in range(27):
        off = np.array([nb % 3 - 1, (nb // 3) % 3 - 1, nb // 9 - 1])
        u = pv - off                                         # the voxel that has this point's voxel as neighbour nb
        ok = np.all((u >= -L.BIAS) & (u < L.BIAS), axis=1)
        k = L.pack_key(np.where(ok[:, None], u, 0))
        pos = np.minimum(np.searchsorted(ukeys, k), len(ukeys) - 1)
        ok &= ukeys[pos] == k
        vi.append(pos[ok]), pi.append(np.nonzero(ok)[0]), nn.append(np.full(int(ok.sum()), nb))
    vi, pi, nn = np.concatenate(vi), np.concatenate(pi), np.concatenate(nn)
    order = np.lexsort((sub[pi], nn, vi))
    vi, pi = vi[order], pi[order]
    idx = L.unpack_key(ukeys)[vi]
    if dtype == np.float32:
        c = ((idx.astype(np.float32) + np.float32(0.5)) * np.float32(voxel)).astype(np.float32)
        d = (xyz[pi].astype(np.float32) - c).astype(np.float32)
        r2 = np.float32(plane_radius * plane_radius)
    else:
        d = xyz[pi].astype(np.float64) - (idx + 0.5) * float(voxel)
        r2 = plane_radius * plane_radius
    inside = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= r2
    return ukeys, vi[inside], pi[inside], d[inside]


def jacobi(A):
    """csrc/sym3_jacobi.h's sym3_jacobi on a batch (V,3,3) float64 -> (eigenvalues (V,3) = the diagonal, eigenvectors in columns)"""
    A = A.copy()
    V = np.broadcast_to(np.eye(3), A.shape).copy()
    live = np.ones(len(A), bool)
    for _ in range(12):
        off = np.abs(A[:, 0, 1]) + np.abs(A[:, 0, 2]) + np.abs(A[:, 1, 2])
        live &= ~((off <= 1e-300) | (off <= 1e-18 * (np.abs(A[:, 0, 0]) + np.abs(A[:, 1, 1]) + np.abs(A[:, 2, 2]))))
        if not live.any():
            break
        for p in range(2):
            for r in range(p + 1, 3):
                m = np.nonzero(live & (A[:, p, r] != 0.0))[0]
                if len(m) == 0:
                    continue
                theta = (A[m, r, r] - A[m, p, p]) / (2.0 * A[m, p, r])
                t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                cs = 1.0 / np.sqrt(t * t + 1.0)
                sn = t * cs
                cs, sn = cs[:, None], sn[:, None]
                akp, akr = A[m, :, p].copy(), A[m, :, r].copy()
                A[m, :, p], A[m, :, r] = cs * akp - sn * akr, sn * akp + cs * akr
                apk, ark = A[m, p, :].copy(), A[m, r, :].copy()
                A[m, p, :], A[m, r, :] = cs * apk - sn * ark, sn * apk + cs * ark
                vkp, vkr = V[m, :, p].copy(), V[m, :, r].copy()
                V[m, :, p], V[m, :, r] = cs * vkp - sn * vkr, sn * vkp + cs * vkr
    return np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], axis=1), V


def finish(lam, vec, counts):
    """eigenvalues (V,3) in any order with eigenvectors in the columns of vec (V,3,3) -> normal (V,3) float32, w (V,) float32,
    gap (V,) = (l1 - l0) / l2: ascending order with the smaller axis first among equals, the unit eigenvector of the smallest
    rounded to fp32, the sign rule on the fp32 values, w = max(l0, 0) / l1; (0,0,0,-1) below three points or for a line, l1 <= LINE_RATIO l2 (which includes l1 <= 0)"""
    n = len(lam)
    order = np.argsort(lam, axis=1, kind="stable")
    rows = np.arange(n)
    l0, l1, l2 = (lam[rows, order[:, k]] for k in range(3))
    v = vec[rows, :, order[:, 0]]
    with np.errstate(invalid="ignore", divide="ignore"):
        nr = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        ok = (counts >= 3) & (l1 > LINE_RATIO * l2) & (nr > 0)
        unit = np.where(ok[:, None], v / np.where(nr > 0, nr, 1.0)[:, None], 0.0).astype(np.float32)
        a = np.abs(unit)
        lead = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), unit[:, 0], np.where(a[:, 1] >= a[:, 2], unit[:, 1], unit[:, 2]))
        sign = np.where(lead < 0, np.float32(-1), np.float32(1))
        normal = (sign[:, None] * unit + np.float32(0)).astype(np.float32)
        w = np.where(ok, np.maximum(l0, 0.0) / np.where(l1 > 0, l1, 1.0), -1.0).astype(np.float32)
        gap = np.where(ok & (l2 > 0), (l1 - l0) / np.where(l2 > 0, l2, 1.0), 0.0)
    return normal, w, gap


def planes(exported, voxel, plane_radius, dtype):
    """the plane of every held voxel of an exported map -> namespace(keys (V,) ascending, counts (V,) int32, normal (V,3)
    float32, w (V,) float32, gap (V,) float64)"""
    ukeys, vi, pi, d = members(exported, voxel, plane_radius, dtype)
    V = len(ukeys)
    counts = np.bincount(vi, minlength=V).astype(np.int32)
    d = d.astype(np.float64)
    if dtype == np.float32:
        n = counts.astype(np.float64)
        S1 = np.zeros((V, 3))
        S2 = np.zeros((V, 3, 3))
        np.add.at(S1, vi, d)
        np.add.at(S2, vi, d[:, :, None] * d[:, None, :])
        A = n[:, None, None] * S2 - S1[:, :, None] * S1[:, None, :]
        lam, vec = jacobi(A)
    else:
        mean = np.zeros((V, 3))
        np.add.at(mean, vi, d)
        mean /= np.maximum(counts, 1)[:, None]
        r = d - mean[vi]
        C = np.zeros((V, 3, 3))
        np.add.at(C, vi, r[:, :, None] * r[:, None, :])
        C /= np.maximum(counts, 1)[:, None, None]
        lam, vec = np.linalg.eigh(C)
    normal, w, gap = finish(lam, vec, counts)
    return SimpleNamespace(keys=ukeys, counts=counts, normal=normal, w=w, gap=gap)


def angle(a, b):
    """the angle between unit vectors (n,3), exact for small ones: 2 atan2(|a - b|, |a + b|)"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    return 2 * np.arctan2(np.linalg.norm(a - b, axis=1), np.linalg.norm(a + b, axis=1))


# ----------------------------------------------------------------------------------------------------------------------- rows
def gate(counts, w, min_points=5, max_ratio=0.1):
    """which voxels give rows: counts >= min_points and 0 <= w <= (float)max_ratio"""
    return (counts >= min_points) & (w >= 0) & (w <= np.float32(max_ratio))


def per_row(exported, P, min_points=5, max_ratio=0.1):
    """the plane of every export row's voxel: normals (n,3) float32 and whether it gives rows (n,)"""
    at = np.searchsorted(P.keys, exported[0])
    return P.normal[at], gate(P.counts, P.w, min_points, max_ratio)[at]


def system(q, win, xyz, normals, rows_ok, kernel_scale, dtype):
    """the 29 sums of the plane rows on given matches (-1: none); a match whose voxel gives no row drops out, count included.
    -> S, J, e, w and the matches that gave rows"""
    win = np.where((win >= 0) & rows_ok[np.maximum(win, 0)], win, -1)
    J, e = I.rows(q, win, xyz, normals, I.PLANE, dtype)
    w = I.weights(e * e, kernel_scale, dtype)
    return I.system(J, e, int((win >= 0).sum()), dtype, w), J, e, w, win


def system_floor(J, e, w, kernel_scale, delta):
    """icp_restated.system_floor with the weights of plane rows.  The rotation entries p x n are linear in the point with
    coefficients of 1-norm <= 2 (|n| = 1), the entries n do not move, the residual n.(p - q) moves by <= 2 delta; with
    E = e e, |dE| <= 2 |e| 2 delta and dw <= 2 w / (k + E) dE."""
    ae, w = np.abs(e).astype(np.float64), w.astype(np.float64)
    dw = np.zeros(len(e))
    if kernel_scale > 0:
        k = kernel_scale * kernel_scale
        dw = 2 * w / (k + ae * ae) * (2 * ae * 2 * delta)
    return I.system_floor(J, e, delta, w, dw)


# --------------------------------------------------------------------------------------------------------------- registration
def register(src, exported, voxel, s, origin, init, schedule, kernel_scale=0.0, tol_rot=1e-7, tol_trans=1e-6,
             dtype=np.float64, metric="point", plane_radius=None, min_points=5, max_ratio=0.1, P=None):
    """lidar_odometry_restated.register with metric "point" (that very function) or "plane": rows on the planes P (default:
    planes(exported, voxel, plane_radius or 1.5 voxel, dtype))"""
    if metric == "point":
        return L.register(src, exported, voxel, s, origin, init, schedule, kernel_scale, tol_rot, tol_trans, dtype)
    assert metric == "plane", metric
    from scipy.spatial import cKDTree
    xyz = exported[3]
    if len(xyz):
        P = planes(exported, voxel, 1.5 * voxel if plane_radius is None else plane_radius, dtype) if P is None else P
        normals, rows_ok = per_row(exported, P, min_points, max_ratio)
    else:
        normals, rows_ok = np.zeros((0, 3), np.float32), np.zeros(0, bool)
    extra = dict(tree=cKDTree(xyz.astype(np.float64))) if len(xyz) else {}

    def system_of(pose, max_dist):
        q = I.transform(pose, src, dtype)
        win = L.search_fast(q, exported, voxel, s, max_dist, dtype, **extra)
        return system(q, win, xyz, normals, rows_ok, kernel_scale, dtype)[0]
    return I.iterate(system_of, len(src), init, schedule, tol_rot, tol_trans, origin)


# -------------------------------------------------------------------------------------------------------------- adaptive gate
def deviation(pred, pose, max_range):
    """|t| + 2 max_range sin(theta / 2) of pred^-1 pose"""
    D = np.linalg.inv(pred) @ pose
    R = D[:3, :3]
    theta = np.arctan2(np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2, (np.trace(R) - 1) / 2)
    return float(np.linalg.norm(D[:3, 3]) + 2 * max_range * np.sin(theta / 2))


def sigma_of(deviations, sigma0, min_motion):
    d = np.array([x for x in deviations if x > min_motion], np.float64)
    return float(sigma0) if len(d) == 0 else float(np.sqrt(np.mean(d * d)))


def gates_of(poses, statuses, sigma0, min_motion, max_range, voxel, max_iter, first_motion=None):
    """the (max_dist, max_iter, kernel_scale) every step after the first must have used, from the poses a run returned"""
    out, dev = [], []
    for k in range(1, len(poses)):
        sg = sigma_of(dev, sigma0, min_motion)
        out.append((min(3 * sg, float(np.float32(voxel))), max_iter, sg / 3))
        motion = np.linalg.inv(poses[k - 2]) @ poses[k - 1] if k >= 2 else (np.eye(4) if first_motion is None else first_motion)
        if statuses[k] in (CONVERGED, MAX_ITER):
            dev.append(deviation(poses[k - 1] @ motion, poses[k], max_range))
    return out


def odometry(frames, voxel=1.0, subdiv=3, max_range=100.0, min_range=0.0, schedule=((1.0, 30),), kernel_scale=0.0,
             first_pose=None, dtype=np.float64, tol_rot=1e-7, tol_trans=1e-6, initial_motion=None, metric="point",
             plane_radius=None, min_points=5, max_ratio=0.1, adaptive=None):
    """lidar_odometry_restated.odometry with the metric and the adaptive gate.  The pose kept after a registration is the
    registered one with its rotation block replaced by the nearest rotation, as deeppointmap_amd/odometry.py keeps it (the
    map is filled under the registered pose itself)."""
    poses, statuses, dev = [], [], []
    m = None
    for k, xyz in enumerate(frames):
        xyz = np.asarray(xyz, np.float32)
        if k == 0:
            P = np.eye(4) if first_pose is None else np.array(first_pose, np.float64)
            m = L.Map(voxel, subdiv, P[:3, 3].copy(), min_range, max_range, dtype)
            status, put = CONVERGED, P
        else:
            motion = np.linalg.inv(poses[-2]) @ poses[-1] if k >= 2 else (np.eye(4) if initial_motion is None else initial_motion)
            pred = poses[-1] @ motion
            stages, scale = schedule, kernel_scale
            if adaptive is not None:
                sg = sigma_of(dev, *adaptive)
                stages, scale = [(min(3 * sg, float(np.float32(voxel))), schedule[-1][1])], sg / 3
            r = register(xyz, m.export(), m.voxel, m.s, m.origin, pred, stages, scale, tol_rot, tol_trans, dtype, metric,
                         plane_radius, min_points, max_ratio)
            status = r["status"]
            put = P = r["pose"] if status in (CONVERGED, MAX_ITER) else pred
            if status in (CONVERGED, MAX_ITER):
                U, _, Vt = np.linalg.svd(P[:3, :3])
                P = P.copy()
                P[:3, :3] = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt
                dev.append(deviation(pred, P, max_range))
        if status in (CONVERGED, MAX_ITER):
            m.insert(xyz, np.arange(len(xyz)), put, k)
            m.prune(put, max_range)
        poses.append(P)
        statuses.append(status)
    return np.stack(poses), statuses, m


# --------------------------------------------------------------------------------------------------------------------- scenes
def sliding_scene(beams=16, columns=256, height=1.8, wall_x=12.0, wall_y=9.0, max_range=60.0):
    """The case point-to-plane rows are for: a sensor `height` over the ground z = 0 with the walls x = wall_x and y = wall_y,
    `beams` x `columns` rays.  Frame 0 is taken at the origin, frame 1 0.5 m on along x and turned by 1 degree.  Most returns
    are ground rings, which travel with the sensor.  -> (frame 0, frame 1 (n,3) float32 sensor frame, pose 0, pose 1)"""
    el = np.radians(np.linspace(8.0, -22.0, beams))
    az = np.arange(columns) * (2 * np.pi / columns)
    e, a = [g.ravel() for g in np.meshgrid(el, az, indexing="ij")]
    rays = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], axis=1)
    P0 = I.se3([0, 0, 0], [0, 0, height])
    P1 = I.se3([0, 0, np.radians(1.0)], [0.5, 0, height])
    frames = []
    for P in (P0, P1):
        d = rays @ P[:3, :3].T
        o = P[:3, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.stack([np.where(d[:, 2] < 0, -o[2] / d[:, 2], np.inf), np.where(d[:, 0] > 0, (wall_x - o[0]) / d[:, 0], np.inf),
                          np.where(d[:, 1] > 0, (wall_y - o[1]) / d[:, 1], np.inf)], axis=1).min(axis=1)
        hit = t <= max_range
        frames.append((rays[hit] * t[hit, None]).astype(np.float32))
    return frames[0], frames[1], P0, P1


def sliding_case(metric, dtype=np.float64, kernel_scale=0.1):
    """frame 1 of sliding_scene registered from the pose of frame 0 against the map of frame 0 (voxel = max_dist = 1 m, 27
    sub-cells) -> (the registration's result, its translation error in metres against the exact pose)"""
    f0, f1, P0, P1 = sliding_scene()
    m = L.Map(1.0, 3, (0.0, 0.0, 0.0), 0.0, 100.0, dtype)
    m.insert(f0, np.arange(len(f0)), P0, 0)
    r = register(f1, m.export(), m.voxel, 3, m.origin, P0, [(1.0, 50)], kernel_scale, dtype=dtype, metric=metric)
    return r, float(np.linalg.norm(r["pose"][:3, 3] - P1[:3, 3]))


def plane_lattice(axis, at, n_side=9, spacing=0.25, centre=(0.0, 0.0, 0.0)):
    """n_side^2 lattice points of `spacing` on the plane coordinate[axis] = at around `centre`, float32"""
    a = (np.arange(n_side) - (n_side - 1) / 2) * spacing
    u, v = [g.ravel() for g in np.meshgrid(a, a, indexing="ij")]
    cols = [u, v]
    cols.insert(axis, np.zeros_like(u))
    pts = np.stack(cols, axis=1) + np.asarray(centre, np.float64)
    pts[:, axis] = at
    return pts.astype(np.float32)


def normals_scene(seed=3, n=1400):
    """a scene for the comparison of normals: a room's floor and walls with 5 mm of noise, seen as one frame"""
    return I.room(n, seed=seed, noise=0.005).astype(np.float32) * np.float32(0.5)


def wall_line(n=9, start=(40.3, 30.1, 1.7), step=(0.11, 0.05, 0.0)):
    """n points along a straight line far from the origin, as a ring of a spinning sensor draws them on a flat wall: in exact
    arithmetic l1 = 0; rounded to float32 the points are a few micrometres off the line, and an eigenvector of that is noise"""
    return (np.asarray(start)[None, :] + np.arange(n)[:, None] * np.asarray(step)[None, :]).astype(np.float32)

