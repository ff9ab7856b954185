"""The batched ICP of csrc/icp.hip restated in numpy, runnable in float32 and float64: transform, exhaustive nearest
neighbour with ties to the smaller index, radius cut, Gauss-Newton rows, fp64 Cholesky solve with the pivot test,
exponential-map update, stop rule, status codes.  This restatement is the yardstick of tests/test_gpu_icp.py: the reference
has no ICP (its refined_SE3.pkl was made offline by a third-party one), so there is no golden file to compare against.
The Gauss-Newton part (csrc/gn_solve.h: weights, system, system_floor, solve, update, iterate) also serves the restatements of
the registration against the local map (tests/lidar_odometry_restated.py, tests/lidar_plane_restated.py).

`dtype` is the precision of everything up to the summed system (transform, distances, rows, sums); the solve and the pose
are float64 in both, as on the GPU.  Also here: the synthetic room scenes the tests register.
"""
import numpy as np

POINT, PLANE = 0, 1
CONVERGED, MAX_ITER, NO_MATCH, SINGULAR = 0, 1, 2, 3
PIV_EPS = 1e-9
NSUM = 29


# ---------------------------------------------------------------------------------------------------------------- algorithm
def transform(pose, src, dtype):
    """pose (4,4) float64, src (n,3) -> (n,3) dtype: R p + t, the pose rounded to dtype first.  In float32 the kernel's own
    chain fma(R2, z, fma(R1, y, R0 * x)) + t: a float32 product is exact in float64, so rounding product + addend from
    float64 is the fused operation (up to a double rounding that needs a float64-inexact sum on a float32 tie)."""
    M = pose.astype(dtype)
    s = src.astype(dtype)
    if dtype == np.float32:
        M64, s64 = M.astype(np.float64), s.astype(np.float64)
        a = (M[None, :3, 0] * s[:, 0:1]).astype(np.float32)
        a = (M64[None, :3, 1] * s64[:, 1:2] + a.astype(np.float64)).astype(np.float32)
        a = (M64[None, :3, 2] * s64[:, 2:3] + a.astype(np.float64)).astype(np.float32)
        return a + M[None, :3, 3]
    return ((M[None, :3, 0] * s[:, 0:1] + M[None, :3, 1] * s[:, 1:2]) + M[None, :3, 2] * s[:, 2:3]) + M[None, :3, 3]


def nearest(q, tgt, dtype, chunk=512, exhaustive=False):
    """per query the index of the nearest target (smallest (distance, index)), its squared distance and the second-smallest
    squared distance; d = (dx*dx + dy*dy) + dz*dz in dtype.  Exhaustive, or -- the same answer, faster -- over the 8
    candidates a cKDTree finds nearest in float64: another point wins in dtype only if nine lie within rounding of the best."""
    t = tgt.astype(dtype)
    n = q.shape[0]
    idx = np.zeros(n, np.int64)
    d1 = np.full(n, np.inf, dtype)
    d2 = np.full(n, np.inf, dtype)
    if t.shape[0] == 0 or n == 0:
        return idx - 1, d1, d2
    if not exhaustive and t.shape[0] > 8 and np.isfinite(q).all():
        from scipy.spatial import cKDTree
        _, cand = cKDTree(t.astype(np.float64)).query(q.astype(np.float64), k=8)
        cand = np.sort(cand, axis=1)   # ascending index: argmin's first minimum is the smaller index
        c = t[cand]
        qq = q.astype(dtype)
        dx, dy, dz = qq[:, None, 0] - c[:, :, 0], qq[:, None, 1] - c[:, :, 1], qq[:, None, 2] - c[:, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        i = np.argmin(d, axis=1)
        rows_ = np.arange(n)
        idx, d1 = cand[rows_, i], d[rows_, i].copy()
        d[rows_, i] = np.inf
        return idx, d1, d.min(axis=1)
    for a in range(0, n, chunk):
        qq = q[a:a + chunk].astype(dtype)
        dx = qq[:, None, 0] - t[None, :, 0]
        dy = qq[:, None, 1] - t[None, :, 1]
        dz = qq[:, None, 2] - t[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        i = np.argmin(d, axis=1)   # first minimum = smaller index
        rows = np.arange(d.shape[0])
        idx[a:a + chunk], d1[a:a + chunk] = i, d[rows, i]
        if t.shape[0] > 1:
            d[rows, i] = np.inf
            d2[a:a + chunk] = d.min(axis=1)
    return idx, d1, d2


def match(pose, src, tgt, max_dist, dtype):
    """-> (transformed source (n,3) dtype, winning index or -1 (n,), best and second-best squared distance)"""
    q = transform(pose, src, dtype)
    idx, d1, d2 = nearest(q, tgt, dtype)
    r2 = np.float32(max_dist * max_dist).astype(dtype)   # the kernel compares against the float32 of max_dist^2
    hit = d1 <= r2
    return q, np.where(hit, idx, -1), d1, d2


def rows(q, win, tgt, normals, metric, dtype):
    """Jacobian rows J (m,6) and residuals e (m,) of the matched queries, in query order"""
    k = win >= 0
    p = q[k].astype(dtype)
    t = tgt[win[k]].astype(dtype)
    r = p - t
    z, o = np.zeros(len(p), dtype), np.ones(len(p), dtype)
    if metric == PLANE:
        n = normals[win[k]].astype(dtype)
        J = np.stack([p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2],
                      p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]], axis=1)
        e = (n[:, 0] * r[:, 0] + n[:, 1] * r[:, 1]) + n[:, 2] * r[:, 2]
        return J, e
    Jx = np.stack([z, p[:, 2], -p[:, 1], o, z, z], axis=1)
    Jy = np.stack([-p[:, 2], z, p[:, 0], z, o, z], axis=1)
    Jz = np.stack([p[:, 1], -p[:, 0], z, z, z, o], axis=1)
    return np.concatenate([Jx, Jy, Jz]), np.concatenate([r[:, 0], r[:, 1], r[:, 2]])


IU = np.triu_indices(6)


def weights(E, kernel_scale, dtype):
    """E (m,) squared residuals of the matches -> Geman-McClure w = (k / (k + E))^2 with k = kernel_scale^2; 0: ones"""
    if not kernel_scale > 0:
        return np.ones(len(E), dtype)
    k = dtype(kernel_scale * kernel_scale)
    r = k / (k + E)
    return (r * r).astype(dtype)


def system(J, e, count, dtype, w=None):
    """the 29 sums: H upper triangle row-major (21), g (6), matches, squared residuals -- summed in dtype.  w (rows,): H and
    g weighted, the count and the squared residuals not"""
    wJ = J if w is None else w[:, None] * J
    H = (wJ[:, :, None] * J[:, None, :]).sum(axis=0, dtype=dtype)
    g = (wJ * e[:, None]).sum(axis=0, dtype=dtype)
    return np.concatenate([H[IU], g, [count], [(e * e).sum(dtype=dtype)]]).astype(np.float64)


def system_floor(J, e, delta, w=None, dw=None):
    """What an error of up to `delta` in every coordinate of the transformed source can move each sum by: the rotation
    entries of a row are linear in that point with coefficients of 1-norm <= 2, the residual moves by <= 2 delta.  With
    weights w (rows,) that this error moves by up to dw, a term w J J moves by w d(J J) + |J J| dw."""
    aJ, ae = np.abs(J).astype(np.float64), np.abs(e).astype(np.float64)
    dJ = np.zeros(6)
    dJ[:3] = 2 * delta
    H = aJ[:, :, None] * dJ[None, None, :] + aJ[:, None, :] * dJ[None, :, None]
    g = aJ * (2 * delta) + ae[:, None] * dJ[None, :]
    if w is not None:
        w = w.astype(np.float64)
        H = w[:, None, None] * H + dw[:, None, None] * aJ[:, :, None] * aJ[:, None, :]
        g = w[:, None] * g + dw[:, None] * aJ * ae[:, None]
    return np.concatenate([H.sum(axis=0)[IU], g.sum(axis=0), [0.0], [(2 * ae * 2 * delta).sum()]])


def solve(S):
    """S (29,) float64 -> (x (6,) or None, status or None): H x = -g by Cholesky with the kernel's pivot test"""
    cnt = S[27]
    if not cnt >= 1:
        return None, NO_MATCH
    H = np.zeros((6, 6))
    H[IU] = S[:21]
    H = H + np.triu(H, 1).T
    g = S[21:27]
    if cnt < 6 or not np.all(np.isfinite(S)):
        return None, SINGULAR
    bm = (max(H[0, 0], H[1, 1], H[2, 2]), max(H[3, 3], H[4, 4], H[5, 5]))
    L = np.zeros((6, 6))
    for k in range(6):
        d = H[k, k] - np.dot(L[k, :k], L[k, :k])
        if not d > PIV_EPS * bm[k // 3]:
            return None, SINGULAR
        L[k, k] = np.sqrt(d)
        for i in range(k + 1, 6):
            L[i, k] = (H[i, k] - np.dot(L[i, :k], L[k, :k])) / L[k, k]
    y = np.zeros(6)
    for i in range(6):
        y[i] = (-g[i] - np.dot(L[i, :i], y[:i])) / L[i, i]
    x = np.zeros(6)
    for i in range(5, -1, -1):
        x[i] = (y[i] - np.dot(L[i + 1:, i], x[i + 1:])) / L[i, i]
    if not np.all(np.isfinite(x)):
        return None, SINGULAR
    return x, None


def exp_rot(w):
    th2 = float(np.dot(w, w))
    th = np.sqrt(th2)
    a, b = (1.0, 0.5) if th < 1e-8 else (np.sin(th) / th, (1.0 - np.cos(th)) / th2)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + a * K + b * (K @ K)


def update(pose, x):
    """[exp(w) | v] composed onto the pose"""
    out = np.eye(4)
    E = exp_rot(x[:3])
    out[:3, :3] = E @ pose[:3, :3]
    out[:3, 3] = E @ pose[:3, 3] + x[3:]
    return out


def _shifted(pose, origin, sign):
    """the pose with sign * origin added to its translation, float64; origin None: the pose itself"""
    if origin is None:
        return pose
    P = np.array(pose, np.float64)
    P[:3, 3] += sign * np.asarray(origin, np.float64)
    return P


def iterate(system_of, n_src, init, schedule, tol_rot=1e-7, tol_trans=1e-6, origin=None):
    """The loop of every registration over schedule = [(max_dist, max_iter), ...] -> dict(pose, fitness, rmse, iterations,
    status).  system_of(pose, max_dist) -> S (29,) is the search and the rows; its pose, and the step, are in the frame
    shifted by -origin (the local map's frame), the pose kept is the world's."""
    pose = np.array(init, np.float64)
    fitness = rmse = 0.0
    iterations, status = 0, MAX_ITER
    for max_dist, max_iter in schedule:
        status = MAX_ITER
        for _ in range(max_iter):
            local = _shifted(pose, origin, -1)
            S = system_of(local, max_dist)
            x, bad = solve(S)
            if bad == NO_MATCH:
                fitness, rmse, status = 0.0, 0.0, NO_MATCH
                break
            fitness, rmse = S[27] / max(n_src, 1), float(np.sqrt(S[28] / S[27]))
            if bad is not None:
                status = bad
                break
            pose = _shifted(update(local, x), origin, 1)
            iterations += 1
            if np.linalg.norm(x[:3]) < tol_rot and np.linalg.norm(x[3:]) < tol_trans:
                status = CONVERGED
                break
    return dict(pose=pose, fitness=fitness, rmse=rmse, iterations=iterations, status=status)


def icp(src, tgt, normals, init, max_dist=1.0, max_iter=30, metric=PLANE, tol_rot=1e-7, tol_trans=1e-6, dtype=np.float64):
    """-> dict(pose, fitness, rmse, iterations, status)"""
    def system_of(pose, max_dist):
        q, win, _, _ = match(pose, src, tgt, max_dist, dtype)
        J, e = rows(q, win, tgt, normals, metric, dtype)
        return system(J, e, int((win >= 0).sum()), dtype)
    return iterate(system_of, len(src), init, [(max_dist, max_iter)], tol_rot, tol_trans)


# ------------------------------------------------------------------------------------------------------------------- scenes
ROOM = (40.0, 30.0, 6.0)


def room(n, seed, noise=0.0):
    """(n,3) float64: a closed room of 40 x 30 x 6 m centred on the origin's xy, half the points on the floor, half on the
    four walls; optional Gaussian noise"""
    rng = np.random.default_rng(seed)
    lx, ly, lz = ROOM
    nf = n // 2
    floor = np.stack([rng.uniform(-lx / 2, lx / 2, nf), rng.uniform(-ly / 2, ly / 2, nf), np.zeros(nf)], axis=1)
    nw = n - nf
    side = rng.integers(0, 4, nw)
    u, z = rng.uniform(0, 1, nw), rng.uniform(0, lz, nw)
    x = np.where(side == 0, -lx / 2, np.where(side == 1, lx / 2, (u - 0.5) * lx))
    y = np.where(side == 2, -ly / 2, np.where(side == 3, ly / 2, (u - 0.5) * ly))
    pts = np.concatenate([floor, np.stack([x, y, z], axis=1)])
    if noise > 0:
        pts = pts + rng.normal(0.0, noise, pts.shape)
    return pts[rng.permutation(n)]


def se3(rotvec, t):
    M = np.eye(4)
    M[:3, :3] = exp_rot(np.asarray(rotvec, np.float64))
    M[:3, 3] = t
    return M


def moved(points, pose):
    """the points as seen from a frame whose pose in the points' frame is `pose`: pose^-1 applied, float32"""
    R, t = pose[:3, :3], pose[:3, 3]
    return ((points - t) @ R).astype(np.float32)


def exact_source(target, n1, pose, seed):
    """a random subset of the (float32) target moved by a known pose: registering it onto the target gives `pose` back up to
    the float32 rounding of the moved coordinates"""
    rng = np.random.default_rng(seed)
    pick = rng.choice(len(target), n1, replace=False)
    return moved(target[pick].astype(np.float64), pose)


def perturbed(pose, seed, trans=0.2, deg=1.0):
    """pose composed with an error of `trans` metres and `deg` degrees in seeded random directions"""
    rng = np.random.default_rng(seed)
    a, d = rng.normal(size=3), rng.normal(size=3)
    return se3(a / np.linalg.norm(a) * np.radians(deg), d / np.linalg.norm(d) * trans) @ pose
