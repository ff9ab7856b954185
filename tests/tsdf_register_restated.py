"""The field at a point, the registration against it and the frame-to-model tracker of the TSDF map restated in numpy, written
from the contract (include/dpm_hip.h: dpm_tsdf_sample, dpm_tsdf_register) before the kernel was trusted.  The
yardstick of tests/test_gpu_tsdf_register.py, beside tests/tsdf_restated.py and tests/tsdf_plane_restated.py, whose exported
fields it reads.

  sample         the trilinear interpolant of a sorted (keys, D) field (tsdf_restated.field) between the 8 voxel centres round a
                 point, and its gradient.  float32: operation for operation what the kernel does (the fma chain of the transform,
                 the correctly rounded quotient, g - 0.5f, floor, the nested lerps, grad = h / v), so it equals dpm_tsdf_sample
                 bit for bit.  float64: independent -- world coordinates with the lattice hanging at `origin`, no map-frame
                 pose, the interpolant as the sum over the 8 corners of the product of the three one-dimensional weights and the
                 gradient as that sum's derivative.
  system         the 29 sums of the rows (and J, e, w, which rows gave): the gate in `dtype`, the rows in float64 of the
                 sampled values, as the kernel forms them.
  system_floor   what the rounding of the inputs can move each sum by (the pattern of icp_restated.system_floor).
  register       the loop over icp_restated.solve / update (icp_restated.iterate).
  tracker        TsdfTracker.step's rule over tsdf_plane_restated.FusedPlane / tsdf_restated.Fused.
MUTANTS, as arguments: anchor_floor (the cell anchored at the voxel's floor: no - 0.5), divide=False (the gradient not divided by
v), corners7 (a row given with 7 corners, the missing one read as 0), negate_rot (J's rotation part negated).
Also here: the scenes the tests register (three tilted patches, a box room).
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restated as I  # noqa: E402
import lidar_odometry_restated as L  # noqa: E402
import tsdf_plane_restated as TP  # noqa: E402
import tsdf_restated as R  # noqa: E402

F32 = np.float32
CONVERGED, MAX_ITER, NO_MATCH, SINGULAR = I.CONVERGED, I.MAX_ITER, I.NO_MATCH, I.SINGULAR
CELL_LO, CELL_HI = -1048576.0, 1048575.0     # fl >= CELL_LO and fl < CELL_HI: fl and fl + 1 fit the 21 bits
NEAR_FACE = 1e-5                             # voxels: a row nearer than this to a cell face may fall into either cell


# ---------------------------------------------------------------------------------------------------------------------- sample
def _corners(fld, idx, valid):
    """D (n,2,2,2) of the 8 voxels idx + (dx, dy, dz) of the sorted field, in the field's dtype, and which of them it holds"""
    keys, D = fld
    n = len(idx)
    val = np.zeros((n, 2, 2, 2), np.asarray(D).dtype)
    held = np.zeros((n, 2, 2, 2), bool)
    if len(keys) == 0:
        return val, held
    base = np.where(valid[:, None], idx, 0)
    for dx in range(2):
        for dy in range(2):
            for dz in range(2):
                key = L.pack_key(base + np.array([dx, dy, dz]))
                pos = np.minimum(np.searchsorted(keys, key), len(keys) - 1)
                hit = valid & (keys[pos] == key)
                held[:, dx, dy, dz] = hit
                val[:, dx, dy, dz] = np.where(hit, D[pos], 0)
    return val, held


def sample(fld, voxel, xyz, pose, origin=(0.0, 0.0, 0.0), dtype=F32, anchor_floor=False, divide=True, corners7=False):
    """fld = (keys sorted, D) of the qualified voxels; xyz (n,3) float32 sensor frame; pose (4,4) float64 world -> namespace(d
    (n,), grad (n,3), n2 (n,), flag (n,) int32: 1 a value / 0 none, q (n,3) the map-frame point, f (n,3) the position in the
    cell, corners (n,) how many of the 8 voxels the field holds), all in dtype; d, grad, n2 are zeros without a value"""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    origin = np.asarray(origin, np.float64)
    half = 0.0 if anchor_floor else 0.5
    with np.errstate(all="ignore"):
        if dtype == F32:
            v = F32(voxel)
            q = I.transform(L.map_pose(pose, origin), xyz, F32)
            g = (q / v) - F32(half)
            D = np.asarray(fld[1], F32)
        else:
            v = float(voxel)
            pose = np.asarray(pose, np.float64)
            q = (xyz.astype(np.float64) @ pose[:3, :3].T + pose[:3, 3]) - origin
            g = q / v - half
            D = np.asarray(fld[1], np.float64)
        fl = np.floor(g)
        valid = np.all((fl >= CELL_LO) & (fl < CELL_HI), axis=1)           # a NaN fails
        f = (g - fl).astype(dtype)
        idx = np.where(valid[:, None], fl, 0).astype(np.int64)
        val, held = _corners((fld[0], D), idx, valid)
        corners = held.reshape(len(xyz), 8).sum(axis=1)
        has = valid & (corners >= (7 if corners7 else 8))
        fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
        if dtype == F32:
            e = val[:, 1] - val[:, 0]                                       # [dy][dz]
            c = val[:, 0] + fx[:, None, None] * e
            m = c[:, 1] - c[:, 0]                                           # [dz]
            b = c[:, 0] + fy[:, None] * m
            hz = b[:, 1] - b[:, 0]
            d = b[:, 0] + fz * hz
            hy = m[:, 0] + fz * (m[:, 1] - m[:, 0])
            t = e[:, 0] + fy[:, None] * (e[:, 1] - e[:, 0])
            hx = t[:, 0] + fz * (t[:, 1] - t[:, 0])
            h = np.stack([hx, hy, hz], axis=1)
        else:
            w = [np.stack([1.0 - f[:, a], f[:, a]], axis=1) for a in range(3)]
            s = np.stack([-np.ones(len(xyz)), np.ones(len(xyz))], axis=1)
            d = np.einsum("nxyz,nx,ny,nz->n", val, w[0], w[1], w[2])
            h = np.stack([np.einsum("nxyz,nx,ny,nz->n", val, s, w[1], w[2]), np.einsum("nxyz,nx,ny,nz->n", val, w[0], s, w[2]),
                          np.einsum("nxyz,nx,ny,nz->n", val, w[0], w[1], s)], axis=1)
        grad = (h / v if divide else h).astype(dtype)
        n2 = (grad[:, 0] * grad[:, 0] + grad[:, 1] * grad[:, 1]) + grad[:, 2] * grad[:, 2]
        zero = dtype(0)
        d, grad, n2 = np.where(has, d, zero).astype(dtype), np.where(has[:, None], grad, zero).astype(dtype), np.where(has, n2, zero).astype(dtype)
    return SimpleNamespace(d=d, grad=grad, n2=n2, flag=has.astype(np.int32), q=q.astype(dtype), f=f, corners=corners)


def compare_samples(s32, s64, voxel):
    """the float32 form against the float64 form on the same rows -> (largest |d32 - d64| over the rows that have a value in
    both, largest |grad32 - grad64| over those of them farther than NEAR_FACE voxels from a cell face, the share of AMBIGUOUS
    rows: nearer than that, or with different flags)"""
    both = (s32.flag == 1) & (s64.flag == 1)
    f = s64.f
    near = (np.minimum(f, 1.0 - f) < NEAR_FACE).any(axis=1)
    doubt = (s32.flag != s64.flag) | ((s32.flag == 1) | (s64.flag == 1)) & near
    dd = np.abs(s32.d.astype(np.float64) - s64.d)[both]
    dg = np.abs(s32.grad.astype(np.float64) - s64.grad)[both & ~near]
    return (float(dd.max()) if dd.size else 0.0), (float(dg.max()) if dg.size else 0.0), float(doubt.mean()) if len(doubt) else 0.0


# ---------------------------------------------------------------------------------------------------------------------- system
def gate(s, max_dist, grad_min, dtype):
    """which rows the accumulate kernel gives: a value, |d| <= (float)max_dist, n2 >= (float)(grad_min^2), n2 finite"""
    md, g2 = (F32(max_dist), F32(grad_min * grad_min)) if dtype == F32 else (float(max_dist), float(grad_min * grad_min))
    with np.errstate(invalid="ignore"):
        return (s.flag == 1) & (np.abs(s.d) <= md) & (s.n2 >= g2) & np.isfinite(s.n2)


def system(s, max_dist, grad_min, kernel_scale, dtype, rows=None, negate_rot=False):
    """s = sample(...) -> (S (29,), J (m,6), e (m,), w (m,), give (n,) bool).  rows: the rows to form the sums on instead of the
    gate's own (the kernel's, for a comparison on equal rows).  The rows are float64 of the sampled values, as on the GPU."""
    give = gate(s, max_dist, grad_min, dtype) if rows is None else np.asarray(rows, bool)
    p, g, e = s.q[give].astype(np.float64), s.grad[give].astype(np.float64), s.d[give].astype(np.float64)
    J = np.concatenate([np.cross(p, g), g], axis=1).reshape(-1, 6)
    if negate_rot:
        J[:, :3] = -J[:, :3]
    w = I.weights(e * e, kernel_scale, np.float64)
    return I.system(J, e, int(give.sum()), np.float64, w), J, e, w, give


def system_floor(J, e, w, kernel_scale, p, delta_p, delta_d, delta_g):
    """What errors of up to delta_p in every coordinate of the moved point p (m,3), delta_d in the residual and delta_g in
    every component of the gradient can move each sum by.  An entry of p x g moves by delta_p (|g_b| + |g_c|) + delta_g
    (|p_b| + |p_c|), an entry of g by delta_g; with E = e e, |dE| <= 2 |e| delta_d and dw <= 2 w / (k + E) dE.  A term w J_i J_j
    moves by w (|J_i| dJ_j + |J_j| dJ_i) + dw |J_i J_j|, w J_i e by w (|J_i| delta_d + |e| dJ_i) + dw |J_i e|, e e by 2 |e| delta_d."""
    aJ, ae, w, ap = np.abs(J).astype(np.float64), np.abs(e).astype(np.float64), w.astype(np.float64), np.abs(p).astype(np.float64)
    ag = aJ[:, 3:]
    dJ = np.zeros_like(aJ)
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        dJ[:, a] = delta_p * (ag[:, b] + ag[:, c]) + delta_g * (ap[:, b] + ap[:, c])
    dJ[:, 3:] = delta_g
    dw = np.zeros(len(e))
    if kernel_scale > 0:
        dw = 2 * w / (kernel_scale * kernel_scale + ae * ae) * (2 * ae * delta_d)
    H = w[:, None, None] * (aJ[:, :, None] * dJ[:, None, :] + aJ[:, None, :] * dJ[:, :, None]) + dw[:, None, None] * aJ[:, :, None] * aJ[:, None, :]
    g = w[:, None] * (aJ * delta_d + ae[:, None] * dJ) + dw[:, None] * aJ * ae[:, None]
    return np.concatenate([H.sum(axis=0)[I.IU], g.sum(axis=0), [0.0], [(2 * ae * delta_d).sum()]])


def input_deltas(s32, fld, voxel, truncation):
    """the deltas system_floor takes, from the precision of float32: the moved point carries 4 ulps of its largest coordinate
    (three products and three sums); a field value is rounded once and the interpolant adds 7 roundings of values within the
    truncation, and moves with the point by at most |grad| delta_p per axis; a gradient entry is a difference of such values
    over v, and moves with the point's place in the cell by at most the cell's largest mixed difference / v per delta_p / v"""
    u = 2.0 ** -24
    delta_p = 4 * u * max(float(np.abs(s32.q[np.isfinite(s32.q).all(axis=1)]).max()), 1.0)
    gmax = float(np.sqrt(np.abs(s32.n2.astype(np.float64)).max())) if len(s32.n2) else 0.0
    delta_d = 8 * u * truncation + 3 * gmax * delta_p
    delta_g = 8 * u * truncation / voxel + 2 * (delta_p / voxel) * (4 * truncation / voxel)
    return delta_p, delta_d, delta_g


# ---------------------------------------------------------------------------------------------------------------- registration
def register(fld, voxel, xyz, origin, init, schedule, kernel_scale=0.0, tol_rot=1e-7, tol_trans=1e-6, grad_min=0.5, dtype=np.float64,
             negate_rot=False, **mutants):
    """-> dict(pose, fitness, rmse, iterations, status): icp_restated.iterate over the field rows.  The step acts on the pose
    in the map frame (the world pose minus origin)."""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)

    def system_of(local, max_dist):
        s = sample(fld, voxel, xyz, I._shifted(local, origin, 1), origin, dtype, **mutants)
        return system(s, max_dist, grad_min, kernel_scale, dtype, negate_rot=negate_rot)[0]
    return I.iterate(system_of, len(xyz), init, schedule, tol_rot, tol_trans, origin)


def tracker(frames, normals=None, first_pose=None, voxel=0.2, truncation=None, step=None, min_range=0.0, max_range=100.0, origin=None,
            distance="ray", cos_min=0.0, schedule=None, kernel_scale=0.0, min_count=1, grad_min=0.5, min_fitness=0.3,
            register_every=1, dtype=np.float64, starts=None):
    """TsdfTracker over frames [(n,3) float32] (normals: one (n,3) array per frame for distance="plane") -> (poses (F,4,4),
    statuses, fitnesses, lost, the map).  The map is the float32 restatement of the fusion; the registration runs in dtype on
    its exported field (float32 values; float64 of the same sums for dtype float64).  starts: {frame: pose} in place of the
    prediction."""
    first = np.eye(4) if first_pose is None else np.array(first_pose, np.float64)
    origin = first[:3, 3].copy() if origin is None else np.asarray(origin, np.float64)
    tau = 3.0 * voxel if truncation is None else float(truncation)
    if distance == "plane":
        m = TP.FusedPlane(voxel, origin, truncation, step, min_range, max_range, cos_min)
        put = lambda k, P: m.integrate(frames[k], P, normals[k])
    else:
        m = R.Fused(voxel, origin, truncation, step, min_range, max_range)
        put = lambda k, P: m.integrate(frames[k], P)
    unit = TP.WEIGHT_ONE if distance == "plane" else 1
    stages = ((tau, 30),) if schedule is None else schedule
    poses, statuses, fits, lost = [], [], [], 0
    for k in range(len(frames)):
        if k == 0:
            P, status, fit = first, CONVERGED, 1.0
            put(0, P)
        else:
            start = poses[-1] @ (np.linalg.inv(poses[-2]) @ poses[-1]) if k >= 2 else poses[-1].copy()
            if starts is not None and k in starts:
                start = np.array(starts[k], np.float64)
            fld = R.field(m.export(), max(1, int(round(min_count * unit))), F32 if dtype == F32 else np.float64)
            r = register(fld, voxel, np.asarray(frames[k], F32)[::register_every], origin, start, stages, kernel_scale,
                         grad_min=grad_min, dtype=dtype)
            status, fit = r["status"], r["fitness"]
            if status in (CONVERGED, MAX_ITER) and fit >= min_fitness:
                P = r["pose"]
                put(k, P)
            else:
                P, lost = start, lost + 1
        poses.append(P), statuses.append(status), fits.append(fit)
    return np.stack(poses), statuses, fits, lost, m


def pose_error(pose, true):
    """(translation error in metres, || R - R_true ||_F)"""
    return float(np.linalg.norm(pose[:3, 3] - true[:3, 3])), float(np.linalg.norm(pose[:3, :3] - true[:3, :3]))


# --------------------------------------------------------------------------------------------------------------------- scenes
PATCHES = (((1.0, 0.2, 0.1), 6.0), ((-0.15, 1.0, 0.2), 5.0), ((0.1, -0.2, -1.0), 2.5))   # planes n . x = d, sensor frame
PATCH_POSE = ([0.11, -0.23, 0.31], [1.37, -0.71, 0.43])                                     # the general pose they are seen under


def patch(n, d, side=41, spacing=0.1):
    """side x side returns `spacing` apart on the plane n . x = d round its foot point, nudged off the voxel lattice -> (xyz
    (side^2,3) float32, the unit normal repeated (side^2,3) float32), sensor frame"""
    n = np.asarray(n, np.float64)
    n = n / np.linalg.norm(n)
    a = np.cross(n, [0.0, 0.0, 1.0] if abs(n[2]) < 0.9 else [1.0, 0.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(n, a)
    s = (np.arange(side) - (side - 1) / 2) * spacing
    u, w = [g.ravel() for g in np.meshgrid(s + 0.0137, s - 0.0291, indexing="ij")]
    pts = n[None, :] * d + u[:, None] * a[None, :] + w[:, None] * b[None, :]
    return pts.astype(F32), np.repeat(n[None, :], len(pts), axis=0).astype(F32)


def patches_case(origin=(0.0, 0.0, 0.0), which=(0, 1, 2), n_src=1100, seed=11):
    """the known-answer scene -> namespace(xyz, normals (the fused returns, sensor frame), pose (the true one, world), origin,
    src (n_src of the returns), start (the pose 0.3 m and 2 degrees off), voxel 0.5)"""
    parts = [patch(*PATCHES[i]) for i in which]
    xyz, nrm = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    pose = I.se3(*PATCH_POSE)
    start = I.perturbed(pose, seed=seed + 1, trans=0.3, deg=2.0)      # turned about the map's origin, not the world's
    pose[:3, 3] += np.asarray(origin, np.float64)
    start[:3, 3] += np.asarray(origin, np.float64)
    rng = np.random.default_rng(seed)
    src = xyz[rng.choice(len(xyz), min(n_src, len(xyz)), replace=False)]
    return SimpleNamespace(xyz=xyz, normals=nrm, pose=pose, origin=np.asarray(origin, np.float64), src=src,
                           start=start, voxel=0.5)


def fuse_case(c, distance="plane"):
    """the float32 restatement's map of a patches_case, fused once -> the map"""
    if distance == "plane":
        return TP.FusedPlane(c.voxel, c.origin).integrate(c.xyz, c.pose, c.normals)
    return R.Fused(c.voxel, c.origin).integrate(c.xyz, c.pose)


BOX = (8.0, 6.0, 3.0)


def box_room(frames=8, advance=0.12, columns=96, beams=48):
    """a sensor moving through a closed box room of 8 x 6 x 3 m centred on the origin: `frames` poses `advance` metres apart along
    a gently turning path, columns x beams rays each -> (xyz per frame [(n,3) float32, sensor frame], analytic normals per frame
    [(n,3) float32, sensor frame], poses (frames,4,4) float64)"""
    az = (np.arange(columns) + 0.37) * (2 * np.pi / columns)
    el = np.radians(np.linspace(-38.0, 38.0, beams) + 0.21)
    e, a = [g.ravel() for g in np.meshgrid(el, az, indexing="ij")]
    rays = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], axis=1)
    half = np.array(BOX) / 2
    out_xyz, out_n, poses = [], [], []
    for k in range(frames):
        P = I.se3([0.002 * k, -0.001 * k, 0.01 * k], [-0.43 + advance * k, 0.17 + 0.01 * k, 0.09 - 0.004 * k])
        d = rays @ P[:3, :3].T
        o = P[:3, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(d > 0, (half - o) / d, np.where(d < 0, (-half - o) / d, np.inf))
        axis = np.argmin(t, axis=1)
        tt = t[np.arange(len(t)), axis]
        nw = np.zeros_like(d)
        nw[np.arange(len(d)), axis] = -np.sign(d[np.arange(len(d)), axis])      # into the room
        out_xyz.append((rays * tt[:, None]).astype(F32))
        out_n.append((nw @ P[:3, :3]).astype(F32))
        poses.append(P)
    return out_xyz, out_n, np.stack(poses)
