"""The inputs of tests/test_gpu_tsdf_raycast.py, shared with tests/test_tsdf_raycast_host.py, which shows on the CPU what they can
tell apart (the mutants of tsdf_raycast_restated.cast32) and that they stay under the ambiguity cap.

A cast case is a SimpleNamespace: map (a case of tsdf_cases / test_tsdf_plane_host: what is fused), distance ("ray" / "plane"),
min_count (full-weight samples), poses (F,4,4) float64, dirs (R,3) float32 in the sensor frame, lo, hi, step.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restated as I  # noqa: E402
import tsdf_cases as C  # noqa: E402
import tsdf_plane_restated as PR  # noqa: E402
import tsdf_register_restated as RR  # noqa: E402
import tsdf_restated as R  # noqa: E402
import test_tsdf_plane_host as H  # noqa: E402
from test_tsdf_host import valid  # noqa: E402

F32 = np.float32
SIZES = (0, 1, 63, 64, 65, 257)
FAR = np.array([1000.0, -2000.0, 500.0])


def log(line):
    """what a test observed: printed, and appended to test_logs/tsdf_raycast.log (scripts/sim_tsdf_raycast_eval.py --accuracy
    turns that into profiles/tsdf_raycast_accuracy.md)"""
    print(line)
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        os.makedirs(os.path.join(root, "test_logs"), exist_ok=True)
        with open(os.path.join(root, "test_logs", "tsdf_raycast.log"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def aim(pose, targets):
    """unit directions, in the sensor frame of `pose`, towards world points -> (n,3) float32"""
    d = (np.asarray(targets, np.float64) - pose[:3, 3]) @ pose[:3, :3]
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)


def shifted(c, far):
    """the whole set-up of a map case moved to `far`, with the map's origin there too"""
    frames = []
    for xyz, count, pose in c.frames:
        P = pose.copy()
        P[:3, 3] += far
        frames.append((xyz, count, P))
    c.frames, c.origin = frames, np.asarray(far, np.float64).copy()
    return c


def cast(map_case, poses, dirs, lo, hi, step, distance="ray", min_count=1):
    return SimpleNamespace(map=map_case, distance=distance, min_count=min_count, poses=np.asarray(poses, np.float64).reshape(-1, 4, 4),
                           dirs=np.ascontiguousarray(dirs, F32).reshape(-1, 3), lo=lo, hi=hi, step=step)


# ------------------------------------------------------------------------------------------------------------ the tilted wall
WALL_POSES = (([0.02, -0.05, 0.1], [0.1, 0.3, -0.2]), ([-0.2, 0.1, 0.3], [-0.6, -0.4, 0.5]), ([0.1, 0.2, -0.4], [1.1, 0.2, 0.1]))


def wall_cast(n_rays=257, n_poses=1, distance="ray", min_count=1, far=None, lo=0.9, hi=9.0, step=0.1):
    """tsdf_cases.wall (dense: cells have their 8 corners, also at min_count 2) seen from poses that did not fuse it: rays
    towards points of the wall's plane, some beside the wall, a zero direction, a NaN direction and one that looks away.  The
    step 0.1 and the start 0.9 are no binary fractions: t_k = t0 + k h and t += h differ."""
    c = H.wall() if distance == "plane" else C.wall()
    poses = np.stack([I.se3(*p) for p in WALL_POSES[:n_poses]])
    rng = np.random.default_rng(5)
    a, b = rng.uniform(-2.6, 2.6, (2, 257))
    targets = np.stack([4.0 + 0.3 * a - 0.2 * b, a, b], axis=1)
    dirs = aim(poses[0], targets)
    dirs[5], dirs[9], dirs[11] = 0.0, np.nan, [-1.0, 0.0, 0.0]
    dirs = dirs[:n_rays] if n_rays != 1 else dirs[20:21]
    if far is not None:
        shifted(c, far)
        poses[:, :3, 3] += far
    return cast(c, poses, dirs, lo, hi, step, distance, min_count)


# --------------------------------------------------------------------------------------------------- the wall on the lattice
WALL_X = -5.3


def lattice_wall():
    """a wall in the plane x = -5.3 over y, z in [-5, 1] (negative coordinates; voxel 0.5, so a block is 4 m and the planes
    y = -4, z = -4, y = 0, z = 0 are block faces), returns 0.1 m apart, seen from one pose"""
    s = np.arange(-50, 11) * 0.1 + 0.013
    y, z = [g.ravel() for g in np.meshgrid(s, s - 0.007)]
    world = np.stack([np.full(len(y), WALL_X), y, z], axis=1)
    pose = at(1.3, -2.1, -1.9)
    xyz = (world - pose[:3, 3]).astype(F32)
    return C._case([(xyz, len(xyz), pose)])


def at(x, y, z):
    P = np.eye(4)
    P[:3, 3] = [x, y, z]
    return P


AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0, 0], [np.nan, 0, 0]], F32)


def lattice_cast():
    """rays along the axes (and a zero and a NaN direction) from points on the lattice, every sample exact in float32: inside
    voxel-face planes (coordinates on multiples of 0.5) and through voxel centres (odd multiples of 0.25), inside block-face
    planes and through block corners (multiples of 4), in front of the wall, inside its negative band (x = -5.75: BACK along
    +x) and beyond it (x = -9: MISS along -x, BACK along +x)"""
    poses = [at(2, 0, 0), at(2, -0.5, -1.0), at(2, -0.25, -0.25), at(2, -4, -4), at(2, -4, 0), at(-5.75, -2, -2), at(-5.0, -2.25, -2.25),
             at(-9, -2, -2), at(-4, -4, -4)]
    return cast(lattice_wall(), np.stack(poses), AXES, 0.0, 9.0, 0.25)


def between_cast(hi):
    """a ray along -x from x = 2.075: the wall at -5.3 is 7.375 m away, between the samples at 7.25 and 7.5.  hi = 7.4 ends the
    samples at 7.25 (MISS); hi = 7.5 holds both (HIT)."""
    return cast(lattice_wall(), at(2.075, -1.3, -1.3)[None], AXES[1:2], 0.0, hi, 0.25)


def table_bytes(exported, cap_vox):
    """(keys, sums, counts) -> the map buffer dpm_tsdf_bytes(cap_vox) long that holds them: the 256-byte header zeroed, every
    key in the first free slot from mix64(key) & (cap_vox - 1) on (include/dpm_hip.h); the slots a table has are not part of
    its meaning, so any order of insertion does"""
    import lidar_odometry_restated as L
    K, S, N = np.full(cap_vox, np.uint64(2 ** 64 - 1)), np.zeros(cap_vox, np.int64), np.zeros(cap_vox, np.uint32)
    for k, a, n in zip(*[np.asarray(x).tolist() for x in exported]):
        slot = L.mix64(k) & (cap_vox - 1)
        while K[slot] != np.uint64(2 ** 64 - 1):
            slot = (slot + 1) & (cap_vox - 1)
        K[slot], S[slot], N[slot] = k, a, n
    return np.concatenate([np.zeros(256, np.uint8), K.view(np.uint8), S.view(np.uint8), N.view(np.uint8)])


def seven_cast():
    """a table written by hand: the voxels [-3, 3]^3 (voxel 0.5) with D = half the x of the centre, one sample each, WITHOUT
    the voxel (-1, 0, 0).  The field is x / 2: positive, then negative along -x.  The ray from (1.1, 0.1, 0.1) along -x has its
    samples at x = 0.35 (valued, positive), 0.1 and -0.15 (the crossing's two samples: their cell lacks exactly the one voxel,
    7 of 8 corners), -0.4 and -0.65 (the next cell, 7 of 8 too), -0.9 (valued, negative): MISS, not HIT.  The same ray from
    (1.1, 1.1, 0.1), a cell further in y, has all its corners: HIT at 1.1 m."""
    import lidar_odometry_restated as L
    idx = np.array([[x, y, z] for x in range(-3, 4) for y in range(-3, 4) for z in range(-3, 4) if (x, y, z) != (-1, 0, 0)])
    keys = L.pack_key(idx)
    order = np.argsort(keys)
    sums = np.rint((0.25 * idx[:, 0] + 0.125) * R.FIX_ONE).astype(np.int64)
    c = cast(C._case([], cap_vox=1 << 10), np.stack([at(1.1, 0.1, 0.1), at(1.1, 1.1, 0.1)]), AXES, 0.0, 2.5, 0.25)
    c.exported = (keys[order], sums[order], np.ones(len(keys), np.uint32))
    return c


def zero_cast():
    """a plane-form map whose field is EXACTLY 0 on a layer of voxels: a wall in the plane x = -5.25 through voxel centres, every
    coordinate a multiple of 1/8 and the pose on the lattice, so that q - c is exactly 0 along the normal for every sample of
    that layer.  Rays along the axes from a voxel centre OF that layer (sample 0 has d = 0: with s(d) = d > 0 it counts as
    negative and the ray along -x, into the negative side, never crosses; s(d) = d >= 0 would call that a HIT at range 0) and
    from 2 m in front of it (the sample at 2 m has d = 0: HIT at exactly 2 m)"""
    s = np.arange(-32, 1) * 0.125
    y, z = [g.ravel() for g in np.meshgrid(s, s)]
    world = np.stack([np.full(len(y), -5.25), y, z], axis=1)
    pose = at(1.25, -2.0, -2.0)
    xyz = (world - pose[:3, 3]).astype(F32)
    c = C._case([(xyz, len(xyz), pose)])
    c.normals, c.cos_min = [np.tile(np.array([-1, 0, 0], F32), (len(xyz), 1))], 0.0
    return cast(c, np.stack([at(-5.25, -2.25, -2.25), at(-3.25, -2.25, -2.25)]), AXES, 0.0, 3.0, 0.25, "plane", 1 / 256)


def outside_cast():
    """tsdf_cases.outside: a sensor 2 m inside the end of the 21-bit key range looking out; the rays leave the 21 bits"""
    c = C.outside()
    xyz, _, pose = c.frames[0]
    dirs = np.concatenate([(xyz / np.linalg.norm(xyz, axis=1, keepdims=True)).astype(F32), AXES[:6]])
    return cast(c, pose[None], dirs, 0.0, 13.0, 0.25)


def empty_cast():
    c = C._case([])
    return cast(c, np.stack([I.se3(*p) for p in WALL_POSES]), wall_cast().dirs[:65], 0.9, 9.0, 0.1)


def cast_cases():
    out = {f"rays{n}": wall_cast(n) for n in SIZES}
    out.update(poses3=wall_cast(257, 3), poses3_min2=wall_cast(257, 3, min_count=2), plane=wall_cast(257, 3, "plane"),
               plane_min2=wall_cast(257, 3, "plane", min_count=2.5), far=wall_cast(257, 3, far=FAR),
               one_sample=wall_cast(65, 3, lo=4.0, hi=4.0), lattice=lattice_cast(), between_miss=between_cast(7.4),
               between_hit=between_cast(7.5), seven=seven_cast(), zero=zero_cast(), outside=outside_cast(), empty=empty_cast())
    return out


def unit_of(c):
    return PR.WEIGHT_ONE if c.distance == "plane" else 1


def count_units(c):
    return max(1, int(round(float(c.min_count) * unit_of(c))))


def export_restated(c):
    """the sorted export of a cast case's map: the table written by hand, or the float32 restatement's fusion"""
    return c.exported if hasattr(c, "exported") else fuse_restated(c).export()


def fuse_restated(c):
    """the float32 restatement's map of a cast case's map"""
    m = c.map
    if c.distance == "plane":
        return H.fuse_plane(m)
    f = R.Fused(m.voxel, m.origin, m.truncation, m.step, m.min_range, m.max_range)
    for frame in m.frames:
        f.integrate(*valid(frame))
    return f


def restated(c, exported, dtype=F32, **mutants):
    """cast32 (or cast64 for dtype float64) of the case on an exported table"""
    import tsdf_raycast_restated as RC
    fld = R.field(exported, count_units(c), dtype)
    if dtype == F32:
        return RC.cast32(fld, c.map.voxel, c.map.origin, c.poses, c.dirs, c.lo, c.hi, c.step, **mutants)
    return RC.cast64(fld, c.map.voxel, c.map.origin, c.poses, c.dirs, c.lo, c.hi, c.step)


# ------------------------------------------------------------------------------------------------------------ known answers
def slanted_dense(tilt):
    """test_tsdf_plane_host.slanted(tilt) -- the same plane, sensor, voxel, truncation and step -- seen by 512 x 96 rays in place
    of 256 x 48.  At tilt 1.2 the part of the plane more than tau + sqrt(3) v inside the border is at least 10 m away under an
    incidence of 53 degrees or more: the 256 x 48 returns lie 0.29 m apart there, more than a voxel (0.25 m), voxels of the band
    stay empty and the float32 restatement itself misses 82 of the 225 rays below.  Twice the rays in each direction leave the
    returns 0.14 m apart."""
    c = H.slanted(tilt)
    n_w = c.plane[0]
    az = np.linspace(-np.pi, np.pi, 512, endpoint=False) + 0.0123
    el = np.linspace(-0.4, 0.4, 96) + 0.0031
    A, E = np.meshgrid(az, el)
    dirs = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)
    den = dirs @ n_w
    hit = den > 1e-3
    t = 6.0 / den[hit]
    xyz = (dirs[hit] * t[:, None])[t < 40.0].astype(F32)
    c.frames = [(xyz, len(xyz), c.frames[0][2])]
    c.normals = [np.tile(n_w.astype(F32), (len(xyz), 1))]
    c.cap_vox = 1 << 19
    return c


def tilted_cast(tilt):
    """slanted_dense(tilt), cast from a second pose: a fan of 15 x 15 rays towards the part of the plane the
    fusing sensor saw at azimuth 0 and elevation 0 (0.15 from tilt 1 on, where elevation 0 is farther off) -> the cast case with
    analytic (R,) float64 = the range to the plane along each ray and required (R,) bool = the analytic hit lies more than tau +
    sqrt(3) v inside the border of the fused patch (range below 40 m from the fusing sensor, elevation within its +-0.4 rad)"""
    c = slanted_dense(tilt)
    n_w, d = c.plane
    s = c.frames[0][2][:3, 3]
    e0 = 0.15 if tilt >= 1.0 else 0.0
    u0 = np.array([np.cos(e0), 0.0, np.sin(e0)])
    centre = s + u0 * ((d - n_w @ s) / (n_w @ u0))
    e1 = np.array([0.0, 1.0, 0.0])
    e2 = np.cross(n_w, e1)
    g = np.linspace(-1.0, 1.0, 15)
    a, b = [x.ravel() for x in np.meshgrid(g + 0.011, g - 0.017)]
    targets = centre + a[:, None] * e1 + b[:, None] * e2
    pose = I.se3([0.05, -0.08, 0.12], [0.41, -0.33, 0.27])
    dirs = aim(pose, targets)
    cc = cast(c, pose[None], dirs, 0.5, 14.0, c.step, "plane", 1 / 256)
    u = dirs.astype(np.float64) @ pose[:3, :3].T
    cc.u_dot_n = u @ n_w
    cc.analytic = (d - n_w @ pose[:3, 3]) / cc.u_dot_n
    hit = pose[:3, 3] + u * cc.analytic[:, None]
    margin = c.truncation + np.sqrt(3.0) * c.voxel
    rel = hit - s
    r = np.linalg.norm(rel, axis=1)
    el = np.arcsin(rel[:, 2] / r)
    cc.required = (r + margin < 40.0) & (np.abs(el - 0.0031) + np.arcsin(margin / r) < 0.4)
    return cc


SPHERE_STARTS = ((0.0, 0.0, 0.0), (0.6, -0.6, 0.5291502622129182))      # the centre (the fusing sensor), and 1 m off it


def sphere_cast(start):
    """tsdf_cases.sphere (ray form) cast from the fusing sensor's place plus `start`: 48 x 23 rays up to 78 degrees of elevation
    (the fused rays reach 88.6) -> the cast case with analytic (R,) ranges to the sphere and normals (R,3) in the sensor frame:
    towards the sensor's side, the inward radius"""
    c = C.sphere()
    s = C.SPHERE
    az = (np.arange(48) + 0.31) * 2 * np.pi / 48
    el = np.radians(np.linspace(-78.0, 78.0, 23) + 0.17)
    az, el = [g.ravel() for g in np.meshgrid(az, el)]
    dirs = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1).astype(F32)
    pose = np.eye(4)
    pose[:3, 3] = s.sensor + np.asarray(start)
    cc = cast(c, pose[None], dirs, 0.0, 5.0, s.step)
    u, o = dirs.astype(np.float64), np.asarray(start, np.float64)      # the sphere's centre is the fusing sensor
    ou = u @ o
    cc.analytic = -ou + np.sqrt(ou * ou - (o @ o - s.rho ** 2))
    hit = o + u * cc.analytic[:, None]
    cc.analytic_normals = -hit / s.rho
    return cc


def walls_cast():
    """test_tsdf_plane_host.two_walls: 5 x 5 rays within 0.1 rad of the sensor's +x, through the middle of the place the wall at
    5 m stood -> the cast case with ux (R,) = the x component of each ray (range * ux is the wall's distance along x)"""
    c = H.two_walls()
    g = np.linspace(-0.1, 0.1, 5)
    a, e = [x.ravel() for x in np.meshgrid(g + 0.003, g - 0.002)]
    dirs = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], axis=1).astype(F32)
    cc = cast(c, c.frames[0][2][None], dirs, 0.5, 14.0, c.step, "plane", 1)
    cc.ux = dirs[:, 0].astype(np.float64)
    return cc


def render_model():
    from deeppointmap_amd.lidar_sim import LidarModel
    return LidarModel(np.linspace(40.0, -85.0, 32), 128, 0.5, 12.0)
