"""The inputs of tests/test_gpu_tsdf.py, shared with tests/test_tsdf_host.py, which shows on the CPU what they can tell apart
(the three mutants of tsdf_restated.Fused) and that they stay under the ambiguity cap.

A case is a SimpleNamespace: voxel, truncation, step, min_range, max_range, origin, cap_vox and frames = [(xyz (cap,3) float32,
count, pose (4,4) float64)]: rows at and past `count` must never be read.
"""
import itertools
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restated as I  # noqa: E402

CAPS = (0, 1, 63, 64, 65, 257)
LIST_SHAPES = [(F, P) for F in (0, 1, 3, 17) for P in (1, 255, 256, 257)]
# both range gates at equality (1 and 13 m), one step beyond each, a NaN row
PLANTED = np.array([[1, 0, 0], [5, 12, 0], [5, 12.25, 0], [0.75, 0, 0], [np.nan, 0, 0]], np.float32)


def _rotations():
    """the 24 rotations with entries in {-1, 0, 1}: fp32 transforms of lattice points under them are exact"""
    out = []
    for p in itertools.permutations(range(3)):
        for sign in itertools.product((1.0, -1.0), repeat=3):
            M = np.zeros((3, 3))
            for r in range(3):
                M[r, p[r]] = sign[r]
            if np.linalg.det(M) > 0:
                out.append(M)
    return out


ROTATIONS = _rotations()


def _case(frames, **kw):
    base = dict(voxel=0.5, truncation=1.5, step=0.25, min_range=1.0, max_range=13.0, origin=np.zeros(3), cap_vox=1 << 14)
    base.update(kw)
    return SimpleNamespace(frames=frames, **base)


def general(cap, seed=0, n_frames=1):
    """random returns within 6 m per axis under general poses; from 8 rows on the planted rows are among them"""
    rng = np.random.default_rng(100 * cap + seed)
    frames = []
    for f in range(n_frames):
        xyz = rng.uniform(-6, 6, (cap, 3)).astype(np.float32)
        if cap >= 8:
            xyz[rng.permutation(cap)[:len(PLANTED)]] = PLANTED
        frames.append((xyz, cap, I.se3(rng.normal(0, 0.3, 3), rng.uniform(-2, 2, 3))))
    return _case(frames)


def counted():
    """count < cap: NaN rows below the count, and past it valid returns that would change the map if they were read"""
    c = general(257, seed=1)
    xyz, _, pose = c.frames[0]
    xyz[[3, 77, 199]] = np.nan
    c.frames = [(xyz, 200, pose)]
    return c


def lattice():
    """returns on multiples of 0.25 m (voxel 0.5: on faces, edges and corners of voxels), negative coordinates, an exact pose"""
    rng = np.random.default_rng(2)
    xyz = (rng.integers(-24, 25, (257, 3)) * 0.25).astype(np.float32)
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = ROTATIONS[7], [-1.25, 0.5, -2.0]
    return _case([(xyz, 257, pose)])


def face_rays():
    """rays along the axes from a sensor on a lattice point: every sample lies exactly in two face planes"""
    xyz = np.array([[4, 0, 0], [-4, 0, 0], [0, -3, 0], [0, 3.25, 0], [0, 0, 2.5], [0, 0, -6]], np.float32)
    pose = np.eye(4)
    pose[:3, 3] = [1.0, -2.0, 0.5]
    return _case([(xyz, len(xyz), pose)])


def short():
    """returns nearer than the truncation (samples with t <= 0 occur), one at range 0 (no direction: its samples are counted
    outside), min_range 0"""
    xyz = np.array([[0.5, 0, 0], [0.3, -0.2, 0.1], [0, 0, 0], [0, 0.75, 0], [-0.26, 0.26, 1.0], [1.5, 0, 0]], np.float32)
    return _case([(xyz, len(xyz), I.se3([0.1, -0.2, 0.3], [0.3, 0.1, -0.2]))], min_range=0.0)


def outside():
    """a sensor 2 m inside the end of the 21-bit key range (2^20 voxels of 0.5 m) looking out: samples beyond it are counted"""
    xyz = np.array([[3, 0.3, 0.2], [2.5, -1, 0], [-3, 0, 0], [1.75, 0.1, 3], [4, 4, 4]], np.float32)
    pose = np.eye(4)
    pose[:3, 3] = [524286.0, 0.0, -524287.0]
    return _case([(xyz, len(xyz), pose)])


def too_small():
    """more voxels than slots"""
    c = general(257, seed=3)
    c.cap_vox = 64
    return c


def two_frames():
    return general(257, seed=4, n_frames=2)


def wall():
    """a tilted wall 4 m away seen densely (returns 0.2 m apart, voxel 0.5) from two poses: whole blocks of voxels hold samples,
    so that cells have their 8 corners and the mesh has triangles, also with min_count 2"""
    a, b = [g.ravel() for g in np.meshgrid(np.arange(-10, 11) * 0.2 + 0.037, np.arange(-10, 11) * 0.2 + 0.061)]   # off the voxel faces
    world = np.stack([4.0 + 0.3 * a - 0.2 * b, a, b], axis=1)
    frames = []
    for rot, t in (([0.05, -0.1, 0.2], [0.3, -0.2, 0.1]), ([-0.1, 0.05, -0.3], [-0.4, 0.5, -0.3])):
        pose = I.se3(rot, t)
        xyz = ((world - pose[:3, 3]) @ pose[:3, :3]).astype(np.float32)        # R^T (w - t)
        frames.append((xyz, len(xyz), pose))
    return _case(frames)


def single_frame_cases():
    out = {f"cap{cap}": general(cap) for cap in CAPS}
    out.update(counted=counted(), lattice=lattice(), face_rays=face_rays(), short=short(), outside=outside(), two_frames=two_frames(),
               wall=wall())
    return out


def list_case(F, P, seed=0):
    """F list entries over a store of F + 2 rows of P columns: lengths 0 / below P / above P / negative, NaN columns, the planted
    rows, general poses; from F = 3 on one entry names a row outside the store"""
    rng = np.random.default_rng(1000 * F + P + seed)
    cap = F + 2
    store = rng.uniform(-6, 6, (cap, 3, P)).astype(np.float32)
    lengths = np.array([[P, P - P // 3, 0, P + 5, -3][(r + 1) % 5] for r in range(cap)], np.int32)
    for r in range(cap):
        store[r, :, r % P] = PLANTED[r % 5]
        if P >= 8:
            for j in range(5):
                store[r, :, (r + 1 + j) % P] = PLANTED[j]
    frames = rng.permutation(cap)[:F].astype(np.int32)
    if F >= 3:
        frames[1] = cap if F == 3 else -1
    poses = np.stack([I.se3(rng.normal(0, 0.3, 3), rng.uniform(-2, 2, 3)) for _ in range(F)]) if F else np.zeros((0, 4, 4))
    c = _case([], store=store, lengths=lengths, rows=frames, poses=poses)
    c.frames = [(np.ascontiguousarray(store[r, :, :min(max(int(lengths[r]), 0), P)].T), None, poses[f])
                for f, r in enumerate(frames) if 0 <= r < cap]
    return c


# ------------------------------------------------------------------------------------------------------------------ the sphere
SPHERE = SimpleNamespace(rho=3.0, voxel=0.25, truncation=0.75, step=0.125, azimuths=128, elevations=64,
                         sensor=np.array([0.03, -0.02, 0.01]))
SPHERE.bound = 3 * SPHERE.voxel ** 2 / (8 * (SPHERE.rho - SPHERE.truncation))    # 10.4 mm: see test_tsdf_host.py


def sphere(far=None):
    """a sphere of radius rho seen from its centre, an off-lattice point: rays on an azimuth x elevation grid.  far: the whole
    set-up moved there, with the map's origin there too"""
    s = SPHERE
    az = (np.arange(s.azimuths) + 0.5) * 2 * np.pi / s.azimuths
    el = (np.arange(s.elevations) + 0.5) * np.pi / s.elevations - np.pi / 2
    az, el = [g.ravel() for g in np.meshgrid(az, el)]
    u = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], axis=1)
    pose = np.eye(4)
    origin = np.zeros(3) if far is None else np.asarray(far, np.float64)
    pose[:3, 3] = s.sensor + origin
    xyz = (s.rho * u).astype(np.float32)
    return _case([(xyz, len(xyz), pose)], voxel=s.voxel, truncation=s.truncation, step=s.step, min_range=0.0, max_range=100.0,
                 origin=origin, cap_vox=1 << 15)
