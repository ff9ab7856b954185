"""CPU: the numpy restatement of the geometric odometry (tests/lidar_odometry_restated.py) checked against itself -- the
owner-word rule across and within frames, prune, the three searches against each other, the known-pose case in float64 --
and the argument refusals of the six C entry points (before any HIP call: they need no GPU)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restated as I  # noqa: E402
import lidar_odometry_restated as L  # noqa: E402

EYE = np.eye(4)
DTYPES = [np.float32, np.float64]


def f32(*rows):
    return np.array(rows, np.float32).reshape(-1, 3)


@pytest.mark.parametrize("dtype", DTYPES)
def test_first_wins_within_and_across_frames(dtype):
    m = L.Map(1.0, 2, dtype=dtype)
    # rows 5 and 2 share a sub-cell: the lower row wins whatever the order they are offered in
    m.insert(f32([0.1, 0.1, 0.1], [0.2, 0.2, 0.2]), [5, 2], EYE, stamp=3)
    keys, sub, owner, xyz = m.export()
    assert len(keys) == 1 and owner[0] == (3 << 32) | 2 and np.allclose(xyz[0], 0.2)
    # a later frame does not displace it, even with a lower row; an EARLIER stamp would
    m.insert(f32([0.3, 0.3, 0.3]), [0], EYE, stamp=4)
    assert m.export()[2][0] == (3 << 32) | 2
    m.insert(f32([0.3, 0.3, 0.3]), [9], EYE, stamp=1)
    assert m.export()[2][0] == (1 << 32) | 9
    # another sub-cell of the same voxel, and a voxel at negative coordinates: floor, not truncation
    m.insert(f32([0.6, 0.1, 0.1], [-0.1, -0.1, -0.1]), [0, 1], EYE, stamp=5)
    keys, sub, owner, xyz = m.export()
    assert len(keys) == 3 and list(L.unpack_key(keys[0])) == [-1, -1, -1] and sub[0] == 7
    assert list(sub[1:]) == [0, 1] and keys[1] == keys[2] == L.pack_key([0, 0, 0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_range_gates_hold_at_equality_and_rows_are_counted_outside(dtype):
    m = L.Map(1.0, 1, min_range=5.0, max_range=13.0, dtype=dtype)
    m.insert(f32([3, 4, 0], [2.5, 4, 0], [5, 12, 0], [5, 12.5, 0], [np.nan, 0, 0]), np.arange(5), EYE, 0)
    assert sorted(map(tuple, m.export()[3].tolist())) == [(3, 4, 0), (5, 12, 0)]
    far = L.Map(1.0, 1, max_range=1e9, dtype=dtype)
    far.insert(f32([2.0 ** 20, 0, 0], [2.0 ** 20 - 1, 0, 0], [-2.0 ** 20, 0, 0], [-2.0 ** 20 - 1, 0, 0]), np.arange(4), EYE, 0)
    assert far.outside == 2 and len(far.export()[0]) == 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_prune_keeps_centres_at_the_radius(dtype):
    m = L.Map(1.0, 1, dtype=dtype)
    m.insert(f32([3.2, 4.2, 0.2], [3.2, 5.2, 0.2], [0.2, 0.2, 0.2], [-4.8, 0.2, 0.2]), np.arange(4), EYE, 0)
    P = EYE.copy()
    P[:3, 3] = 0.5        # centres (3.5, 4.5, .5) and (-4.5, .5, .5) are exactly 5 away, (3.5, 5.5, .5) is farther
    m.prune(P, 5.0)
    assert sorted(map(tuple, L.unpack_key(m.export()[0]).tolist())) == [(-5, 0, 0), (0, 0, 0), (3, 4, 0)]
    m.prune(P, 0.0)
    assert sorted(map(tuple, L.unpack_key(m.export()[0]).tolist())) == [(0, 0, 0)]
    P[:3, 3] = 100.0
    m.prune(P, 1.0)
    assert len(m.export()[0]) == 0 and L.search27(f32([0, 0, 0]), m.export(), 1.0, 1, 1.0, dtype)[0] == -1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("voxel,s,max_dist", [(1.0, 3, 1.0), (1.0, 2, 0.4), (0.7, 3, 0.7), (2.0, 1, 1.5)])
def test_the_27_voxel_search_is_the_exhaustive_one(dtype, voxel, s, max_dist):
    rng = np.random.default_rng(7)
    m = L.Map(voxel, s, dtype=dtype)
    m.insert(rng.uniform(-4, 4, (1500, 3)).astype(np.float32), np.arange(1500), EYE, 0)
    ex = m.export()
    q = rng.uniform(-6, 6, (700, 3)).astype(dtype)
    win, near = L.search_exhaustive(q, ex, m.voxel, s, max_dist, dtype)
    assert near.all(), "a winner within max_dist <= voxel lay outside the 27 voxels"
    assert (win >= 0).sum() > 50 and (win < 0).sum() > 10
    assert np.array_equal(L.search27(q, ex, m.voxel, s, max_dist, dtype), win)
    assert np.array_equal(L.search_fast(q, ex, m.voxel, s, max_dist, dtype), win)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_ties_go_to_the_geometric_key(dtype):
    m = L.Map(1.0, 2, dtype=dtype)
    # two sub-cells of one voxel, and the same pair one voxel further along x
    m.insert(f32([0.25, 0.25, 0.25], [0.75, 0.25, 0.25], [1.25, 0.25, 0.25]), np.arange(3), EYE, 0)
    ex = m.export()
    q = f32([0.5, 0.25, 0.25], [1.0, 0.25, 0.25], [1.0, 0.25, 5.0]).astype(dtype)
    for search in (L.search27, L.search_fast, lambda *a: L.search_exhaustive(*a)[0]):
        win = search(q, ex, 1.0, 2, 1.0, dtype)
        # query 0: sub-cells 0 and 1 of its own voxel tie -> sub-cell 0; query 1 sits in voxel 1: voxel 0 is neighbour 12,
        # its own is 13 -> the point of voxel 0
        assert list(ex[3][win[:2], 0]) == [0.25, 0.75] and win[2] == -1


def known_pose_case(origin=(0.0, 0.0, 0.0)):
    """the map points (world, float64), the true pose, the queries and the start: tests/test_gpu_local_map.py uses the same"""
    origin = np.asarray(origin, np.float64)
    pts = L.three_planes() + origin
    axis, shift = np.array([0.6, -0.5, 0.62]), np.array([0.2, -0.1, 0.2])
    true = I.se3(axis / np.linalg.norm(axis) * np.radians(2.0), origin + shift * (0.3 / np.linalg.norm(shift)))
    start = np.eye(4)
    start[:3, 3] = origin
    return pts, true, I.moved(pts, true), start


def pose_error(P, Q):
    dR = P[:3, :3].T @ Q[:3, :3]
    return float(np.linalg.norm(P[:3, 3] - Q[:3, 3])), float(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))


@pytest.mark.parametrize("origin", [(0.0, 0.0, 0.0), (1000.0, -500.0, 20.0)])
def test_known_pose_converges_in_float64(origin):
    pts, true, src, start = known_pose_case(origin)
    assert 900 <= len(pts) <= 1100
    m = L.Map(1.0, 3, origin, 0.0, 100.0, np.float64)
    m.insert((pts - np.asarray(origin)).astype(np.float32), np.arange(len(pts)), start, 0)
    assert len(m.export()[0]) == len(pts)
    r = L.register(src, m.export(), m.voxel, 3, m.origin, start, [(1.0, 40)], dtype=np.float64)
    dt, dr = pose_error(r["pose"], true)
    assert r["status"] == L.CONVERGED and dt < 1e-5 and dr < 1e-5, (r, dt, dr)   # a tenth of the GPU test's bound


def test_restated_odometry_follows_a_moving_sensor():
    """a sensor sliding through a random cloud: every frame sees the points within 12 m, exactly (no noise).  Points that
    come into range have no partner in the map yet and match a stranger up to a voxel away: the robust kernel is what keeps
    them from pulling the pose (unweighted the same run is 7 mm off)."""
    rng = np.random.default_rng(3)
    world = rng.uniform(-20, 20, (6000, 3)) * [1, 1, 0.2]
    truth = [I.se3([0, 0, 0.01 * k], [0.4 * k, 0.05 * k, 0]) for k in range(5)]
    frames = []
    for P in truth:
        loc = I.moved(world, P)
        frames.append(loc[np.linalg.norm(loc, axis=1) < 12])
    poses, statuses, m = L.odometry(frames, max_range=15.0, kernel_scale=0.1, dtype=np.float64)
    assert all(s in (L.CONVERGED, L.MAX_ITER) for s in statuses)
    assert max(pose_error(P, Q)[0] for P, Q in zip(poses, truth)) < 1e-3
    assert len(m.export()[0]) > 1000


# ------------------------------------------------------------------------------------------------------------ the C ABI
NAMES = ["dpm_local_map_bytes", "dpm_local_map_init", "dpm_local_map_insert", "dpm_local_map_prune", "dpm_local_map_register",
         "dpm_local_map_export"]


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    from deeppointmap_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    EINVAL = -1
    assert lib.dpm_local_map_bytes(64, 3) == 256 + 2 * (64 * 8 + 64 * 27 * 24)
    for cap_vox, s in [(0, 3), (1, 3), (63, 3), (64, 0), (64, 4), (1 << 25, 1)]:
        assert lib.dpm_local_map_bytes(cap_vox, s) == 0
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) & ~255   # never dereferenced: every call below is refused first
    o = (ctypes.c_double * 3)(0, 0, 0)
    oa = ctypes.addressof(o)
    bad_o = (ctypes.c_double * 3)(0, float("nan"), 0)
    dist, iters = (ctypes.c_double * 1)(1.0), (ctypes.c_int32 * 1)(5)
    da, ia = ctypes.addressof(dist), ctypes.addressof(iters)
    assert lib.dpm_local_map_init(None, 64, 3, None) == EINVAL and lib.dpm_local_map_init(p, 48, 3, None) == EINVAL
    assert lib.dpm_local_map_init(p + 8, 64, 3, None) == EINVAL
    ins = lambda **k: lib.dpm_local_map_insert(*[{**dict(map=p, cap_vox=64, s=3, half=0, voxel=1.0, origin=oa, xyz=p, idx=p, count=p,
                                                         cap=8, pose=p, stamp=0, lo=0.0, hi=10.0, stream=None), **k}[n]
                                                  for n in ("map", "cap_vox", "s", "half", "voxel", "origin", "xyz", "idx", "count",
                                                            "cap", "pose", "stamp", "lo", "hi", "stream")])
    for k in (dict(map=None), dict(cap_vox=65), dict(s=4), dict(half=2), dict(voxel=0.0), dict(voxel=float("nan")), dict(origin=None),
              dict(origin=ctypes.addressof(bad_o)), dict(xyz=None), dict(idx=None), dict(count=None), dict(cap=-1), dict(pose=None),
              dict(stamp=0xFFFFFFFF), dict(lo=-1.0), dict(lo=11.0), dict(hi=float("inf"))):
        assert ins(**k) == EINVAL, k
    pr = lambda **k: lib.dpm_local_map_prune(*[{**dict(map=p, cap_vox=64, s=3, half=0, voxel=1.0, origin=oa, pose=p, radius=5.0,
                                                       stream=None), **k}[n]
                                               for n in ("map", "cap_vox", "s", "half", "voxel", "origin", "pose", "radius", "stream")])
    for k in (dict(map=None), dict(half=-1), dict(pose=None), dict(radius=-1.0), dict(radius=float("nan")), dict(voxel=-1.0)):
        assert pr(**k) == EINVAL, k
    order = ("map", "cap_vox", "s", "half", "voxel", "origin", "xyz", "count", "cap", "init", "dist", "iters", "n", "ks", "tr", "tt",
             "pose", "fit", "rmse", "it", "st", "dk", "ds", "dsys", "ws", "stream")
    base = dict(map=p, cap_vox=64, s=3, half=0, voxel=1.0, origin=oa, xyz=p, count=p, cap=8, init=p, dist=da, iters=ia, n=1, ks=0.0,
                tr=1e-7, tt=1e-6, pose=p + 512, fit=p, rmse=p, it=p, st=p, dk=None, ds=None, dsys=None, ws=p, stream=None)
    reg = lambda **k: lib.dpm_local_map_register(*[{**base, **k}[n] for n in order])
    far = (ctypes.c_double * 1)(1.5)
    for k in (dict(map=None), dict(xyz=None), dict(count=None), dict(cap=0), dict(init=None), dict(dist=None), dict(iters=None),
              dict(n=0), dict(n=17), dict(ks=-1.0), dict(tr=-1.0), dict(tt=-1.0), dict(pose=None), dict(pose=p), dict(fit=None),
              dict(st=None), dict(ws=None), dict(dist=ctypes.addressof(far)), dict(voxel=0.5)):
        assert reg(**k) == EINVAL, k
    ex = lambda **k: lib.dpm_local_map_export(*[{**dict(map=p, cap_vox=64, s=3, half=0, keys=p, sub=p, owner=p, xyz=p, count=p, n=4,
                                                        stream=None), **k}[n]
                                                for n in ("map", "cap_vox", "s", "half", "keys", "sub", "owner", "xyz", "count", "n",
                                                          "stream")])
    for k in (dict(map=None), dict(half=3), dict(count=None), dict(n=-1), dict(keys=None), dict(xyz=None)):
        assert ex(**k) == EINVAL, k


def test_python_layer_refuses_before_the_gpu():
    from deeppointmap_amd import odometry
    with pytest.raises(ValueError):
        odometry.LocalMap(max_voxels=100)
    with pytest.raises(ValueError):
        odometry.LocalMap(subdivisions=4)
    with pytest.raises(ValueError):
        odometry.LidarOdometry(voxel_size=1.0, schedule=((1.5, 10),))
    with pytest.raises(ValueError):
        odometry.LidarOdometry(deskew=True, time="column")
    odo = odometry.LidarOdometry()
    assert np.array_equal(odo.predicted_motion(), np.eye(4)) and np.array_equal(odo.predicted_pose(), np.eye(4))
    odo.poses = [np.eye(4), I.se3([0, 0, 0.1], [1, 0, 0])]
    assert np.allclose(odo.predicted_pose(), odo.poses[1] @ odo.poses[1]) and callable(odo.predicted_motion)
