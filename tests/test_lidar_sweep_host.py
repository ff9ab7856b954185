"""CPU: the sweep-motion model (deeppointmap_amd/lidar_sim.py's docstring) on the host and in the float64
restatement (tests/lidar_sweep_restated.py): its algebra, `sweep_poses`, and the experiment that says the model is sound and
its effect large -- raw points of a moving SMALL16 sensor lie decimetres off their surfaces, the same points deskewed with
the true motion lie ON them (1e-9 m) at any reference time, and a point's own azimuth names its column without exception."""
import ctypes

import numpy as np
import pytest

import lidar_sim_cases as C
import lidar_sim_restated as RS
import lidar_sweep_cases as SC
import lidar_sweep_restated as SW
import map_eval_restated as ME
from deeppointmap_amd import lidar_sim as LS


# ---------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("name", list(SC.MOTIONS))
def test_the_motion_starts_at_identity_ends_at_D_and_a_change_of_reference_composes(name):
    D = SC.MOTIONS[name]
    assert np.array_equal(LS.motion_at(D, 0.0), np.eye(4))
    assert np.abs(LS.motion_at(D, 1.0) - D).max() < 1e-15
    for s in (0.0, 0.3, 1.0):      # the package's host functions and the restatement are one model
        assert np.abs(LS.motion_at(D, s) - SW.motion64(D, s)).max() < 1e-15
    assert np.abs(LS.sweep_delta(C.pose(3, 4, 5, yaw=1.0), C.pose(3, 4, 5, yaw=1.0) @ D) - D).max() < 1e-14
    g = np.random.default_rng(1)
    p, s = g.uniform(-100, 100, (50, 3)), g.random(50)
    a = SW.deskew64(p, s, D, 0.25)
    # the points deskewed to 0.25 are measurements of a sensor standing at D(0.25): moving them on to 0.8 is one rigid map
    hop = np.linalg.inv(SW.motion64(D, 0.8)) @ SW.motion64(D, 0.25)
    assert np.abs(a @ hop[:3, :3].T + hop[:3, 3] - SW.deskew64(p, s, D, 0.8)).max() < 1e-12
    assert np.abs(SW.deskew64(p, np.full(50, 0.6), D, 0.6) - p).max() < 1e-12       # a point fired at the reference time stays
    # constant rate: D(s) D(t) = D(s + t) for the rotation, and the origin moves on a straight line
    assert np.abs(SW.exp64(SW.log64(D[:3, :3]), 0.3) @ SW.exp64(SW.log64(D[:3, :3]), 0.45) - SW.exp64(SW.log64(D[:3, :3]), 0.75)).max() < 1e-15


def test_tiny_and_zero_angles_have_no_zero_over_zero():
    for D in (SC.TINY, SC.ZERO):
        t = SW.table64(np.eye(4), D, 7)
        assert np.isfinite(t).all() and np.isfinite(LS.motion_at(D, 0.5)).all()
    assert np.array_equal(SW.table64(C.pose(1, 2, 3, yaw=0.7, pitch=0.1), C.pose(1, 2, 3, yaw=0.7, pitch=0.1), 5),
                          np.tile(np.r_[np.eye(3).reshape(9), np.zeros(3)], (5, 1)))
    assert abs(SW.log64(SC.TINY[:3, :3])[2] - 1e-9) < 1e-24


def test_sweep_poses():
    poses = LS.circuit(LS.street_scene(2), spacing=1.5)
    P0, P1 = LS.sweep_poses(poses)
    assert P0.shape == P1.shape == poses.shape and np.array_equal(P0, poses) and np.array_equal(P1[:-1], poses[1:])
    want = poses[-1] @ (np.linalg.inv(poses[-2]) @ poses[-1])        # the last frame goes on by its previous delta
    assert np.abs(P1[-1] - want).max() < 1e-12
    one0, one1 = LS.sweep_poses(poses[:1])
    assert np.array_equal(one0, one1)
    travel = [SW.travel64(a, b) for a, b in zip(P0, P1)]
    assert 1.4 < min(travel) and max(travel) < 1.6


# ---------------------------------------------------------------------------------------------------------------- the casts
def test_the_per_ray_float64_cast_is_cast64_dirs_column_by_column():
    scene, P0, P1, m = SC.far_sweep()
    dirs, A = m.directions(), m.azimuth_steps
    r, p, c = SW.cast64_sweep(scene.params, scene.kind, scene.z0, P0[0], P1[0], dirs, A, m.min_range, m.max_range)
    poses = SW.column_poses64(P0[0], P1[0], A)
    for col in (0, 1, 77, A - 1):
        rays = np.arange(col, m.rays, A)
        want = RS.cast64(scene.params, scene.kind, scene.z0, poses[col], dirs[rays], m.min_range, m.max_range)
        assert np.array_equal(r[rays], want[0]) and np.array_equal(p[rays], want[1]) and np.array_equal(c[rays], want[2])
    assert np.abs(poses[0] - P0[0]).max() == 0 and (p >= 0).mean() > 0.3


def test_the_float32_sweep_cast_with_an_identity_table_is_the_static_cast():
    scene, poses = C.scene_600()
    m = C.MODEL_385
    prims, kind, ground, _, _ = scene.arrays()
    table = SW.table64(poses[0], poses[0], m.azimuth_steps).astype(np.float32)
    cull = SW.cull_sweep(prims, kind, ground, poses[0], poses[0], m.max_range)
    got = SW.cast32_sweep(*cull, scene.P, m.directions(), table, m.min_range, m.max_range)
    want = RS.cast32(*RS.cull(prims, kind, ground, poses[0], m.max_range), scene.P, m.directions(), m.min_range, m.max_range)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


def test_the_float32_sweep_cast_against_float64_and_the_ambiguity_cap_of_the_chosen_poses():
    """what tests/test_gpu_lidar_sweep.py asks of the kernel, asked of the float32 restatement first: 1 mm, equal ids on
    unambiguous rays, at most 1 % of the rays ambiguous"""
    scene, P0, P1, m = SC.far_sweep()
    prims, kind, ground, _, _ = scene.arrays()
    dirs, A = m.directions(), m.azimuth_steps
    n_amb = n = 0
    for f in range(2):
        r64, p64, _ = SW.cast64_sweep(scene.params, scene.kind, scene.z0, P0[f], P1[f], dirs, A, m.min_range, m.max_range)
        amb = SW.ambiguous_sweep(scene.params, scene.kind, scene.z0, P0[f], P1[f], dirs, A, m.min_range, m.max_range, p64)
        table = SW.table64(P0[f], P1[f], A).astype(np.float32)
        r32, p32, _ = SW.cast32_sweep(*SW.cull_sweep(prims, kind, ground, P0[f], P1[f], m.max_range), scene.P, dirs, table,
                                      m.min_range, m.max_range)
        ok = ~amb
        same = ok & (p32 == p64)
        err = float(np.abs(r32[same].astype(np.float64) - r64[same]).max())
        SC.log(f"float32 restatement vs float64, sweep, frame {f}: {int(amb.sum())} of {len(amb)} rays ambiguous, "
               f"{int((p32[ok] != p64[ok]).sum())} ids differ, max |t - t64| = {err:.3e} m")
        assert (p32[ok] == p64[ok]).all() and err <= 1e-3 and (p64 >= 0).mean() > 0.3
        n_amb, n = n_amb + int(amb.sum()), n + len(amb)
    assert n_amb <= 0.01 * n


# ---------------------------------------------------------------------------------------------------------------- the experiment
def test_raw_points_miss_their_surfaces_and_deskewed_points_lie_on_them():
    scene, P0, P1, m = SC.street_sweep()
    P0, P1 = P0[0], P1[0]
    dirs, A = m.directions(), m.azimuth_steps
    rng, prim, _ = SW.cast64_sweep(scene.params, scene.kind, scene.z0, P0, P1, dirs, A, m.min_range, m.max_range)
    hit = prim >= 0
    raw = rng[hit, None] * dirs[hit].astype(np.float64)            # t * dir: the sensor's frame at the ray's own time
    s = SW.column_fraction(np.nonzero(hit)[0], A)
    D = SW.delta64(P0, P1)
    world = lambda p, M: M[:3, :3] @ p.T + M[:3, 3:]
    off = ME.scene_distance64(scene.params, scene.kind, scene.z0, world(raw, P0))[0]
    share = float((off > 0.01).mean())
    worst = 0.0
    for s_ref in (0.0, 0.5, 1.0):
        fixed = SW.deskew64(raw, s, D, s_ref)
        worst = max(worst, float(ME.scene_distance64(scene.params, scene.kind, scene.z0, world(fixed, P0 @ SW.motion64(D, s_ref)))[0].max()))
    SC.log(f"host experiment, street_scene(2) frame 7, SMALL16, {int(hit.sum())} returns: raw under the start pose max {off.max():.3f} m "
           f"off, {100 * share:.1f} % beyond 1 cm; deskewed with the true motion max {worst:.2e} m at s_ref 0, 0.5, 1")
    assert hit.sum() > 4000 and worst <= 1e-9 and share > 0.10
    # the column from the point's own azimuth, float32 as the kernel computes it: no exception
    raw32 = (rng[hit].astype(np.float32)[:, None] * dirs[hit])
    assert np.array_equal(SW.azimuth_column32(raw32, A), np.nonzero(hit)[0] % A)
    assert SW.azimuth_column32(raw32[np.nonzero(hit)[0] % A == 0], A).tolist() == [0] * int((np.nonzero(hit)[0] % A == 0).sum())


# ---------------------------------------------------------------------------------------------------------------- the entry point
def test_deskew_refuses_bad_arguments_before_it_touches_a_device():
    """DPM_EINVAL (-1) comes back from the argument checks: no GPU is needed to see it, so nothing was launched"""
    from deeppointmap_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 12)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    D = (ctypes.c_double * 16)(*SC.CORNER.reshape(-1))
    Dp = ctypes.cast(D, ctypes.c_void_p)
    call = lambda *a: lib.dpm_points_deskew(*a, None)
    assert call(None, ptr, ptr, 4, 0, None, 0, 8, Dp, 0.0) == -1            # no points
    assert call(ptr, ptr, None, 4, 0, None, 0, 8, Dp, 0.0) == -1            # no count
    assert call(ptr, ptr, ptr, 0, 0, None, 0, 8, Dp, 0.0) == -1             # capacity 0
    assert call(ptr, ptr, ptr, 4, 3, None, 0, 8, Dp, 0.0) == -1             # no such time mode
    assert call(ptr, ptr, ptr, 4, 0, None, 0, 0, Dp, 0.0) == -1             # column mode without columns
    assert call(ptr, None, ptr, 4, 0, None, 0, 8, Dp, 0.0) == -1            # column mode without idx
    assert call(ptr, ptr, ptr, 4, 1, None, 0, -1, Dp, 0.0) == -1            # negative azimuth_steps
    assert call(ptr, ptr, ptr, 4, 2, None, 0, 0, Dp, 0.0) == -1             # times mode without times
    assert call(ptr, ptr, ptr, 4, 2, ptr, 0, 0, Dp, 0.0) == -1              # ... or with an empty table
    assert call(ptr, ptr, ptr, 4, 0, None, 0, 8, None, 0.0) == -1           # no motion
    assert call(ptr, ptr, ptr, 4, 0, None, 0, 8, Dp, 1.5) == -1             # reference outside the sweep
    assert call(ptr, ptr, ptr, 4, 0, None, 0, 8, Dp, float("nan")) == -1
    bad = (ctypes.c_double * 16)(*([float("inf")] + [0.0] * 15))
    assert call(ptr, ptr, ptr, 4, 0, None, 0, 8, ctypes.cast(bad, ctypes.c_void_p), 0.0) == -1
    # the simulator's two new entry points check theirs too
    assert lib.dpm_lidar_cull_sweep(None, None, 0, None, None, None, 1, 8, 10.0, 1, None, None, None, None, None) == -1
    assert lib.dpm_lidar_cast_sweep(ptr, ptr, ptr, 1, 0, ptr, 4, 1, ptr, 3, 0.5, 10.0, ptr, ptr, ptr, None) == -1   # 4 rays, 3 columns
    assert lib.dpm_lidar_cast_sweep(ptr, ptr, ptr, 1, 0, ptr, 4, 1, None, 2, 0.5, 10.0, ptr, ptr, ptr, None) == -1  # no table


def test_the_class_layer_without_a_gpu():
    from deeppointmap_amd import augment
    t = augment.Deskew("frame", time="column", azimuth_steps=512, reference=0.5)
    assert repr(t) == "Deskew(motion=frame, time=column, azimuth_steps=512, reference=0.5)"
    assert augment.PointCloud.sweep_motion is None
    a, b = C.pose(0, 0, 0), C.pose(1.5, 0, 0, yaw=0.1)
    assert np.abs(augment.constant_velocity_motion(a, b) - np.linalg.inv(a) @ b).max() < 1e-15
