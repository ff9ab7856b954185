"""GPU: the simulator with sweep motion (dpm_lidar_cull_sweep / dpm_lidar_cast_sweep in csrc/lidar_sim.hip) against this
project's own restatement (tests/lidar_sweep_restated.py); the reference has no counterpart.

* standing still (end pose == start pose) the sweep entry points give the static ones' bytes;
* the column table against float64: every entry within one float32 ulp;
* the cast against the float32 restatement FED the device's table: bit for bit;
* the cast against the independent float64 form (one world pose per column): 1 mm, the simulator's bound, and equal ids on
  every unambiguous ray, at most 1 % ambiguous.

Every observed figure goes to test_logs/lidar_sweep_errors.log.
"""
import numpy as np
import pytest
import torch

import lidar_sim_cases as C
import lidar_sim_restated as RS
import lidar_sweep_cases as SC
import lidar_sweep_restated as SW

pytestmark = pytest.mark.gpu
DEV = "cuda"
T_BOUND = 1e-3
AMBIGUOUS_CAP = 0.01


def mods():
    from deeppointmap_amd import augment, lidar_sim, ops
    return lidar_sim, ops, augment


def bits(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.tobytes()


def differing(name, got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    bad = got.view(np.int32) != want.view(np.int32) if got.dtype == np.float32 else got != want
    worst = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()) if got.size else 0.0
    SC.log(f"sweep kernel vs float32 restatement, {name}: {int(bad.sum())} of {bad.size} entries differ, max difference {worst:.3e}")
    return int(bad.sum())


# ---------------------------------------------------------------------------------------------------------------- standing still
def test_a_sensor_that_stands_still_gives_the_static_entry_points_bytes():
    LS, ops, _ = mods()
    scene, poses = C.scene_600()
    m = C.MODEL_385
    sd = scene.to_device(DEV)
    static = LS.cast_rays(sd, poses, m)
    moving = LS.cast_rays(sd, poses, m, poses_end=poses.copy())
    assert static.table is None and moving.table.shape == (3, m.azimuth_steps, 12)
    want = np.tile(np.r_[np.eye(3).reshape(9), np.zeros(3)].astype(np.float32), (3, m.azimuth_steps, 1))
    assert np.array_equal(moving.table.cpu().numpy(), want)                       # exactly identity and zero
    assert bits(moving.status) == bits(static.status)
    for name, a, b in zip(("range", "prim", "cos_inc"), moving, static):
        assert bits(a) == bits(b), name
    assert (static[1].cpu().numpy() >= 0).mean() > 0.3
    frames = LS.LidarSimulator(sd, m).frames(poses)
    assert all(f.sweep_motion is None for f in frames)


# ---------------------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("A", [1, 255, 512])
def test_the_column_table_against_float64(A):
    LS, ops, _ = mods()
    scene = C.random_scene(3, 1, 5.0)
    sd = scene.to_device(DEV)
    far = C.pose(1000.0, -1000.0, 1.8, yaw=2.3, pitch=0.07, roll=-0.05)
    near = C.pose(2.0, 3.0, 1.7, yaw=-0.4, pitch=0.02, roll=0.01)
    # the angle of 1e-9 from an axis-aligned pose: P0^-1 P1 is then free of rounding, and the entries compared are the
    # table's.  Behind a turned P0 the products of float64 leave 1e-16 in the entries of R_D that the motion leaves at zero;
    # the kernel and numpy sum them in different orders, and one ulp of such an entry measures that noise, not the table.
    flat = C.pose(2.0, 3.0, 1.7)
    P0 = np.stack([near, near, flat, far])
    P1 = np.stack([near @ SC.ZERO, near @ SC.CORNER, flat @ SC.TINY, far @ SC.CORNER])
    *_, table = ops.lidar_cull_sweep(sd.prims, sd.kind, sd.ground, torch.from_numpy(P0).to(DEV), torch.from_numpy(P1).to(DEV),
                                     A, 50.0, 1)
    got = table.cpu().numpy()
    assert got.shape == (4, A, 12) and np.isfinite(got).all()
    for f, name in enumerate(("zero motion", "0.25 rad corner", "angle 1e-9", "corner, 1 km from the origin")):
        want = SW.table64(P0[f], P1[f], A)
        w32 = want.astype(np.float32)
        err = np.abs(got[f].astype(np.float64) - want)
        ulp = np.spacing(np.abs(w32)).astype(np.float64)
        n_diff = int((got[f].view(np.int32) != w32.view(np.int32)).sum())
        SC.log(f"column table vs float64, {name}, A = {A}: {n_diff} of {want.size} entries differ from the rounded float64 value, "
               f"largest error {float((err / ulp).max()):.3f} ulp")
        assert (err <= ulp).all()
    assert np.array_equal(got[0], np.tile(np.r_[np.eye(3).reshape(9), np.zeros(3)].astype(np.float32), (A, 1)))
    assert np.array_equal(got[:, 0], np.tile(np.r_[np.eye(3).reshape(9), np.zeros(3)].astype(np.float32), (4, 1)))   # s_0 = 0


# ---------------------------------------------------------------------------------------------------------------- float32
def sweep_models(LS):
    return [LS.LidarModel([0.0], 1, 0.9, 40.0), LS.LidarModel(np.linspace(6.0, -20.0, 3), 85, 0.9, 40.0),
            LS.LidarModel(np.linspace(6.0, -20.0, 3), 86, 0.9, 40.0), LS.SMALL16]


@pytest.mark.parametrize("P", [0, 1, 64, 65, 130])
def test_the_sweep_cast_equals_the_float32_restatement_bit_for_bit(P):
    LS, ops, _ = mods()
    scene = C.random_scene(20 + P, P, 18.0)
    P0 = np.stack([C.free_pose(scene, 1.0, -2.0, 1.7, yaw=0.4, pitch=0.05, roll=-0.08),
                   C.free_pose(scene, -6.0, 5.0, 2.1, yaw=-2.1, pitch=-0.06, roll=0.04)])
    P1 = np.stack([P0[0] @ SC.CORNER, P0[1] @ np.linalg.inv(SC.CORNER)])
    prims, kind, ground, _, _ = scene.arrays()
    sd = scene.to_device(DEV)
    bad = 0
    for m in sweep_models(LS):
        assert m.rays in (1, 255, 258, 8192)
        cast = LS.cast_rays(sd, P0, m, poses_end=P1)
        table = cast.table.cpu().numpy()
        counts = cast.status.cpu().numpy()
        for f in range(2):
            cull = SW.cull_sweep(prims, kind, ground, P0[f], P1[f], m.max_range)
            assert counts[f].tolist() == [len(cull[1]), 0]
            want = SW.cast32_sweep(*cull, scene.P, m.directions(), table[f], m.min_range, m.max_range)
            for name, g, w in zip(("range", "prim", "cos_inc"), cast, want):
                bad += differing(f"P = {P}, {m.beams} x {m.azimuth_steps} rays, frame {f}, {name}", g[f], w)
        if P >= 64 and m.rays > 255:
            prim = cast[1].cpu().numpy()
            assert len(np.unique(prim)) > 10 and (prim == scene.P).any()
    assert bad == 0


# ---------------------------------------------------------------------------------------------------------------- float64
def test_the_sweep_cast_against_float64_one_kilometre_from_the_origin():
    LS, _, _ = mods()
    scene, P0, P1, m = SC.far_sweep()
    dirs, A = m.directions(), m.azimuth_steps
    rng, prim, _ = (t.cpu().numpy() for t in LS.cast_rays(scene.to_device(DEV), P0, m, poses_end=P1))
    worst, n_amb, n = 0.0, 0, 0
    for f in range(2):
        r64, p64, _ = SW.cast64_sweep(scene.params, scene.kind, scene.z0, P0[f], P1[f], dirs, A, m.min_range, m.max_range)
        amb = SW.ambiguous_sweep(scene.params, scene.kind, scene.z0, P0[f], P1[f], dirs, A, m.min_range, m.max_range, p64)
        ok = ~amb
        n_amb, n = n_amb + int(amb.sum()), n + len(amb)
        wrong = int((prim[f][ok] != p64[ok]).sum())
        same = ok & (prim[f] == p64)
        err = float(np.abs(rng[f][same].astype(np.float64) - r64[same]).max())
        SC.log(f"sweep kernel vs float64, 1 km from the origin, frame {f}: {len(amb)} rays, {int(amb.sum())} ambiguous, {wrong} ids "
               f"differ, max |t - t64| = {err:.3e} m (bound {T_BOUND:.0e}), {(p64 >= 0).mean():.2f} of the rays return")
        assert wrong == 0 and (p64 >= 0).mean() > 0.3
        worst = max(worst, err)
    assert n_amb <= AMBIGUOUS_CAP * n and worst <= T_BOUND


# ---------------------------------------------------------------------------------------------------------------- reach
def test_a_box_only_the_moving_sensor_brings_within_max_range_returns():
    """four columns, one beam, max_range 10: the sensor slides 8 m along -y; column 3 looks along -y at s = 0.75, from
    (0, -6, 0).  The box's face at y = -15.5 is 15.5 m from the start pose (beyond max_range plus the box) and 9.5 m from there."""
    LS, _, _ = mods()
    scene = LS.Scene(z0=None)
    scene.add_box((0.0, -16.5, 0.0), (1.0, 1.0, 1.0))
    m = LS.LidarModel([0.0], 4, 0.5, 10.0)
    P0 = np.eye(4)[None]
    P1 = P0.copy()
    P1[0, 1, 3] = -8.0
    sd = scene.to_device(DEV)
    static = LS.cast_rays(sd, P0, m)
    assert static.status.cpu().tolist() == [[0, 0]] and static[1].cpu().tolist() == [[-1] * 4]
    moving = LS.cast_rays(sd, P0, m, poses_end=P1)
    assert moving.status.cpu().tolist() == [[1, 0]]
    assert moving[1].cpu().tolist() == [[-1, -1, -1, 0]]
    assert abs(float(moving[0][0, 3]) - 9.5) < 1e-5 and abs(float(moving[2][0, 3]) - 1.0) < 1e-6


# ---------------------------------------------------------------------------------------------------------------- overflow
def test_overflow_of_max_kept_still_raises_at_the_read_back():
    LS, ops, augment = mods()
    scene, poses = C.scene_600()
    m = C.MODEL_385
    P1 = poses @ SC.CORNER
    prims, kind, ground, _, _ = scene.arrays()
    counts = [len(SW.cull_sweep(prims, kind, ground, a, b, m.max_range)[1]) for a, b in zip(poses, P1)]
    most = max(counts)
    assert most > 64 and counts[0] >= RS.kept_counts(prims, kind, ground, poses[:1], m.max_range)[0]
    sd = scene.to_device(DEV)
    cast = LS.cast_rays(sd, poses, m, max_kept=most - 1, poses_end=P1)
    assert cast.status.cpu().tolist() == [[n, int(n > most - 1)] for n in counts]
    with pytest.raises(ValueError, match="max_kept"):
        cast.check()
    LS.cast_rays(sd, poses, m, max_kept=most, poses_end=P1).check()
    frames = LS.LidarSimulator(sd, m, max_kept=most - 1).frames(poses, poses_end=P1)
    with pytest.raises(ValueError, match="max_kept"):
        frames[0].check()
    frames = LS.LidarSimulator(sd, m, max_kept=most - 1).frames(poses, poses_end=P1)
    with pytest.raises(ValueError, match="max_kept"):
        augment.collate_frames(frames, padding_to=m.rays)


# ---------------------------------------------------------------------------------------------------------------- determinism
def test_two_runs_and_a_graph_replay_give_identical_bytes():
    LS, ops, _ = mods()
    scene, poses = C.scene_600()
    m = C.MODEL_385
    sd = scene.to_device(DEV)
    dirs = torch.from_numpy(m.directions()).to(DEV)
    d0, d1 = torch.from_numpy(poses).to(DEV), torch.from_numpy(poses @ SC.CORNER).to(DEV)

    def run():
        kept, plane, status, table = ops.lidar_cull_sweep(sd.prims, sd.kind, sd.ground, d0, d1, m.azimuth_steps, m.max_range, scene.P)
        cast = ops.lidar_cast_sweep(kept, plane, status, table, scene.P, dirs, m.min_range, m.max_range)
        return (table,) + cast + ops.lidar_emit(*cast, dirs, sd.albedo, sd.class_id)
    eager = [bits(t) for t in run()]
    assert [bits(t) for t in run()] == eager
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = run()
    for t in captured:
        t.fill_(0) if t.dtype != torch.float32 else t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert [bits(t) for t in captured] == eager
    # the class layer: raw frames under the start pose, carrying the motion
    frames = LS.LidarSimulator(sd, m).frames(poses, poses_end=poses @ SC.CORNER)
    for f, pcd in enumerate(frames):
        assert np.abs(pcd.sweep_motion - SC.CORNER).max() < 1e-12 and pcd.sweep_motion.dtype == np.float64
        assert np.array_equal(pcd.R.numpy(), poses[f, :3, :3].astype(np.float32))
        assert np.array_equal(pcd.T.numpy(), poses[f, :3, 3:].astype(np.float32))
