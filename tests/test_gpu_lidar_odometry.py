"""GPU: the geometric odometry end to end (deeppointmap_amd/odometry.py) on simulated frames with exact poses, against the
numpy restatement (tests/lidar_odometry_restated.py) run on the same frames in float32 and float64.

The scene is lidar_sim.street_scene(2) seen by 16 beams x 256 columns from the first 12 poses of its circuit at about 1 m
spacing, without range noise or drops.  Every pose must lie within max(3 |r32 - r64|, 1 mm) of the float64 restatement's, and
the ATE rmse against the exact poses (evaluate.ate) within twice the float64 restatement's plus 1 mm: an fp32 search may
choose differently at near-ties, and a different match set moves every later frame.  Observed on MI355X: see
profiles/lidar_odometry_accuracy.md, generated from what these tests log.  With sweep motion and deskew=True the run must
work, leave the caller's frames alone and synchronise once per step; raw against deskewed ATE is logged, not asserted.

The motion between the first two frames is GIVEN (LidarOdometry(initial_motion=...)): 80 % of this sensor's returns are rings
on flat ground, which travel with the sensor, and from a start one metre off the second frame settles on "no motion" --
restatement and GPU alike (ATE rmse 3.39 m each over these 12 frames, which the factor-2 check passes without saying
anything).  With it the run follows the circuit and the check compares two working odometries.
"""
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lidar_odometry_restated as L  # noqa: E402
from test_gpu_local_map import log  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FRAMES = 12
KW = dict(voxel_size=1.0, subdivisions=3, schedule=((1.0, 30),), kernel_scale=0.1, min_range=0.0)


@pytest.fixture(scope="module")
def world():
    from deeppointmap_amd import lidar_sim as LS
    scene = LS.street_scene(2)
    model = LS.LidarModel(np.linspace(10.0, -20.0, 16), 256, 0.9, 80.0, range_sigma=0.0, drop_prob=0.0)
    poses = LS.circuit(scene, spacing=1.0)[:FRAMES]
    sim = LS.LidarSimulator(scene, model, device=DEV)
    # the speed the vehicle starts with is given: over flat ground this sensor's second frame cannot find it (module docstring)
    first = dict(first_pose=poses[0], initial_motion=LS.sweep_delta(poses[0], poses[1]))
    return SimpleNamespace(scene=scene, model=model, poses=poses, sim=sim, first=first)


def host_rows(frames):
    return [f.xyz[:int(f.count.item())].cpu().numpy() for f in frames]


@pytest.fixture(scope="module")
def runs(world):
    """the GPU run and both restatements of the static circuit, computed once"""
    from deeppointmap_amd.odometry import LidarOdometry
    frames = world.sim.frames(world.poses)
    odo = LidarOdometry(max_range=world.model.max_range, **world.first, **KW)
    steps = [odo.step(f) for f in frames]
    rows = host_rows(frames)
    out = SimpleNamespace(odo=odo, steps=steps, gpu=np.stack(odo.poses), rows=rows)
    for name, dtype in (("r32", np.float32), ("r64", np.float64)):
        t = time.time()
        poses, statuses, m = L.odometry(rows, KW["voxel_size"], KW["subdivisions"], world.model.max_range, KW["min_range"],
                                        KW["schedule"], KW["kernel_scale"], world.poses[0], dtype,
                                        initial_motion=world.first["initial_motion"])
        setattr(out, name, poses)
        setattr(out, name + "_status", statuses)
        log(f"end to end: restatement {name} of {FRAMES} frames ({sum(map(len, rows))} points) in {time.time() - t:.1f} s, "
            f"statuses {statuses}, map {len(m.export()[0])} points")
    return out


def test_every_frame_registers(world, runs):
    assert len(runs.steps) == FRAMES and np.array_equal(runs.gpu[0], world.poses[0])
    assert all(s.status in (L.CONVERGED, L.MAX_ITER) for s in runs.steps), [s.status for s in runs.steps]
    assert all(s in (L.CONVERGED, L.MAX_ITER) for s in runs.r64_status)
    assert np.isfinite(runs.gpu).all() and all(s.fitness > 0.5 for s in runs.steps[1:])
    log("end to end: GPU statuses " + str([s.status for s in runs.steps]) + ", iterations " + str([s.iterations for s in runs.steps])
        + ", fitness " + " ".join(f"{s.fitness:.2f}" for s in runs.steps))
    assert runs.odo.local_map.overflow == 0 and runs.odo.local_map.n_points > 1000


def test_every_pose_is_the_restatements(world, runs):
    worst = 0.0
    for k in range(FRAMES):
        spread = np.abs(runs.r32[k] - runs.r64[k]).max()
        err = np.abs(runs.gpu[k] - runs.r64[k]).max()
        bound = max(3 * spread, 1e-3)
        worst = max(worst, err / bound)
        log(f"end to end frame {k}: |gpu - r64| {err:.3e}, |r32 - r64| {spread:.3e}, |gpu - r32| {np.abs(runs.gpu[k] - runs.r32[k]).max():.3e}, "
            f"|gpu - exact| {np.linalg.norm(runs.gpu[k][:3, 3] - world.poses[k][:3, 3]):.3e} m")
        assert err <= bound, (k, err, bound)
    log(f"end to end: worst |gpu - r64| / max(3 |r32 - r64|, 1 mm) over {FRAMES} frames {worst:.3e}")


def test_ate_against_the_exact_poses(world, runs):
    from deeppointmap_amd import evaluate
    a_gpu, a_64, a_32 = (evaluate.ate(p, world.poses)["rmse"] for p in (runs.gpu, runs.r64, runs.r32))
    log(f"end to end: ATE rmse against the exact poses: GPU {a_gpu:.4e} m, restatement float64 {a_64:.4e} m, float32 {a_32:.4e} m "
        f"(bound: 2 x float64 + 1 mm = {2 * a_64 + 1e-3:.4e} m)")
    assert a_gpu <= 2 * a_64 + 1e-3


def test_sweep_motion_with_deskew_runs_and_leaves_the_frames_alone(world, runs):
    from deeppointmap_amd import augment, evaluate, lidar_sim as LS
    from deeppointmap_amd.odometry import LidarOdometry, run_odometry
    P0, P1 = LS.sweep_poses(world.poses)
    frames = world.sim.frames(P0, poses_end=P1)
    before = [(f.xyz.clone(), f.idx.clone(), f.count.clone()) for f in frames]
    kw = dict(max_range=world.model.max_range, sample_map=0.25, sample_register=0.75, **world.first, **KW)
    odo = LidarOdometry(deskew=True, time="column", azimuth_steps=world.model.azimuth_steps, **kw)
    torch.cuda.synchronize()
    for f in frames:
        n = augment.host_syncs()
        step = odo.step(f)
        assert augment.host_syncs() == n + 1, "one host synchronisation per step"
        assert step.status in (L.CONVERGED, L.MAX_ITER)
    for f, (xyz, idx, count) in zip(frames, before):
        assert torch.equal(f.xyz.view(torch.int32), xyz.view(torch.int32)) and torch.equal(f.idx, idx) and torch.equal(f.count, count)
        assert f.sweep_motion is not None, "the caller's frame is still a raw one"
    assert np.allclose(odo.predicted_motion(frames[0]), np.linalg.inv(odo.poses[-2]) @ odo.poses[-1])
    raw = run_odometry(frames, **kw)
    a_desk, a_raw = evaluate.ate(np.stack(odo.poses), world.poses)["rmse"], evaluate.ate(raw, world.poses)["rmse"]
    log(f"sweep motion, {FRAMES} frames: ATE rmse deskewed by the odometry's own prediction {a_desk:.4e} m, raw {a_raw:.4e} m "
        f"(logged, not asserted), static frames {evaluate.ate(runs.gpu, world.poses)['rmse']:.4e} m")
    assert np.isfinite(a_desk) and np.isfinite(a_raw)
