"""GPU: point-to-plane registration against the local map (csrc/local_map.hip: dpm_local_map_register_planes) and the odometry
with metric="plane" and the adaptive gate, against the numpy restatement (tests/lidar_plane_restated.py).

  matches          every match of metric "plane" is that of metric "point" and of the exhaustive search; which matches give rows is
                   the restatement's gate on the GPU's OWN planes and counts (so the Jacobi's rounding stays out of it).
  sums             the 29 values on the kernel's own rows against the float64 restatement, per entry max(3 |r32 - r64|, floor),
                   unweighted and with kernel_scale 0.1, an outlier among the rows.
  known answer     the three_planes lattice, 0.3 m and 2 degrees, within 1e-4 m at the origin and 1 mm a kilometre away.
  sliding case     ground rings and two walls (lidar_plane_restated.sliding_scene): both metrics within 1 mm of the float64
                   restatement's pose, and the plane metric within 5 mm of the truth where the point metric is 0.49 m off.
  odometry         LidarOdometry(metric="plane") over the 12 simulated frames of tests/test_gpu_lidar_odometry.py: statuses,
                   poses within 1 mm of the restatement's, one host synchronisation a step, frames untouched, same bytes twice;
                   adaptive=: the gates used are the host function of the returned poses; metric="point" by default.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restated as I  # noqa: E402
import lidar_odometry_restated as L  # noqa: E402
import lidar_plane_restated as PR  # noqa: E402
from test_gpu_lidar_odometry import FRAMES, KW, host_rows, world  # noqa: E402,F401
from test_gpu_local_map import frame, gpu_map, lattice, log, matches_of  # noqa: E402
from test_lidar_odometry_host import known_pose_case, pose_error  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EYE = np.eye(4)


def gpu_planes(g):
    """the GPU's own planes as the restatement's namespace, and per row of the sorted export: normals, gate"""
    keys, counts, normal, w = g.export_planes()
    return PR.SimpleNamespace(keys=keys, counts=counts, normal=normal, w=w)


# -------------------------------------------------------------------------------------------------------------------- matches
@pytest.mark.parametrize("voxel,s,max_dist", [(1.0, 3, 0.75), (1.0, 2, 1.0), (0.5, 3, 0.5)])
def test_matches_are_the_point_metrics_and_the_gate_is_the_restatements(voxel, s, max_dist):
    rng = np.random.default_rng(23)
    scene = PR.normals_scene(seed=6, n=1500) * np.float32(voxel)
    pts = np.concatenate([scene, rng.uniform(-3, 3, (300, 3)).astype(np.float32) * np.float32(voxel), lattice(rng, 200, voxel / 4, 3 * voxel)])
    g = gpu_map(voxel, s, 1 << 12)
    g.insert(frame(pts), EYE)
    ex = g.export()
    q = np.concatenate([scene[rng.choice(len(scene), 500, replace=False)] + rng.normal(0, 0.05 * voxel, (500, 3)).astype(np.float32),
                        lattice(rng, 150, voxel / 4, 3 * voxel), rng.uniform(-4, 4, (150, 3)).astype(np.float32) * np.float32(voxel),
                        np.array([[80.0, 0, 0]], np.float32)])
    f = frame(q, len(q) + 5)
    _, (key0, sub0, sys0) = g.register(f, EYE, [(max_dist, 1)], debug=True)
    _, (key1, sub1, sys1) = g.register(f, EYE, [(max_dist, 1)], debug=True, metric="plane")
    point, plane = matches_of(key0, sub0, ex), matches_of(key1, sub1, ex)
    win, near = L.search_exhaustive(q, ex, np.float32(voxel), s, max_dist, np.float32)
    assert near.all() and np.array_equal(point[:len(q)], win) and (point[len(q):] == -1).all() and (plane[len(q):] == -1).all()
    normals, ok = PR.per_row(ex, gpu_planes(g))
    want = np.where((win >= 0) & ok[np.maximum(win, 0)], win, -1)
    assert np.array_equal(plane[:len(q)], want)
    rows, hits = int((want >= 0).sum()), int((win >= 0).sum())
    assert sys0[27].item() == hits and sys1[27].item() == rows and 100 < rows < hits
    # other gates: everything with three points, and nothing
    for min_points, max_ratio in ((3, 1.0), (5, 0.01), (10 ** 6, 0.1)):
        res, (key, sub, system) = g.register(f, EYE, [(max_dist, 1)], debug=True, metric="plane", min_points=min_points, max_ratio=max_ratio)
        ok = PR.per_row(ex, gpu_planes(g), min_points, max_ratio)[1]
        want = np.where((win >= 0) & ok[np.maximum(win, 0)], win, -1)
        assert np.array_equal(matches_of(key, sub, ex)[:len(q)], want) and system[27].item() == (want >= 0).sum()
        if min_points == 10 ** 6:
            assert int(res.status) == L.NO_MATCH and (want == -1).all() and res.pose[0].cpu().numpy().tobytes() == EYE.tobytes()
    log(f"plane matches voxel {voxel} s {s} max_dist {max_dist}: {len(q)} queries, {hits} matched as with point rows and the exhaustive "
        f"search, {rows} gave rows (min_points 5, max_ratio 0.1) as the restatement's gate on the GPU's planes says")


# ----------------------------------------------------------------------------------------------------------------------- sums
@pytest.mark.parametrize("kernel_scale", [0.0, 0.1])
def test_the_29_sums_of_the_plane_rows(kernel_scale):
    rng = np.random.default_rng(17)
    room = I.room(3000, seed=31).astype(np.float32)
    g = gpu_map(1.0, 3, 1 << 13)
    g.insert(frame(room), EYE)
    ex = g.export()
    true = I.se3([0.01, -0.02, 0.03], [0.3, -0.2, 0.1])
    src = I.moved(room[rng.choice(len(room), 1100, replace=False)].astype(np.float64) + rng.normal(0, 0.01, (1100, 3)), true)
    src[7] += np.float32(0.6)                         # a gross outlier that still finds a match, in a voxel with a plane
    init = I.perturbed(true, seed=5, trans=0.05, deg=0.2)
    res, (key, sub, system) = g.register(frame(src, 1300), init, [(1.0, 1)], kernel_scale=kernel_scale, debug=True, metric="plane")
    system = system.cpu().numpy()
    win = matches_of(key, sub, ex)[:len(src)]          # the matches that gave rows
    assert win[7] >= 0 and 800 < (win >= 0).sum() < 1100
    normals, ok = PR.per_row(ex, gpu_planes(g))
    assert ok[win[win >= 0]].all()
    S, parts = {}, {}
    for dtype in (np.float32, np.float64):
        q = I.transform(init, src, dtype)
        S[dtype], *parts[dtype] = PR.system(q, win, ex[3], normals, ok, kernel_scale, dtype)
    J, e, w, _ = parts[np.float64]
    q32 = I.transform(init, src, np.float32)
    delta = 4 * 2.0 ** -24 * max(float(np.abs(q32).max()), float(np.abs(ex[3]).max()))
    floor = PR.system_floor(J, e, w, kernel_scale, delta)
    bound = np.maximum(3 * np.abs(S[np.float32] - S[np.float64]), floor)
    err = np.abs(system - S[np.float64])
    assert system[27] == S[np.float64][27] == (win >= 0).sum()
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))))
    out_w = float(w[int((win[:7] >= 0).sum())])
    log(f"plane sums kernel_scale {kernel_scale}: rows {int(system[27])}/{len(src)}, max |gpu-r64| / bound over 29 sums {ratio:.3e}, "
        f"max |r32-r64| / |r64| {float(np.max(np.abs(S[np.float32] - S[np.float64]) / np.maximum(np.abs(S[np.float64]), 1e-300))):.3e}, "
        f"the outlier's weight {out_w:.3e}")
    assert (err <= bound).all(), (np.nonzero(err > bound)[0], err, bound)
    assert out_w == 1.0 if kernel_scale == 0 else out_w < 1e-2
    x, bad = I.solve(system)
    assert bad is None and int(res.iterations) == 1
    assert np.abs(res.pose[0].cpu().numpy() - I.update(init, x)).max() <= 1e-12
    assert abs(float(res.fitness) - system[27] / len(src)) < 1e-6 and abs(float(res.rmse) - np.sqrt(system[28] / system[27])) < 1e-6


# --------------------------------------------------------------------------------------------------------------- known answer
@pytest.mark.parametrize("origin,bound_t", [((0.0, 0.0, 0.0), 1e-4), ((1000.0, -500.0, 20.0), 1e-3)])
def test_known_pose_is_recovered_with_plane_rows(origin, bound_t):
    pts, true, src, start = known_pose_case(origin)
    g = gpu_map(1.0, 3, 1 << 12, origin=origin, max_range=100.0)
    g.insert(frame((pts - np.asarray(origin)).astype(np.float32)), start)
    res = g.register(frame(src, len(src) + 11), start, [(1.0, 40)], metric="plane")
    dt, dr = pose_error(res.pose[0].cpu().numpy(), true)
    log(f"known pose (0.3 m, 2 deg) with plane rows, map origin {origin}: status {int(res.status)}, iterations {int(res.iterations)}, "
        f"translation error {dt:.3e} m, rotation error {dr:.3e} rad, fitness {float(res.fitness):.3f}, rmse {float(res.rmse):.3e}")
    assert int(res.status) == L.CONVERGED and float(res.fitness) > 0.8
    assert dt <= bound_t and dr <= 1e-4, (dt, dr)


# --------------------------------------------------------------------------------------------------------------- sliding case
def test_sliding_case_on_the_gpu():
    f0, f1, P0, P1 = PR.sliding_scene()
    g = gpu_map(1.0, 3, 1 << 12, max_range=100.0)
    g.insert(frame(f0), P0)
    errors = {}
    for metric in ("plane", "point"):
        res = g.register(frame(f1, len(f1) + 7), P0, [(1.0, 50)], kernel_scale=0.1, metric=metric)
        pose = res.pose[0].cpu().numpy()
        want, want_err = PR.sliding_case(metric)
        errors[metric] = float(np.linalg.norm(pose[:3, 3] - P1[:3, 3]))
        diff = float(np.abs(pose - want["pose"]).max())
        log(f"sliding case {metric} rows: status {int(res.status)}, iterations {int(res.iterations)}, translation error {errors[metric]:.3e} m "
            f"(float64 restatement {want_err:.3e} m), |gpu - r64| {diff:.3e}")
        assert int(res.status) in (L.CONVERGED, L.MAX_ITER)
        assert diff <= 1e-3
    assert errors["plane"] <= 5e-3
    assert errors["point"] >= 20 * errors["plane"]


# ------------------------------------------------------------------------------------------------------------------- odometry
@pytest.fixture(scope="module")
def plane_run(world):
    from deeppointmap_amd import augment
    from deeppointmap_amd.odometry import LidarOdometry
    frames = world.sim.frames(world.poses)
    before = [(f.xyz.clone(), f.idx.clone(), f.count.clone()) for f in frames]
    runs = []
    for _ in range(2):
        odo = LidarOdometry(max_range=world.model.max_range, metric="plane", **world.first, **KW)
        torch.cuda.synchronize()
        syncs = []
        for f in frames:
            n = augment.host_syncs()
            odo.step(f)
            syncs.append(augment.host_syncs() - n)
        runs.append(PR.SimpleNamespace(odo=odo, syncs=syncs))
    return PR.SimpleNamespace(frames=frames, before=before, runs=runs, rows=host_rows(frames))


def test_plane_odometry_runs_like_the_restatement(world, plane_run):
    odo = plane_run.runs[0].odo
    assert len(odo.steps) == FRAMES and np.array_equal(odo.poses[0], world.poses[0])
    assert all(s.status in (L.CONVERGED, L.MAX_ITER) for s in odo.steps), [s.status for s in odo.steps]
    assert plane_run.runs[0].syncs == [1] * FRAMES == plane_run.runs[1].syncs, "one host synchronisation per step"
    for f, (xyz, idx, count) in zip(plane_run.frames, plane_run.before):
        assert torch.equal(f.xyz.view(torch.int32), xyz.view(torch.int32)) and torch.equal(f.idx, idx) and torch.equal(f.count, count)
    assert np.stack(odo.poses).tobytes() == np.stack(plane_run.runs[1].odo.poses).tobytes(), "two runs, the same bytes"
    assert [s[1:] for s in odo.steps] == [s[1:] for s in plane_run.runs[1].odo.steps]
    poses, statuses, _ = PR.odometry(plane_run.rows, KW["voxel_size"], KW["subdivisions"], world.model.max_range, KW["min_range"],
                                     KW["schedule"], KW["kernel_scale"], world.poses[0], np.float64,
                                     initial_motion=world.first["initial_motion"], metric="plane")
    assert all(s in (L.CONVERGED, L.MAX_ITER) for s in statuses)
    worst = 0.0
    for k in range(FRAMES):
        err = float(np.abs(odo.poses[k] - poses[k]).max())
        worst = max(worst, err)
        log(f"plane odometry frame {k}: |gpu - r64| {err:.3e}, |gpu - exact| {np.linalg.norm(odo.poses[k][:3, 3] - world.poses[k][:3, 3]):.3e} m, "
            f"status {odo.steps[k].status}, iterations {odo.steps[k].iterations}, fitness {odo.steps[k].fitness:.2f}")
    from deeppointmap_amd import evaluate
    log(f"plane odometry: worst |gpu - r64| over {FRAMES} frames {worst:.3e}; ATE rmse against the exact poses: GPU "
        f"{evaluate.ate(np.stack(odo.poses), world.poses)['rmse']:.4e} m, float64 restatement {evaluate.ate(poses, world.poses)['rmse']:.4e} m")
    assert worst <= 1e-3


def test_adaptive_gate_is_the_host_function_of_the_returned_poses(world, plane_run):
    from deeppointmap_amd import augment
    from deeppointmap_amd.odometry import LidarOdometry
    sigma0, min_motion = 0.3, 0.01
    odo = LidarOdometry(max_range=world.model.max_range, metric="plane", adaptive=(sigma0, min_motion), **world.first, **KW)
    for f in plane_run.frames:
        n = augment.host_syncs()
        step = odo.step(f)
        assert augment.host_syncs() == n + 1
        assert step.status in (L.CONVERGED, L.MAX_ITER)
    want = PR.gates_of(odo.poses, [s.status for s in odo.steps], sigma0, min_motion, world.model.max_range, KW["voxel_size"],
                       KW["schedule"][-1][1], world.first["initial_motion"])
    assert len(odo.gates) == len(want) == FRAMES - 1
    for k, ((schedule, scale), (max_dist, max_iter, want_scale)) in enumerate(zip(odo.gates, want)):
        assert len(schedule) == 1 and schedule[0][1] == max_iter
        assert abs(schedule[0][0] - max_dist) <= 1e-12 * max_dist and abs(scale - want_scale) <= 1e-12 * want_scale, k
        assert schedule[0][0] <= KW["voxel_size"]
    assert odo.gates[0] == (((min(3 * sigma0, 1.0), 30),), sigma0 / 3)
    from deeppointmap_amd import evaluate
    log(f"plane + adaptive ({sigma0}, {min_motion}): gates " + " ".join(f"{g[0][0][0]:.3f}" for g in odo.gates)
        + f", ATE rmse {evaluate.ate(np.stack(odo.poses), world.poses)['rmse']:.4e} m")


def test_metric_point_by_default_is_the_run_without_the_new_arguments(world, plane_run):
    from deeppointmap_amd.odometry import LidarOdometry
    frames = plane_run.frames[:6]
    kw = dict(max_range=world.model.max_range, **world.first, **KW)
    a = LidarOdometry(**kw)
    b = LidarOdometry(metric="point", plane_radius=None, min_points=5, max_ratio=0.1, adaptive=None, **kw)
    for f in frames:
        a.step(f), b.step(f)
    assert np.stack(a.poses).tobytes() == np.stack(b.poses).tobytes() and [s[1:] for s in a.steps] == [s[1:] for s in b.steps]
    assert a.local_map._planes is None and b.local_map._planes is None, "no plane launch with point rows"
    ea, eb = a.local_map.export(), b.local_map.export()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ea, eb))
