"""The geometric odometry (deeppointmap_amd/odometry.py) over a simulated circuit with sweep motion, from three inputs:
  raw        the frames as a moving sensor takes them
  predicted  deskewed by the odometry's own constant-velocity prediction (LidarOdometry(deskew=True))
  true       deskewed with the motion the simulator used (the frames' sweep_motion) before the odometry sees them
and, next to them, the same circuit without sweep motion, there also with point-to-plane rows (metric="plane") and with the
adaptive gate on top (adaptive=(spacing, 0.1)).  For each: ATE, RPE and KITTI segment errors against the exact
poses (evaluate.trajectory_metrics) and map_accuracy of the odometry's own map, the points it holds at the end under the poses
it estimated, against the scene.  The motion between the first two frames is given to every run (initial_motion): see
LidarOdometry's docstring.  --no-initial-motion adds the run without it.  A report, not a target: nothing is asserted.
--accuracy: only turn test_logs/lidar_odometry_errors.log, which the tests write, into profiles/lidar_odometry_accuracy.md.

  python scripts/sim_odometry_eval.py [--frames 120] [--spacing 1.0] [--beams 16] [--columns 512] [--sigma 0.02] | --accuracy
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

DEV = "cuda"


def accuracy_md():
    src = os.path.join(ROOT, "test_logs", "lidar_odometry_errors.log")
    if not os.path.exists(src):
        return False
    lines = list(dict.fromkeys(open(src).read().splitlines()))
    with open(os.path.join(ROOT, "profiles", "lidar_odometry_accuracy.md"), "w") as f:
        f.write("# Local map and geometric odometry: observed errors\n\nEvery comparison tests/test_gpu_local_map.py, "
                "tests/test_gpu_lidar_odometry.py, tests/test_gpu_local_map_planes.py and tests/test_gpu_lidar_odometry_plane.py made "
                "on the GPU, as they logged it; the bounds are derived in those files.  `r32` / `r64`: the numpy restatement "
                "(tests/lidar_odometry_restated.py, tests/lidar_plane_restated.py) in float32 and float64.  The reference "
                "has no geometric odometry: there is nothing else to compare with.\n\n```\n")
        f.write("\n".join(lines) + "\n```\n")
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--spacing", type=float, default=1.0)
    ap.add_argument("--beams", type=int, default=16)
    ap.add_argument("--columns", type=int, default=512)
    ap.add_argument("--sigma", type=float, default=0.02)
    ap.add_argument("--no-initial-motion", action="store_true")
    ap.add_argument("--accuracy", action="store_true")
    a = ap.parse_args()
    if a.accuracy:
        sys.exit(0 if accuracy_md() else "test_logs/lidar_odometry_errors.log not found: run the GPU tests first")
    if not torch.cuda.is_available():
        sys.exit("sim_odometry_eval.py runs on a GPU; none is visible")
    from deeppointmap_amd import augment, evaluate, lidar_sim as LS
    from deeppointmap_amd.odometry import LidarOdometry
    scene = LS.street_scene(2)
    model = LS.LidarModel(np.linspace(10.0, -20.0, a.beams), a.columns, 0.9, 80.0, range_sigma=a.sigma)
    poses = LS.circuit(scene, spacing=a.spacing)[:a.frames]
    F = len(poses)
    rng = torch.Generator(device=DEV)
    rng.manual_seed(1)
    sim = LS.LidarSimulator(scene, model, rng=rng if a.sigma > 0 else None, device=DEV)
    P0, P1 = LS.sweep_poses(poses)
    kw = dict(max_range=model.max_range, first_pose=poses[0], initial_motion=LS.sweep_delta(poses[0], poses[1]),
              sample_map=0.25, sample_register=0.75)
    rows = []

    def run(name, frames, **extra):
        odo = LidarOdometry(**{**kw, **extra})
        for f in frames:
            odo.step(f)
        est = np.stack(odo.poses)
        if not np.isfinite(est).all():
            rows.append((name + " (poses not finite: no metrics)", {}, None, sum(s.status not in (0, 1) for s in odo.steps), 0))
            return
        its = [s.iterations for s in odo.steps[1:]]
        print(f"{name}: statuses {np.bincount([s.status for s in odo.steps], minlength=4).tolist()}, iterations {min(its)}..{max(its)}, "
              f"fitness {min(s.fitness for s in odo.steps[1:]):.2f}..{max(s.fitness for s in odo.steps[1:]):.2f}, position error per "
              f"tenth frame {[round(float(np.linalg.norm(est[k][:3, 3] - poses[k][:3, 3])), 2) for k in range(0, F, 10)]}", flush=True)
        m = evaluate.trajectory_metrics(est, poses)
        cloud = torch.from_numpy(np.ascontiguousarray(odo.local_map.points().T)).to(DEV, torch.float32)
        acc = evaluate.map_accuracy(cloud, scene) if cloud.shape[1] else None
        bad = sum(s.status not in (0, 1) for s in odo.steps)
        rows.append((name, m, acc, bad, odo.local_map.n_points))

    run("no sweep motion", sim.frames(poses))
    run("sweep motion, raw", sim.frames(P0, poses_end=P1))
    run("sweep motion, deskewed by the own prediction", sim.frames(P0, poses_end=P1), deskew=True, time="column",
        azimuth_steps=model.azimuth_steps)
    run("sweep motion, deskewed with the true motion",
        [augment.deskew(f, f.sweep_motion, time="column", azimuth_steps=model.azimuth_steps) for f in sim.frames(P0, poses_end=P1)])
    # point-to-plane rows, and with them the adaptive gate (sigma0 = the spacing, min_motion 0.1 m: KISS-ICP's defaults scaled)
    adaptive = (a.spacing, 0.1)
    run("no sweep motion, plane", sim.frames(poses), metric="plane")
    run("no sweep motion, plane + adaptive", sim.frames(poses), metric="plane", adaptive=adaptive)
    run("sweep motion, deskewed by the own prediction, plane + adaptive", sim.frames(P0, poses_end=P1), deskew=True, time="column",
        azimuth_steps=model.azimuth_steps, metric="plane", adaptive=adaptive)
    if a.no_initial_motion:
        run("no sweep motion, initial_motion not given", sim.frames(poses), initial_motion=None)
        run("no sweep motion, plane, initial_motion not given", sim.frames(poses), initial_motion=None, metric="plane")
        run("no sweep motion, plane + adaptive, initial_motion not given", sim.frames(poses), initial_motion=None, metric="plane",
            adaptive=adaptive)

    def num(d, k, fmt="{:.4f}"):
        return "-" if not d or d.get(k) is None else fmt.format(d[k])
    with open(os.path.join(ROOT, "profiles", "sim_odometry_eval.md"), "w") as f:
        f.write("# Geometric odometry on a simulated circuit\n\n")
        f.write(f"`python scripts/sim_odometry_eval.py --frames {a.frames} --spacing {a.spacing} --beams {a.beams} --columns {a.columns} "
                f"--sigma {a.sigma}{' --no-initial-motion' if a.no_initial_motion else ''}` on {torch.cuda.get_device_name(0)}: lidar_sim.street_scene(2), {F} poses of its circuit "
                f"{a.spacing} m apart, {a.beams} beams x {a.columns} columns, range noise {a.sigma} m; LidarOdometry with its defaults, "
                "sample_map 0.25 m, sample_register 0.75 m, the first motion given unless the row says otherwise; `plane`: "
                f"metric=\"plane\", `adaptive`: adaptive=({a.spacing}, 0.1).  A report, not a target.\n\n"
                "| input | ATE rmse m | ATE max m | RPE trans rmse m | RPE rot rmse rad | KITTI t % | KITTI r deg/m | failed steps | "
                "map points | map mean dist m | map rmse m |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
        for name, m, acc, bad, n in rows:
            ate, rpe, kitti = m.get("ate"), m.get("rpe"), m.get("kitti")
            tot = acc.get("total") if acc else None
            k = dict(t=100 * kitti["t_err"], r=float(np.degrees(kitti["r_err"]))) if kitti else None
            f.write(f"| {name} | {num(ate, 'rmse')} | {num(ate, 'max')} | {num(rpe, 'trans_rmse')} | {num(rpe, 'rot_rmse', '{:.2e}')} | "
                    f"{num(k, 't', '{:.3f}')} | {num(k, 'r', '{:.4f}')} | {bad} | {n} | {num(tot, 'mean')} | {num(tot, 'rmse')} |\n")
        f.write("\n`-`: the metric does not exist for this run (KITTI segments need 100 m of path).  The columns are "
                "evaluate.trajectory_metrics' and evaluate.map_accuracy's.\n")
    print(open(os.path.join(ROOT, "profiles", "sim_odometry_eval.md")).read())


if __name__ == "__main__":
    main()
