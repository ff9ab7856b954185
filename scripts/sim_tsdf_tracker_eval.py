"""Frame-to-model tracking on the TSDF (deeppointmap_amd/tsdf.py: TsdfTracker) over a simulated circuit with sweep motion,
next to the geometric odometry with point-to-plane rows (LidarOdometry(metric="plane")) on the same frames: every frame is
deskewed with the motion the simulator used (the frames' sweep_motion) before either sees it.  The tracker fuses the plane
distance with normals estimated from each frame alone within --normals-radius (TsdfMap's `normals=<radius>`); both are given
the motion between the first two frames, as scripts/sim_odometry_eval.py gives it.  For each: ATE against the exact poses
(evaluate.ate), the frames lost, and the fitness per frame.  A report, not a target: nothing is asserted.
--accuracy: only turn test_logs/tsdf_register_errors.log, which the tests write, into profiles/tsdf_register_accuracy.md.

  python scripts/sim_tsdf_tracker_eval.py [--frames 120] [--spacing 1.0] [--beams 16] [--columns 512] [--sigma 0.02] [--voxel 0.5] | --accuracy
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
    src = os.path.join(ROOT, "test_logs", "tsdf_register_errors.log")
    if not os.path.exists(src):
        return False
    lines = list(dict.fromkeys(open(src).read().splitlines()))
    with open(os.path.join(ROOT, "profiles", "tsdf_register_accuracy.md"), "w") as f:
        f.write("# Scan-to-TSDF registration: observed errors\n\nEvery comparison tests/test_tsdf_register_host.py made on the CPU "
                "(`host:`) and tests/test_gpu_tsdf_register.py made on the GPU (`gpu:`), as they logged it; the bounds are derived in "
                "those files.  `r32` / `r64`: the numpy restatement (tests/tsdf_register_restated.py) in float32 and float64.  The "
                "reference has no TSDF: there is nothing else to compare with.\n\n```\n")
        f.write("\n".join(lines) + "\n```\n")
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--spacing", type=float, default=1.0)
    ap.add_argument("--beams", type=int, default=16)
    ap.add_argument("--columns", type=int, default=512)
    ap.add_argument("--sigma", type=float, default=0.02)
    ap.add_argument("--voxel", type=float, default=0.5)
    ap.add_argument("--normals-radius", type=float, default=1.0)
    ap.add_argument("--accuracy", action="store_true")
    a = ap.parse_args()
    if a.accuracy:
        sys.exit(0 if accuracy_md() else "test_logs/tsdf_register_errors.log not found: run the tests first")
    if not torch.cuda.is_available():
        sys.exit("sim_tsdf_tracker_eval.py runs on a GPU; none is visible")
    from deeppointmap_amd import augment, evaluate, lidar_sim as LS
    from deeppointmap_amd.odometry import LidarOdometry
    from deeppointmap_amd.tsdf import TsdfTracker
    scene = LS.street_scene(2)
    model = LS.LidarModel(np.linspace(10.0, -20.0, a.beams), a.columns, 0.9, 80.0, range_sigma=a.sigma)
    poses = LS.circuit(scene, spacing=a.spacing)[:a.frames]
    F = len(poses)
    rng = torch.Generator(device=DEV)
    rng.manual_seed(1)
    sim = LS.LidarSimulator(scene, model, rng=rng if a.sigma > 0 else None, device=DEV)
    P0, P1 = LS.sweep_poses(poses)
    frames = [augment.deskew(f, f.sweep_motion, time="column", azimuth_steps=model.azimuth_steps) for f in sim.frames(P0, poses_end=P1)]
    first_motion = LS.sweep_delta(poses[0], poses[1])

    tr = TsdfTracker(a.voxel, max_voxels=1 << 22, max_range=model.max_range, device=DEV, distance="plane", kernel_scale=a.voxel)
    for k, f in enumerate(frames):
        tr.step(f, a.normals_radius, pose=poses[0] if k == 0 else poses[0] @ first_motion if k == 1 else None)
    tr.map.check()
    odo = LidarOdometry(max_range=model.max_range, first_pose=poses[0], initial_motion=first_motion, sample_map=0.25,
                        sample_register=0.75, metric="plane")
    for f in frames:
        odo.step(f)
    runs = {"TsdfTracker (plane distance)": (np.stack(tr.poses), [s.fitness for s in tr.steps], tr.lost,
                                             [s.iterations for s in tr.steps]),
            "LidarOdometry(metric=\"plane\")": (np.stack(odo.poses), [s.fitness for s in odo.steps],
                                                sum(s.status not in (0, 1) for s in odo.steps), [s.iterations for s in odo.steps])}
    path = os.path.join(ROOT, "profiles", "sim_tsdf_tracker_eval.md")
    with open(path, "w") as f:
        f.write("# Frame-to-model tracking on the TSDF, on a simulated circuit\n\n")
        f.write(f"`python scripts/sim_tsdf_tracker_eval.py --frames {a.frames} --spacing {a.spacing} --beams {a.beams} --columns {a.columns} "
                f"--sigma {a.sigma} --voxel {a.voxel}` on {torch.cuda.get_device_name(0)}: lidar_sim.street_scene(2), {F} poses of its circuit "
                f"{a.spacing} m apart, {a.beams} beams x {a.columns} columns, range noise {a.sigma} m, sweep motion deskewed with the true "
                f"motion.  TsdfTracker: voxel {a.voxel} m, truncation {tr.map.truncation:g} m, plane distance with normals estimated within "
                f"{a.normals_radius} m of each frame alone, kernel_scale {a.voxel}, every row registered; LidarOdometry: its defaults with "
                "sample_map 0.25 m, sample_register 0.75 m.  Both are given the first motion.  A report, not a target.\n\n"
                "| system | ATE rmse m | ATE max m | final position error m | frames lost | fitness min / median | iterations median |\n"
                "|---|---|---|---|---|---|---|\n")
        for name, (est, fit, lost, its) in runs.items():
            ok = np.isfinite(est).all()
            ate = evaluate.ate(est, poses) if ok else None
            fin = float(np.linalg.norm(est[-1][:3, 3] - poses[-1][:3, 3])) if ok else float("nan")
            f.write(f"| {name} | {ate['rmse'] if ate else float('nan'):.4f} | {ate['max'] if ate else float('nan'):.4f} | {fin:.4f} | {lost} | "
                    f"{min(fit[1:]):.3f} / {float(np.median(fit[1:])):.3f} | {int(np.median(its[1:]))} |\n")
        f.write("\nFitness per frame (rows given / rows registered; the first frame has no registration):\n\n```\n")
        for name, (est, fit, lost, its) in runs.items():
            f.write(f"{name}: {[round(float(v), 2) for v in fit]}\n")
        f.write("```\n\nPosition error per tenth frame (m):\n\n```\n")
        for name, (est, fit, lost, its) in runs.items():
            f.write(f"{name}: {[round(float(np.linalg.norm(est[k][:3, 3] - poses[k][:3, 3])), 3) for k in range(0, F, 10)]}\n")
        f.write("```\n\nThe tracker does not deskew, prune, close loops or thin its input; a sparse sensor loses rows between its rings, "
                "where a cell lacks one of its 8 corners.\n")
    print(open(path).read())


if __name__ == "__main__":
    main()
