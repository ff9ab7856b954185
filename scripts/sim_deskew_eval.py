#!/usr/bin/env python3
"""profiles/sim_deskew_eval.md: what sweep motion does to a map and what deskewing gives back.  A SMALL16 sensor drives the
circuit of street_scene(--seed) at --spacing metres a frame and turns once per frame (lidar_sim.sweep_poses); the voxel map
of all frames under their EXACT start poses is measured against the scene (evaluate.map_accuracy) for

  raw            the clouds as the moving sensor delivers them;
  true motion    augment.Deskew("frame"): every frame compensated with its own exact motion;
  constant vel.  augment.Deskew(motion=constant_velocity_motion(P[f-1], P[f])): the previous relative pose of the ground-truth
                 trajectory as the prediction (frame 0 has no predecessor and stays raw) -- what a caller without ground truth
                 for the CURRENT sweep can do.

A report of one run, not a target.

  python scripts/sim_deskew_eval.py [--seed 2] [--spacing 1.5] [--voxel 0.2] [--batch 16]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

DEV = "cuda"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--spacing", type=float, default=1.5)
    ap.add_argument("--voxel", type=float, default=0.2)
    ap.add_argument("--batch", type=int, default=16)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sim_deskew_eval.py runs on a GPU; none is visible")
    from deeppointmap_amd import augment, evaluate, globalmap, lidar_sim as LS
    scene = LS.street_scene(a.seed)
    m = LS.SMALL16
    P0, P1 = LS.sweep_poses(LS.circuit(scene, spacing=a.spacing))
    F = P0.shape[0]
    sim = LS.LidarSimulator(scene, m, device=DEV)
    predicted = [np.eye(4)] + [augment.constant_velocity_motion(P0[f - 1], P0[f]) for f in range(1, F)]
    variants = {
        "raw": lambda f: None,
        "true motion": lambda f: augment.Deskew("frame", time="column", azimuth_steps=m.azimuth_steps),
        "constant velocity": lambda f: augment.Deskew(predicted[f], time="column", azimuth_steps=m.azimuth_steps),
    }
    rows, points = {}, 0
    for name, make in variants.items():
        clouds = []
        for b in range(0, F, a.batch):
            for k, pcd in enumerate(sim.frames(P0[b:b + a.batch], poses_end=P1[b:b + a.batch])):
                t = make(b + k)
                pcd = pcd if t is None else t(pcd)
                clouds.append(pcd.points().T.contiguous())
        points = sum(c.shape[1] for c in clouds)
        centroids, _ = globalmap.voxel_map(clouds, P0, voxel_size=a.voxel)
        rows[name] = (centroids.shape[1], evaluate.map_accuracy(centroids, scene)["total"])
        print(name, rows[name], flush=True)
    err = [float(np.linalg.norm((np.linalg.inv(LS.sweep_delta(P0[f], P1[f])) @ predicted[f])[:3, 3])) for f in range(1, F)]
    with open(os.path.join(ROOT, "profiles", "sim_deskew_eval.md"), "w") as f:
        f.write("# Sweep motion and deskew: the map against the scene\n\n")
        f.write(f"`python scripts/sim_deskew_eval.py --seed {a.seed} --spacing {a.spacing} --voxel {a.voxel}` on "
                f"{torch.cuda.get_device_name(0)} (torch {torch.__version__}): street_scene({a.seed}), {scene.P} primitives, {F} frames "
                f"{a.spacing} m apart round the circuit, SMALL16 ({m.rays} rays), the sensor turning once per frame, {points} returns "
                f"in all.  The voxel map ({a.voxel} m centroids) of all frames under their exact start poses against the scene "
                "(evaluate.map_accuracy, total row; distances in metres).  The constant-velocity prediction misses the true end "
                f"position of a sweep by {np.mean(err):.3f} m on average, {np.max(err):.3f} m at most (the corners).  A report of "
                "one run, not a target.\n\n")
        thr = list(next(iter(rows.values()))[1]["within"])
        f.write("| clouds | map points | mean | rmse | max | " + " | ".join(f"within {t} m" for t in thr) + " |\n")
        f.write("|---|---|---|---|---|" + "---|" * len(thr) + "\n")
        for name, (M, r) in rows.items():
            f.write(f"| {name} | {M} | {r['mean']:.5f} | {r['rmse']:.5f} | {r['max']:.4f} | "
                    + " | ".join(f"{100 * r['within'][t]:.2f} %" for t in thr) + " |\n")


if __name__ == "__main__":
    main()
