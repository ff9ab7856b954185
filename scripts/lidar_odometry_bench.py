"""The local map and the registration against it (csrc/local_map.hip) at HDL64E size: two consecutive simulated frames of
lidar_sim.street_scene(2), 64 beams x 2048 columns, one metre apart.
  insert           claim + commit of the first frame into an empty map (the init that empties it is timed apart)
  prune            the clear of the other half + the re-claim, everything surviving
  planes           one plane per voxel over ALL slots of the table (dpm_local_map_planes), the map holding the first frame
  per iteration    (register with --iters iterations and the stop rule off - register with none) / iters: accumulate + solve,
                   with point rows and with plane rows
  register         a default run of the second frame (30 iterations at most) from a start 0.1 m off
  step             LidarOdometry.step of the second frame, host time around the call: its one synchronisation included
  batched ICP      dpm_icp_refine_batched, point metric, on the same frame pair and start: grids and per iteration
Device time between two events, median [min, max] of --reps runs after --warmup.  Reports, not thresholds; written to
profiles/lidar_odometry_bench.md.  Not run here: a profile of the kernels' counters, and any size but this one.

  python scripts/lidar_odometry_bench.py [--iters 10] [--reps 5] [--warmup 2] [--sample 0.0]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

sys.path.insert(0, os.path.join(ROOT, "scripts"))
from icp_bench import timed  # noqa: E402

DEV = "cuda"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=float, default=0.0, help="voxel_sample edge applied to both frames first (0: none)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lidar_odometry_bench.py measures on a GPU; none is visible")
    from deeppointmap_amd import augment, lidar_sim as LS, ops
    from deeppointmap_amd.odometry import LidarOdometry, LocalMap
    scene = LS.street_scene(2)
    model = LS.HDL64E
    poses = LS.circuit(scene, spacing=1.0)[:2]
    frames = LS.LidarSimulator(scene, model, device=DEV).frames(poses)
    if a.sample > 0:
        frames = [augment.voxel_sample(f, a.sample) for f in frames]
    n = [f.nbr_point for f in frames]
    start = poses[1].copy()
    start[:3, 3] += [0.08, -0.05, 0.03]
    P = [torch.from_numpy(p).to(DEV) for p in (poses[0], poses[1], start)]
    kw = dict(voxel_size=1.0, subdivisions=3, max_voxels=1 << 17, max_range=model.max_range)

    def fresh():
        m = LocalMap(origin=poses[0][:3, 3], device=DEV, **kw)
        m._ready(torch.device(DEV))
        return m
    rows = []
    m = fresh()
    rows.append(("init (both halves emptied)", timed(lambda: ops.local_map_new(m.max_voxels, m.subdivisions, DEV), a.reps, a.warmup), None))
    # every repetition inserts the same frame with a later stamp: the claims find their voxels, the owner words stay
    rows.append((f"insert, {n[0]} points (claim + commit)", timed(lambda: m.insert(frames[0], P[0]), a.reps, a.warmup), None))
    held = m.n_points
    rows.append((f"prune, {held} points held, all surviving (clear + re-claim)", timed(lambda: m.prune(P[0]), a.reps, a.warmup), None))
    none = timed(lambda: m.register(frames[1], P[2], [(1.0, 0)]), a.reps, a.warmup)
    t = timed(lambda: m.register(frames[1], P[2], [(1.0, a.iters)], kernel_scale=0.1, tol_rot=0.0, tol_trans=0.0), a.reps, a.warmup)
    rows.append((f"register, {a.iters} iterations, stop rule off, {n[1]} points", t, (t[0] - none[0]) / a.iters))
    point_iter = (t[0] - none[0]) / a.iters
    planes_t = timed(lambda: ops.local_map_planes(*m._args(), m.plane_radius, *m.planes()), a.reps, a.warmup)
    rows.append((f"planes, all {m.max_voxels} slots, {held} points held (one launch)", planes_t, None))
    counts, w = m.planes()[1], m.planes()[0][:, 3]
    n_vox, n_flat = int((counts > 0).sum()), int(((counts >= 5) & (w >= 0) & (w <= 0.1)).sum())
    none_p = timed(lambda: m.register(frames[1], P[2], [(1.0, 0)], metric="plane"), a.reps, a.warmup)
    t = timed(lambda: m.register(frames[1], P[2], [(1.0, a.iters)], kernel_scale=0.1, tol_rot=0.0, tol_trans=0.0, metric="plane"),
              a.reps, a.warmup)
    rows.append((f"register with plane rows, {a.iters} iterations, stop rule off (planes cached)", t, (t[0] - none_p[0]) / a.iters))
    res_p = m.register(frames[1], P[2], [(1.0, 30)], kernel_scale=0.1, metric="plane")
    err_p = float(np.linalg.norm(res_p.pose[0].cpu().numpy()[:3, 3] - poses[1][:3, 3]))
    res = m.register(frames[1], P[2], [(1.0, 30)], kernel_scale=0.1)
    rows.append(("register, default run (30 iterations at most)", timed(lambda: m.register(frames[1], P[2], [(1.0, 30)], kernel_scale=0.1),
                                                                   a.reps, a.warmup), None))
    err = float(np.linalg.norm(res.pose[0].cpu().numpy()[:3, 3] - poses[1][:3, 3]))
    # the batched ICP on the same pair: frames as (F,3,N)
    N = max(f.cap for f in frames)
    pcd = torch.zeros(2, 3, N, device=DEV)
    for k, f in enumerate(frames):
        pcd[k, :, :f.cap] = f.xyz.T
    lengths = torch.tensor(n, dtype=torch.int32, device=DEV)
    src, dst = torch.tensor([1], dtype=torch.int32, device=DEV), torch.tensor([0], dtype=torch.int32, device=DEV)
    rel = torch.from_numpy((np.linalg.inv(poses[0]) @ start)[None]).to(DEV)
    grids = timed(lambda: ops.icp_refine(pcd, lengths, src, dst, rel, [(1.0, 0)], ops.ICP_POINT), a.reps, a.warmup)
    t = timed(lambda: ops.icp_refine(pcd, lengths, src, dst, rel, [(1.0, a.iters)], ops.ICP_POINT, tol_rot=0.0, tol_trans=0.0), a.reps, a.warmup)
    rows.append(("dpm_icp_refine_batched, one pair, no iteration (grid build)", grids, None))
    rows.append((f"dpm_icp_refine_batched, one pair, point metric, {a.iters} iterations, stop rule off", t, (t[0] - grids[0]) / a.iters))
    # the whole step, host time
    odo = LidarOdometry(first_pose=poses[0], initial_motion=LS.sweep_delta(poses[0], poses[1]), sample_map=a.sample or None, **kw)
    odo.step(frames[0])
    wall = []
    for _ in range(a.reps + a.warmup):
        keep = (list(odo.poses), list(odo.steps))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = odo.step(frames[1])
        wall.append((time.perf_counter() - t0) * 1e3)
        odo.poses, odo.steps = keep
    wall = sorted(wall[a.warmup:])
    with open(os.path.join(ROOT, "profiles", "lidar_odometry_bench.md"), "w") as f:
        f.write("# Local map and registration: time per launch and per frame\n\n")
        f.write(f"`python scripts/lidar_odometry_bench.py --iters {a.iters} --sample {a.sample}` on {torch.cuda.get_device_name(0)} "
                f"(torch {torch.__version__}): street_scene(2), HDL64E (64 x 2048 rays), frames of {n[0]} and {n[1]} returns one metre "
                f"apart, voxel 1.0 m, 3^3 sub-cells, 2^17 slots ({ops.local_map_new(1 << 17, 3, DEV).numel() / 2**20:.0f} MiB); device "
                f"time between two events, median [min, max] ms of {a.reps} runs after {a.warmup} warm-up runs.  Reports, not "
                "thresholds.\n\n| what | ms | ms per iteration |\n|---|---|---|\n")
        for what, (med, lo, hi), per in rows:
            f.write(f"| {what} | {med:.3f} [{lo:.3f}, {hi:.3f}] | {'' if per is None else f'{per:.3f}'} |\n")
        f.write(f"| LidarOdometry.step of the second frame, host time, one synchronisation | {wall[len(wall) // 2]:.3f} [{wall[0]:.3f}, {wall[-1]:.3f}] | |\n")
        f.write(f"\nDefault run: {int(res.iterations)} iterations, status {int(res.status)}, fitness {float(res.fitness):.3f}, refined "
                f"translation {err:.4f} m from the exact pose (start 0.1 m off); the step took {s.iterations} iterations.  init and "
                "prune write every key and owner word of a half (28 words a slot here) whatever the map holds.\n"
                f"Plane rows: {n_vox} voxels held, {n_flat} of them give rows (>= 5 points, w <= 0.1); default run "
                f"{int(res_p.iterations)} iterations, status {int(res_p.status)}, fitness {float(res_p.fitness):.3f}, refined translation "
                f"{err_p:.4f} m from the exact pose.  The planes launch over all slots costs {planes_t[0] / point_iter:.2f} point "
                "iterations" + (": more than one, and it is paid once a step; recomputing only the voxels whose 27-neighbourhood an "
                                "insert or a prune changed is the next step.\n" if planes_t[0] > point_iter else ".\n") +
                "Not run: hardware counters of the new kernels; other sensor sizes; the batched ICP with more than one pair.\n")
    print(open(os.path.join(ROOT, "profiles", "lidar_odometry_bench.md")).read())


if __name__ == "__main__":
    main()
