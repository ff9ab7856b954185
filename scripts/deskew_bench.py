#!/usr/bin/env python3
"""profiles/deskew_bench.md: what sweep motion costs the simulator and what the deskew transform costs.

* dpm_lidar_cull_sweep / dpm_lidar_cast_sweep next to dpm_lidar_cull / dpm_lidar_cast on the batch profiles/lidar_sim_bench.md
  records: --frames HDL64E frames of street_scene(0, 3 x 3 blocks), 225 primitives;
* augment.deskew (column mode) next to a points_affine rotation + translation, both in place on the same --points point
  frame: the affine map reads and writes every row once, the copy-rate yardstick of a per-row transform.

Device time between two events around --inner launches, per launch, median [min, max] of --reps such windows after --warmup.
--static-only measures nothing but the two static launches and appends one JSON line (tagged --tag) to --log: run from a
checkout of the parent commit and from this one, alternating, it says whether the static path moved and by how much the
same code moves from run to run; the full run copies the lines of --log into the profile.  A report, not a target.
--accuracy: only turn test_logs/deskew_errors.log and test_logs/lidar_sweep_errors.log, which the tests write, into
profiles/deskew_accuracy.md.

  python scripts/deskew_bench.py [--frames 16] [--points 120000] [--reps 30] [--inner 20] [--warmup 3] [--log FILE]
  python scripts/deskew_bench.py --static-only --tag parent --log FILE
  python scripts/deskew_bench.py --accuracy
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

DEV = "cuda"


def accuracy_md():
    logs = [os.path.join(ROOT, "test_logs", n) for n in ("deskew_errors.log", "lidar_sweep_errors.log")]
    if not all(os.path.exists(p) for p in logs):
        return False
    with open(os.path.join(ROOT, "profiles", "deskew_accuracy.md"), "w") as f:
        f.write("# Sweep motion and deskew: observed errors\n\nEvery comparison tests/test_lidar_sweep_host.py, "
                "tests/test_gpu_lidar_sweep.py and tests/test_gpu_deskew.py made, as they logged it; the bounds are stated in those "
                "files.  Neither the simulator's sweep motion nor the deskew has a counterpart in the reference: they are pinned to "
                "this project's own numpy restatement (tests/lidar_sweep_restated.py) and to the exact scene.\n")
        for title, p in zip(("Deskew", "Simulator with sweep motion"), logs):
            lines = list(dict.fromkeys(open(p).read().splitlines()))
            f.write(f"\n## {title}\n\n```\n" + "\n".join(lines) + "\n```\n")
    return True


def timed(fn, reps, inner, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--static-only", action="store_true")
    ap.add_argument("--tag", default="this commit")
    ap.add_argument("--log", default=None)
    ap.add_argument("--accuracy", action="store_true")
    a = ap.parse_args()
    if a.accuracy:
        sys.exit(0 if accuracy_md() else "test_logs/deskew_errors.log and lidar_sweep_errors.log not found: run the tests first")
    if not torch.cuda.is_available():
        sys.exit("deskew_bench.py measures on a GPU; none is visible")
    from deeppointmap_amd import lidar_sim as LS, ops
    m = LS.HDL64E
    scene = LS.street_scene(0, blocks=(3, 3))
    all_poses = LS.circuit(scene, 2.0)
    sel = np.linspace(0, len(all_poses) - 2, a.frames).astype(int)
    poses, ends = all_poses[sel], all_poses[sel + 1]
    sd = scene.to_device(DEV)
    dirs = torch.from_numpy(m.directions()).to(DEV)
    dp = torch.from_numpy(poses).to(DEV)
    F, P = a.frames, scene.P
    cull = lambda: ops.lidar_cull(sd.prims, sd.kind, sd.ground, dp, m.max_range, max(P, 1))
    kept, plane, status = cull()
    cast = lambda: ops.lidar_cast(kept, plane, status, P, dirs, m.min_range, m.max_range)
    static = {"dpm_lidar_cull": timed(cull, a.reps, a.inner, a.warmup), "dpm_lidar_cast": timed(cast, a.reps, a.inner, a.warmup)}
    if a.static_only:
        line = json.dumps({"tag": a.tag, **{k: [round(v, 5) for v in t] for k, t in static.items()}})
        print(line, flush=True)
        if a.log:
            with open(a.log, "a") as f:
                f.write(line + "\n")
        return
    from deeppointmap_amd import augment
    de = torch.from_numpy(ends).to(DEV)
    cull_s = lambda: ops.lidar_cull_sweep(sd.prims, sd.kind, sd.ground, dp, de, m.azimuth_steps, m.max_range, max(P, 1))
    kept_s, plane_s, status_s, table = cull_s()
    cast_s = lambda: ops.lidar_cast_sweep(kept_s, plane_s, status_s, table, P, dirs, m.min_range, m.max_range)
    sweep = {"dpm_lidar_cull_sweep": timed(cull_s, a.reps, a.inner, a.warmup), "dpm_lidar_cast_sweep": timed(cast_s, a.reps, a.inner, a.warmup)}
    # one frame of --points rows: a simulated frame's first rows when it has that many, else the frame padded by repetition
    frame = LS.LidarSimulator(sd, m).frames(poses[:1], poses_end=ends[:1])[0]
    n = frame.nbr_point
    rows = torch.arange(a.points, device=DEV) % n
    pcd = augment.PointCloud.from_buffers(frame.xyz[rows].contiguous(), frame.idx[rows].contiguous(),
                                          torch.tensor([a.points], dtype=torch.int32, device=DEV), host_n=a.points)
    D = LS.sweep_delta(poses[0], ends[0])
    R_aug, T_aug = torch.from_numpy(D[:3, :3]).float(), torch.from_numpy(D[:3, 3:]).float()
    params = R_aug.flatten().tolist() + T_aug.flatten().tolist()
    rowwise = {"augment.deskew (column mode)": timed(lambda: ops.points_deskew(pcd.xyz, pcd.idx, pcd.count, D, ops.DESKEW_COLUMN,
                                                                                m.azimuth_steps, None, 0.0), a.reps, a.inner, a.warmup),
               "points_affine (R x + T)": timed(lambda: augment._affine(pcd, 0, params), a.reps, a.inner, a.warmup)}
    with open(os.path.join(ROOT, "profiles", "deskew_bench.md"), "w") as f:
        f.write("# Sweep motion and deskew: time per launch\n\n")
        f.write(f"`python scripts/deskew_bench.py --frames {F} --points {a.points}` on {torch.cuda.get_device_name(0)} (torch "
                f"{torch.__version__}).  Device time between two events around {a.inner} launches, per launch: median [min, max] ms of "
                f"{a.reps} windows after {a.warmup} warm-up calls.  A report, not a target.\n\n")
        f.write(f"## The simulator: {F} HDL64E frames ({m.rays} rays each), street_scene(0, 3 x 3), {P} primitives\n\n"
                f"{int(status[:, 0].min())} to {int(status[:, 0].max())} primitives within range of a static frame, "
                f"{int(status_s[:, 0].min())} to {int(status_s[:, 0].max())} of a frame that moves to the next pose of the circuit "
                "(2 m on).\n\n| launch | ms per batch | ms per frame |\n|---|---|---|\n")
        for what, (med, lo, hi) in {**static, **sweep}.items():
            f.write(f"| {what} | {med:.4f} [{lo:.4f}, {hi:.4f}] | {med / F:.5f} |\n")
        f.write(f"\n## Per-row transforms in place on one frame of {a.points} points\n\n"
                "Bytes = 24 a row (xyz read and written) and, for the deskew, 4 more (idx).\n\n| launch | ms | GB/s |\n|---|---|---|\n")
        for what, (med, lo, hi) in rowwise.items():
            by = a.points * (28 if "deskew" in what else 24)
            f.write(f"| {what} | {med:.5f} [{lo:.5f}, {hi:.5f}] | {by / med / 1e6:.0f} |\n")
        if a.log and os.path.exists(a.log):
            f.write("\n## The static launches, parent commit and this one\n\nThe same script with --static-only, one process each, "
                    "alternating, in one session on one GPU (ms per batch, median [min, max]).  The spread between the parent's own "
                    "runs is the yardstick for any difference between the two.\n\n| run | dpm_lidar_cull | dpm_lidar_cast |\n|---|---|---|\n")
            for line in open(a.log).read().splitlines():
                r = json.loads(line)
                cell = lambda t: f"{t[0]:.4f} [{t[1]:.4f}, {t[2]:.4f}]"
                f.write(f"| {r['tag']} | {cell(r['dpm_lidar_cull'])} | {cell(r['dpm_lidar_cast'])} |\n")
    for k, v in {**static, **sweep, **rowwise}.items():
        print(k, v, flush=True)


if __name__ == "__main__":
    main()
