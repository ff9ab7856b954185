#!/usr/bin/env python3
"""profiles/lidar_sim_bench.md: what the LiDAR simulator (csrc/lidar_sim.hip) costs for the HDL64E model (64 x 2048 rays) on a
street scene: device time per launch (cull, cast, emit) and per frame for a batch of --frames poses, next to the numpy
restatement (tests/lidar_sim_restated.py, float32 form) on --cpu-rays rays of one frame, scaled to a frame.  Device time
between two events, median [min, max] of --reps runs after --warmup.  A report of one run, not a target.
--accuracy: only turn test_logs/lidar_sim_errors.log, which the tests write, into profiles/lidar_sim_accuracy.md.

  python scripts/lidar_sim_bench.py [--frames 16] [--blocks 3 3] [--reps 10] [--warmup 3] [--cpu-rays 4096] | --accuracy
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

DEV = "cuda"


def accuracy_md():
    src = os.path.join(ROOT, "test_logs", "lidar_sim_errors.log")
    if not os.path.exists(src):
        return False
    lines = list(dict.fromkeys(open(src).read().splitlines()))
    with open(os.path.join(ROOT, "profiles", "lidar_sim_accuracy.md"), "w") as f:
        f.write("# LiDAR simulator: observed errors\n\nEvery comparison tests/test_lidar_sim_host.py and tests/test_gpu_lidar_sim.py "
                "made, as they logged it; the bounds are stated in those files.  The simulator has no counterpart in the reference: "
                "it is pinned to this project's own numpy restatement (tests/lidar_sim_restated.py) -- its float32 form, which "
                "follows the kernels' order of operations (bit for bit), and its independent float64 form in world coordinates "
                "(ids equal, 1 mm, on the rays whose id survives a tilt of 1e-5 rad).\n\n```\n")
        f.write("\n".join(lines) + "\n```\n")
    return True


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--blocks", type=int, nargs=2, default=[3, 3])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-rays", type=int, default=4096)
    ap.add_argument("--accuracy", action="store_true")
    a = ap.parse_args()
    if a.accuracy:
        sys.exit(0 if accuracy_md() else "test_logs/lidar_sim_errors.log not found: run the tests first")
    if not torch.cuda.is_available():
        sys.exit("lidar_sim_bench.py measures on a GPU; none is visible")
    import lidar_sim_restated as RS
    from deeppointmap_amd import lidar_sim as LS, ops
    m = LS.HDL64E
    scene = LS.street_scene(0, blocks=tuple(a.blocks))
    all_poses = LS.circuit(scene, 2.0)
    poses = all_poses[np.linspace(0, len(all_poses) - 1, a.frames).astype(int)]
    sd = scene.to_device(DEV)
    dirs = torch.from_numpy(m.directions()).to(DEV)
    dp = torch.from_numpy(poses).to(DEV)
    F, P = a.frames, scene.P
    cull = lambda: ops.lidar_cull(sd.prims, sd.kind, sd.ground, dp, m.max_range, max(P, 1))
    kept, plane, status = cull()
    cast = lambda: ops.lidar_cast(kept, plane, status, P, dirs, m.min_range, m.max_range)
    out = cast()
    emit = lambda: ops.lidar_emit(*out, dirs, sd.albedo, sd.class_id)
    count = emit()[2]
    rows = [("dpm_lidar_cull", timed(cull, a.reps, a.warmup)), ("dpm_lidar_cast", timed(cast, a.reps, a.warmup)),
            ("dpm_lidar_emit", timed(emit, a.reps, a.warmup)),
            ("all three", timed(lambda: ops.lidar_emit(*ops.lidar_cast(*cull(), P, dirs, m.min_range, m.max_range), dirs,
                                                       sd.albedo, sd.class_id), a.reps, a.warmup))]
    prims, kind, ground, _, _ = scene.arrays()
    rays = np.arange(a.cpu_rays) * (m.rays // a.cpu_rays)
    t0 = time.perf_counter()
    RS.simulate32(prims, kind, ground, poses[:1], m.directions(), m.min_range, m.max_range, rays=rays)
    cpu_ms = (time.perf_counter() - t0) * 1e3 * (m.rays / a.cpu_rays)
    with open(os.path.join(ROOT, "profiles", "lidar_sim_bench.md"), "w") as f:
        f.write("# LiDAR simulator: time per launch and per frame\n\n")
        f.write(f"`python scripts/lidar_sim_bench.py --frames {F} --blocks {a.blocks[0]} {a.blocks[1]}` on {torch.cuda.get_device_name(0)} "
                f"(torch {torch.__version__}): HDL64E, {m.rays} rays a frame, a street scene of {P} primitives "
                f"({int(status[:, 0].min())} to {int(status[:, 0].max())} within range of a frame), {F} frames a batch, "
                f"{int(count.min())} to {int(count.max())} returns a frame.  Device time between two events, median [min, max] ms of "
                f"{a.reps} runs after {a.warmup} warm-up runs.  A report, not a target.\n\n| launch | ms per batch | ms per frame |\n|---|---|---|\n")
        for what, (med, lo, hi) in rows:
            f.write(f"| {what} | {med:.3f} [{lo:.3f}, {hi:.3f}] | {med / F:.4f} |\n")
        f.write(f"\nThe numpy restatement (float32 form, one thread of the host) casts {a.cpu_rays} rays of one frame in "
                f"{cpu_ms * a.cpu_rays / m.rays:.1f} ms: {cpu_ms:.0f} ms scaled to a frame of {m.rays} rays.\n")
    for r in rows:
        print(r, flush=True)
    print("numpy restatement, ms per frame (scaled):", cpu_ms)


if __name__ == "__main__":
    main()
