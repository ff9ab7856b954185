"""The batched ICP (csrc/icp.hip) on --pairs pairs of consecutive synthetic scans of --points points (synthetic.py, metres):
  grids            the call with no iteration: target grids only
  per iteration    (time of --iters iterations with the stop rule off - grids) / iters, both metrics
  per pair         a default run (30 iterations at most, default tolerances, plane metric) divided by the number of pairs
  search only      dpm_infomat_search_grids on the same pairs and poses: the yardstick for the accumulate stage
Device time between two events, median [min, max] of --reps runs after --warmup.  Reports, not thresholds; written to
profiles/icp_bench.md.  --accuracy: only turn test_logs/icp_errors.log, which tests/test_gpu_icp.py writes, into
profiles/icp_accuracy.md.

  python scripts/icp_bench.py [--pairs 64] [--points 65536] [--iters 10] [--reps 5] [--warmup 2] | --accuracy
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
    src = os.path.join(ROOT, "test_logs", "icp_errors.log")
    if not os.path.exists(src):
        return False
    lines = list(dict.fromkeys(open(src).read().splitlines()))
    with open(os.path.join(ROOT, "profiles", "icp_accuracy.md"), "w") as f:
        f.write("# Batched ICP: observed errors\n\nEvery comparison tests/test_gpu_icp.py made on the GPU, as it logged it; the "
                "bounds are derived in that file.  `r32` / `r64`: the numpy restatement of the algorithm (tests/icp_restated.py) "
                "in float32 and float64.  Pinned to that restatement and to scenes with a known answer -- not to the third-party "
                "ICP that made the reference's tables, which cannot be run here.\n\n```\n")
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
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--points", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--accuracy", action="store_true")
    a = ap.parse_args()
    if a.accuracy:
        sys.exit(0 if accuracy_md() else "test_logs/icp_errors.log not found: run the GPU tests first")
    if not torch.cuda.is_available():
        sys.exit("icp_bench.py measures on a GPU; none is visible")
    from deeppointmap_amd import ops, synthetic
    P, N = a.pairs, a.points
    pts, _ = synthetic.frames(P + 1, N)
    pcd = (pts * synthetic.COOR_SCALE).to(DEV).contiguous()
    lengths = torch.full((P + 1,), N, dtype=torch.int32, device=DEV)
    src = torch.arange(1, P + 1, dtype=torch.int32, device=DEV)
    dst = torch.arange(0, P, dtype=torch.int32, device=DEV)
    truth = torch.stack([synthetic.relative_pose(f + 1, f) for f in range(P)])
    init = truth.clone()
    init[:, :3, 3] += torch.tensor([0.1, -0.05, 0.02], dtype=torch.float64)   # a start a decimetre off
    init = init.to(DEV)
    normals = ops.icp_target_normals(pcd, lengths, dst, 1.0)
    rows = []

    def icp(metric, schedule, **kw):
        return lambda: ops.icp_refine(pcd, lengths, src, dst, init, schedule, metric, normals=normals, **kw)
    grids = timed(icp(ops.ICP_POINT, [(1.0, 0)]), a.reps, a.warmup)
    rows.append(("grids (no iteration)", grids, None))
    for name, metric in (("point", ops.ICP_POINT), ("plane", ops.ICP_PLANE)):
        t = timed(icp(metric, [(1.0, a.iters)], tol_rot=0.0, tol_trans=0.0), a.reps, a.warmup)
        rows.append((f"{a.iters} iterations, {name} metric, stop rule off", t, (t[0] - grids[0]) / a.iters))
    out = ops.icp_refine(pcd, lengths, src, dst, init, [(1.0, 30)], ops.ICP_PLANE, normals=normals)
    t = timed(icp(ops.ICP_PLANE, [(1.0, 30)]), a.reps, a.warmup)
    rows.append(("default run (plane, 30 iterations at most)", t, None))
    pose = out[0].cpu()
    err = float((pose[:, :3, 3] - truth[:, :3, 3]).norm(dim=1).max())
    Rt = torch.cat([init[:, :3, :3].reshape(P, 9), init[:, :3, 3]], dim=1).float().contiguous()
    info = torch.empty(P, 36, device=DEV)
    g = ops.information_matrix_grids(pcd, dst, 1.0)
    search = timed(lambda: ops.information_matrix_batched(pcd, src, dst, Rt, info, 1.0, grids=g), a.reps, a.warmup)
    rows.append(("dpm_infomat_search_grids, same pairs and poses", search, None))
    with open(os.path.join(ROOT, "profiles", "icp_bench.md"), "w") as f:
        f.write("# Batched ICP: time per iteration and per pair\n\n")
        f.write(f"`python scripts/icp_bench.py --pairs {P} --points {N} --iters {a.iters}` on {torch.cuda.get_device_name(0)} (torch "
                f"{torch.__version__}): {P} pairs of consecutive synthetic scans, max_dist 1.0 m, start 0.11 m off; device time "
                f"between two events, median [min, max] ms of {a.reps} runs after {a.warmup} warm-up runs.  Reports, not "
                "thresholds.\n\n| what | ms | ms per iteration (all pairs) |\n|---|---|---|\n")
        for what, (med, lo, hi), per in rows:
            f.write(f"| {what} | {med:.3f} [{lo:.3f}, {hi:.3f}] | {'' if per is None else f'{per:.3f}'} |\n")
        f.write(f"\nDefault run: {rows[3][1][0] / P:.4f} ms per pair; iterations taken {out[3].min().item()} to {out[3].max().item()}, "
                f"status counts {np.bincount(out[4].cpu().numpy(), minlength=4).tolist()} (converged, max_iter, no_match, singular); "
                f"largest distance of a refined translation from the generating pose {err:.4f} m (the scans carry 0.01 m jitter).\n"
                f"The accumulate stage against the search it is modelled on: {rows[1][2]:.3f} (point) / {rows[2][2]:.3f} (plane) ms per "
                f"iteration against {search[0]:.3f} ms for one information-matrix search.\n")
    for r in rows:
        print(r, flush=True)


if __name__ == "__main__":
    main()
