"""Ray-casting the TSDF map (csrc/tsdf_map.hip: dpm_tsdf_raycast, dpm_tsdf_blocks) at HDL64E size: the 64 x 2048 directions of
lidar_sim.HDL64E from 1 and from 16 poses of the circuit of street_scene(2), against the maps of 50 and 200 stored frames that
scripts/tsdf_bench.py builds (voxel 0.2 m, truncation 0.6 m; thinned frames one metre apart under their exact poses).  The ray
is sampled every 0.1 m (the map's step) from 0.9 to 120 m (the sensor's limits): 1192 samples a ray.
  plain / blocks     dpm_tsdf_raycast with blocks = NULL (the 8 lookups of every sample, of which an empty one ends at the first)
                     and with the occupied-block set, alternating in one process; their outputs are compared: the same bytes.
  block build        dpm_tsdf_blocks alone (two launches), outside the windows above.
  lidar_cast         lidar_sim.cast_rays of the same rays from the same poses against the scene itself (cull + cast, two
                     launches), alongside: the exact answer the simulator has, at what cost.
Device time between two events, median [min, max] of --reps runs after --warmup; the spread is the [min, max].  A report, not a
threshold: no time is asserted.  Written to profiles/tsdf_raycast_bench.md.

  python scripts/tsdf_raycast_bench.py [--frames 50 200] [--poses 1 16] [--reps 11] [--warmup 2]
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
    ap.add_argument("--frames", type=int, nargs="+", default=[50, 200])
    ap.add_argument("--poses", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tsdf_raycast_bench.py measures on a GPU; none is visible")
    from deeppointmap_amd import augment, lidar_sim as LS, ops
    from deeppointmap_amd.odometry import _copy
    from deeppointmap_amd.tsdf import HIT, BACK, TsdfMap
    scene, model = LS.street_scene(2), LS.HDL64E
    F, P = max(a.frames), a.points
    truth = LS.circuit(scene, spacing=1.0)[:F]
    F = len(truth)
    sim = LS.LidarSimulator(scene, model, device=DEV)
    store = torch.zeros(F, 3, P, device=DEV)
    lengths = torch.zeros(F, device=DEV, dtype=torch.int32)
    for k, f in enumerate(sim.frames(truth)):
        work = augment.voxel_sample(_copy(f), 0.5)
        n = min(work.cap, P)
        store[k, :, :n] = work.xyz[:n].t()
        lengths[k:k + 1] = torch.clamp(work.count, min=0, max=n)
    scene_dev = scene.to_device(DEV)
    dirs = torch.from_numpy(model.directions()).to(DEV)
    fmt = lambda v: f"{sorted(v)[len(v) // 2]:.3f} [{min(v):.3f}, {max(v):.3f}]"

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    rows = []
    for n in [v for v in a.frames if v <= F]:
        g = TsdfMap(max_voxels=1 << 22, max_range=model.max_range, origin=truth[n // 2][:3, 3], device=DEV)
        g.integrate_frames(store, lengths, torch.arange(n, device=DEV, dtype=torch.int32),
                           torch.from_numpy(np.ascontiguousarray(truth[:n])).to(DEV)).check()
        voxels = ops.tsdf_export(g.table, g.max_voxels, 0)
        blocks = g.blocks(1)
        g.check()
        n_blocks = int((blocks[256:].view(torch.int64) != -1).sum().item())
        build = [window(lambda: ops.tsdf_blocks(g.table, g.max_voxels, 1, g.max_blocks, out=blocks))[0] for _ in range(a.warmup + a.reps)][a.warmup:]
        for n_poses in a.poses:
            pick = np.linspace(0, n - 1, n_poses + 2).astype(int)[1:-1]
            poses = torch.from_numpy(np.ascontiguousarray(truth[pick])).to(DEV)
            args = (model.min_range, model.max_range, g.step, 1)
            forms = {"plain": lambda: ops.tsdf_raycast(*g._map(), None, 0, poses, dirs, *args),
                     "blocks": lambda: ops.tsdf_raycast(*g._map(), blocks, g.max_blocks, poses, dirs, *args),
                     "lidar_cast": lambda: LS.cast_rays(scene_dev, poses, model, dirs=dirs)}
            ms, kept = {k: [] for k in forms}, {}
            for rep in range(a.warmup + a.reps):
                for name, fn in forms.items():
                    t, out = window(fn)
                    if rep >= a.warmup:
                        ms[name].append(t)
                    if rep == 0:
                        kept[name] = out
            for x, y in zip(kept["plain"], kept["blocks"]):
                assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), "the two forms differ"
            flag = kept["plain"][2]
            sim_hit = kept["lidar_cast"][1] >= 0
            rows.append(dict(n=n, voxels=voxels, blocks=n_blocks, poses=n_poses, rays=flag.numel(), hit=int((flag == HIT).sum()),
                             back=int((flag == BACK).sum()), sim_hit=int(sim_hit.sum()), ms={k: fmt(v) for k, v in ms.items()},
                             ratio=sorted(ms["plain"])[len(ms["plain"]) // 2] / sorted(ms["blocks"])[len(ms["blocks"]) // 2],
                             disjoint=min(ms["plain"]) > max(ms["blocks"]), build=fmt(build)))
            print(rows[-1], flush=True)
    K = int(np.floor((model.max_range - model.min_range) / 0.1)) + 1
    path = os.path.join(ROOT, "profiles", "tsdf_raycast_bench.md")
    with open(path, "w") as f:
        f.write("# Ray-casting the TSDF map at HDL64E size\n\n")
        f.write(f"`python scripts/tsdf_raycast_bench.py --frames {' '.join(str(v) for v in a.frames)} --poses {' '.join(str(v) for v in a.poses)}` "
                f"on {torch.cuda.get_device_name(0)} (torch {torch.__version__}): street_scene(2); the maps of scripts/tsdf_bench.py (stored "
                f"frames one metre apart under their exact poses, voxel 0.2 m, truncation 0.6 m, 2^22 slots, 2^21 block slots); the "
                f"{model.rays} directions of HDL64E from poses spread along the fused stretch; samples every 0.1 m from {model.min_range} to "
                f"{model.max_range:g} m ({K} a ray).  Device time between two events, median [min, max] ms of {a.reps} runs after {a.warmup} "
                "warm-up runs: the [min, max] is the run-to-run spread.  The three calls alternated in one process; the outputs of the "
                "plain form and of the block form were compared: the same bytes.  A report, not a threshold.\n\n")
        f.write("| frames fused | voxels | occupied blocks | poses | rays | HIT | BACK | the simulator's hits | plain: blocks = NULL, ms | with "
                "the block set, ms | plain / blocks (medians) | windows disjoint | dpm_tsdf_blocks alone, ms | lidar_sim.cast_rays of the same "
                "rays (cull + cast), ms |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['n']} | {r['voxels']} | {r['blocks']} | {r['poses']} | {r['rays']} | {r['hit']} | {r['back']} | {r['sim_hit']} | "
                    f"{r['ms']['plain']} | {r['ms']['blocks']} | {r['ratio']:.2f} | {'yes' if r['disjoint'] else 'no'} | {r['build']} | "
                    f"{r['ms']['lidar_cast']} |\n")
        f.write("\n\"Windows disjoint\": the slowest run of the block form was faster than the fastest run of the plain form.  HIT and BACK "
                "are what the map of thinned frames holds along the rays; the simulator's column is the scene's own answer.\n")
        f.write("\nNot measured: hardware counters of the new kernels, other sensors, other steps, a marcher that steps over whole blocks.\n")
    print(open(path).read())


if __name__ == "__main__":
    main()
