"""Rebuilding the local map from stored keyframes (dpm_local_map_insert_frames, csrc/local_map.hip) at HDL64E size: F frames of
lidar_sim.street_scene(2), 64 beams x 2048 columns, one metre apart along the circuit, thinned as LoopCloser stores them
(voxel_sample 0.5, the first 8192 valid rows) into a channel-major store (F,3,8192), each under its exact pose.
  rebuild          LocalMap.rebuild around the middle frame: init (both halves emptied) + claim + commit, two + two launches
  insert_frames    the claim + commit alone, into the emptied table (the init is timed apart)
  sequential       the same input through today's per-frame path: F x LocalMap.insert (two launches each) + one prune, on a
                   table large enough to take every frame's voxels before the prune drops most of them
  shortcut         insert_frames without and with a read-before-atomic shortcut in the claim: the shipped library (every offer is
                   one atomicMin) against a second build of it (--other-lib; csrc/build.py --out <lib>) whose claim has
                       if (__hip_atomic_load(o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < word) return;
                   before the atomicMin(o, word), alternating in one process on the same emptied table.  Without that
                   library only the shipped form is timed.
Device time between two events, median [min, max] of --reps runs after --warmup.  A report, not a threshold; written to
profiles/local_map_rebuild_bench.md.

  python scripts/local_map_rebuild_bench.py [--frames 50 200] [--reps 9] [--warmup 3] [--other-lib PATH]
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

sys.path.insert(0, os.path.join(ROOT, "scripts"))
from icp_bench import timed  # noqa: E402

DEV = "cuda"
OTHER = os.path.join(ROOT, "deeppointmap_amd", "csrc", "build", "libdpm_hip_frames_other.so")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[50, 200])
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--other-lib", default=OTHER, help="a build of the library whose claim reads the owner word first")
    ap.add_argument("--other-name", default="with the shortcut")
    ap.add_argument("--shipped-name", default="without the shortcut (shipped)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("local_map_rebuild_bench.py measures on a GPU; none is visible")
    from deeppointmap_amd import _lib, augment, lidar_sim as LS, ops
    from deeppointmap_amd.odometry import LocalMap, _copy, _pose_tensor
    scene, model = LS.street_scene(2), LS.HDL64E
    F, P = max(a.frames), a.points
    truth = LS.circuit(scene, spacing=1.0)[:F]
    F = len(truth)
    sim = LS.LidarSimulator(scene, model, device=DEV)
    store = torch.zeros(F, 3, P, device=DEV)
    lengths = torch.zeros(F, device=DEV, dtype=torch.int32)
    clouds = []
    for k, f in enumerate(sim.frames(truth)):
        work = augment.voxel_sample(_copy(f), 0.5)
        n = min(work.cap, P)
        store[k, :, :n] = work.xyz[:n].t()
        lengths[k:k + 1] = torch.clamp(work.count, min=0, max=n)
        clouds.append(augment.PointCloud.from_buffers(store[k].t().contiguous(), torch.arange(P, device=DEV, dtype=torch.int32),
                                                      lengths[k:k + 1].clone()))
    held = lengths.cpu().numpy()
    other = None
    if os.path.exists(a.other_lib):
        other = ctypes.CDLL(a.other_lib).dpm_local_map_insert_frames
        other.restype, other.argtypes = _lib.SIGNATURES["dpm_local_map_insert_frames"]
    kw = dict(voxel_size=1.0, subdivisions=3, max_range=model.max_range)
    out = []
    for n in [v for v in a.frames if v <= F]:
        rows = list(range(n))
        centre = truth[n // 2]
        poses = truth[:n]
        m = LocalMap(max_voxels=1 << 18, origin=centre[:3, 3], device=DEV, **kw)
        m._ready(torch.device(DEV))
        big = LocalMap(max_voxels=1 << 20, origin=centre[:3, 3], device=DEV, **kw)
        big._ready(torch.device(DEV))
        rebuild = timed(lambda: m.rebuild(store, lengths, rows, poses, centre), a.reps, a.warmup)
        m.check()
        cells, ref = m.n_points, [x.tobytes() for x in m.export()]
        init = timed(lambda: ops.local_map_clear(m.table, m.max_voxels, m.subdivisions), a.reps, a.warmup)

        def sequential():
            ops.local_map_clear(big.table, big.max_voxels, big.subdivisions)
            big.half = 0
            for k in rows:
                big.stamp = k
                big.insert(clouds[k], poses[k])
            big.prune(centre)
        seq = timed(sequential, a.reps, a.warmup)
        big.check()
        assert [x.tobytes() for x in big.export()] == ref, "the sequential path gives other bytes"
        big_init = timed(lambda: ops.local_map_clear(big.table, big.max_voxels, big.subdivisions), a.reps, a.warmup)
        # the two forms of the claim, alternating: each run clears the table outside the timed window
        dev_rows = torch.tensor(rows, device=DEV, dtype=torch.int32)
        dev_poses, dev_centre = torch.from_numpy(np.ascontiguousarray(poses)).to(DEV), _pose_tensor(centre, DEV)
        m.half = 0
        origin = (ctypes.c_double * 3)(*m.origin)
        args = (m.table.data_ptr(), m.max_voxels, m.subdivisions, 0, m.voxel_size, ctypes.addressof(origin), store.data_ptr(),
                lengths.data_ptr(), F, P, dev_rows.data_ptr(), dev_poses.data_ptr(), dev_rows.data_ptr(), n, dev_centre.data_ptr(),
                m.max_range, m.min_range, m.max_range, torch.cuda.current_stream().cuda_stream)
        forms = {a.shipped_name: _lib.load().dpm_local_map_insert_frames}
        if other is not None:
            forms[a.other_name] = other
        ms = {name: [] for name in forms}
        for rep in range(a.warmup + a.reps):
            for name, fn in forms.items():
                ops.local_map_clear(m.table, m.max_voxels, m.subdivisions)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.check(fn(*args), "dpm_local_map_insert_frames")
                e1.record()
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    ms[name].append(e0.elapsed_time(e1))
                if rep == a.warmup + a.reps - 1:
                    assert [x.tobytes() for x in m.export()] == ref, name + ": other bytes"
        out.append(dict(n=n, points=int(held[:n].sum()), cells=cells, rebuild=rebuild, init=init, seq=seq, big_init=big_init,
                        forms={k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ms.items()}))
    fmt = lambda t: f"{t[0]:.3f} [{t[1]:.3f}, {t[2]:.3f}]"
    path = os.path.join(ROOT, "profiles", "local_map_rebuild_bench.md")
    with open(path, "w") as f:
        f.write("# Rebuilding the local map from stored keyframes: one batched insert against the per-frame path\n\n")
        f.write(f"`python scripts/local_map_rebuild_bench.py --frames {' '.join(str(v) for v in a.frames)}` on {torch.cuda.get_device_name(0)} "
                f"(torch {torch.__version__}): street_scene(2), HDL64E frames one metre apart, thinned with voxel_sample 0.5 into a store "
                f"({F},3,{P}); voxel 1.0 m, 3^3 sub-cells, centre = the middle frame's pose, radius = max_range {model.max_range:g} m; "
                f"device time between two events, median [min, max] ms of {a.reps} runs after {a.warmup} warm-up runs.  A report, not a "
                "threshold.  Every path's sorted export was compared with the rebuild's: the same bytes.\n\n")
        f.write("| frames | stored points | cells held | rebuild (init + 2 launches), 2^18 slots | init alone, 2^18 slots | "
                "F x insert + prune (2 F + 2 launches, init included), 2^20 slots | init alone, 2^20 slots |\n|---|---|---|---|---|---|---|\n")
        for r in out:
            f.write(f"| {r['n']} | {r['points']} | {r['cells']} | {fmt(r['rebuild'])} | {fmt(r['init'])} | {fmt(r['seq'])} | {fmt(r['big_init'])} |\n")
        f.write("\nThe claim with and without reading the owner word before the atomicMin (claim + commit into an emptied table, "
                "alternating in one process):\n\n| frames | " + " | ".join(out[0]["forms"]) + " |\n|---|" + "---|" * len(out[0]["forms"]) + "\n")
        for r in out:
            f.write(f"| {r['n']} | " + " | ".join(fmt(t) for t in r["forms"].values()) + " |\n")
        if other is None:
            f.write("\nThe second build of the library was not there: only the shipped form was timed.\n")
        f.write("\nThe per-frame path needs the larger table: every frame's voxels take a slot before the prune drops those outside the "
                "radius.  Not measured: hardware counters of the new kernels, other sensors, other radii.\n")
    print(open(path).read())


if __name__ == "__main__":
    main()
