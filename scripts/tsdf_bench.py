"""The TSDF surface map (csrc/tsdf_map.hip) at HDL64E size: frames of lidar_sim.street_scene(2), 64 beams x 2048 columns, one
metre apart along the circuit, under their exact poses; voxel 0.2 m, truncation 0.6 m, step 0.1 m (TsdfMap's defaults).
  integrate          dpm_tsdf_integrate of one whole frame (131072 rows) into an emptied table, in two forms of the atomics,
                     alternating in one process: the shipped library (every lane of a wave walks the samples together, runs of
                     neighbouring lanes with one key are summed by a segmented suffix sum over shuffles, and the first lane of
                     a run adds the run's sum and count) against a second build of it (--other-lib; csrc/build.py --out <lib>)
                     in the plain form, which was written first: a lane leaves the loop's body as soon as its sample is
                     skipped, and every kept sample is one 64-bit and one 32-bit atomic add of its own.  Without that library
                     only the shipped form is timed.
  local map insert   dpm_local_map_insert of the same frame (voxel 1 m, 3^3 sub-cells) alongside as a yardstick: one point
                     per row against the TSDF's up to 13 samples per row.
  integrate_frames   dpm_tsdf_integrate_frames of 50 and 200 stored frames, thinned as LoopCloser stores them (voxel_sample 0.5,
                     the first 8192 valid rows), in one launch into an emptied table
  surface, mesh      dpm_tsdf_surface and dpm_tsdf_mesh on that result, outputs sized by a counting pass first
Device time between two events, median [min, max] of --reps runs after --warmup; the spread is the [min, max].  A report, not
a threshold: no time is asserted.  Written to profiles/tsdf_bench.md.

  python scripts/tsdf_bench.py [--frames 50 200] [--reps 21] [--warmup 3] [--other-lib PATH]
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
OTHER = os.path.join(ROOT, "deeppointmap_amd", "csrc", "build", "libdpm_hip_tsdf_plain.so")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[50, 200])
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--other-lib", default=OTHER, help="a build of the library whose integrate has the plain form")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tsdf_bench.py measures on a GPU; none is visible")
    from deeppointmap_amd import _lib, augment, lidar_sim as LS, ops
    from deeppointmap_amd.odometry import LocalMap, _copy, _pose_tensor
    from deeppointmap_amd.tsdf import TsdfMap
    scene, model = LS.street_scene(2), LS.HDL64E
    F, P = max(a.frames), a.points
    truth = LS.circuit(scene, spacing=1.0)[:F]
    F = len(truth)
    sim = LS.LidarSimulator(scene, model, device=DEV)
    store = torch.zeros(F, 3, P, device=DEV)
    lengths = torch.zeros(F, device=DEV, dtype=torch.int32)
    first = None
    for k, f in enumerate(sim.frames(truth)):
        if k == 0:
            first = _copy(f)
        work = augment.voxel_sample(_copy(f), 0.5)
        n = min(work.cap, P)
        store[k, :, :n] = work.xyz[:n].t()
        lengths[k:k + 1] = torch.clamp(work.count, min=0, max=n)
    held = lengths.cpu().numpy()
    stream = torch.cuda.current_stream().cuda_stream
    fmt = lambda t: f"{t[0]:.3f} [{t[1]:.3f}, {t[2]:.3f}]"

    # -- one whole frame, both forms of the atomics, alternating
    m = TsdfMap(max_voxels=1 << 22, max_range=model.max_range, origin=truth[0][:3, 3], device=DEV)
    m._ready(torch.device(DEV))
    pose0 = _pose_tensor(truth[0], DEV)
    origin = (ctypes.c_double * 3)(*m.origin)
    args = (m.table.data_ptr(), m.max_voxels, m.voxel_size, ctypes.addressof(origin), first.xyz.data_ptr(), first.count.data_ptr(),
            first.cap, pose0.data_ptr(), m.min_range, m.max_range, m.truncation, m.step, stream)
    forms = {"equal keys merged within a wave (shipped)": _lib.load().dpm_tsdf_integrate}
    if os.path.exists(a.other_lib):
        other = ctypes.CDLL(a.other_lib).dpm_tsdf_integrate
        other.restype, other.argtypes = _lib.SIGNATURES["dpm_tsdf_integrate"]
        forms["plain: one pair of atomics a sample"] = other
    ms, ref = {name: [] for name in forms}, None
    for rep in range(a.warmup + a.reps):
        for name, fn in forms.items():
            ops.tsdf_clear(m.table, m.max_voxels)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(fn(*args), "dpm_tsdf_integrate")
            e1.record()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
            if rep == 0:
                got = [x.tobytes() for x in m.check().export()]
                ref = got if ref is None else ref
                assert got == ref, name + ": other bytes"
    frame = {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ms.items()}
    rows, voxels, samples = int(first.count.item()), len(m.export()[0]), int(m.export()[2].astype(np.int64).sum())
    clear = timed(lambda: ops.tsdf_clear(m.table, m.max_voxels), a.reps, a.warmup)
    lm = LocalMap(voxel_size=1.0, subdivisions=3, max_voxels=1 << 18, max_range=model.max_range, origin=truth[0][:3, 3], device=DEV)
    lm._ready(torch.device(DEV))
    lm_ms = []
    for rep in range(a.warmup + a.reps):
        ops.local_map_clear(lm.table, lm.max_voxels, lm.subdivisions)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.local_map_insert(*lm._args(), first.xyz, first.idx, first.count, pose0, 0, lm.min_range, lm.max_range)
        e1.record()
        torch.cuda.synchronize()
        if rep >= a.warmup:
            lm_ms.append(e0.elapsed_time(e1))
    lm_t = (sorted(lm_ms)[len(lm_ms) // 2], min(lm_ms), max(lm_ms))

    # -- lists of stored frames, then the extractions on the result
    out = []
    for n in [v for v in a.frames if v <= F]:
        g = TsdfMap(max_voxels=1 << 22, max_range=model.max_range, origin=truth[n // 2][:3, 3], device=DEV)
        g._ready(torch.device(DEV))
        dev_rows = torch.arange(n, device=DEV, dtype=torch.int32)
        dev_poses = torch.from_numpy(np.ascontiguousarray(truth[:n])).to(DEV)

        def fuse():
            ops.tsdf_clear(g.table, g.max_voxels)
            g.integrate_frames(store, lengths, dev_rows, dev_poses)
        both = timed(fuse, a.reps, a.warmup)
        g.check()
        n_vox, n_surf, n_tri = (ops.tsdf_export(g.table, g.max_voxels, 0), ops.tsdf_surface(g.table, g.max_voxels, g.voxel_size, 1, 0),
                                ops.tsdf_mesh(g.table, g.max_voxels, g.voxel_size, 1, 0))
        surface = timed(lambda: ops.tsdf_surface(g.table, g.max_voxels, g.voxel_size, 1, n_surf), a.reps, a.warmup)
        mesh = timed(lambda: ops.tsdf_mesh(g.table, g.max_voxels, g.voxel_size, 1, n_tri), a.reps, a.warmup)
        out.append(dict(n=n, points=int(held[:n].sum()), voxels=n_vox, records=n_surf, triangles=n_tri, fuse=both, surface=surface,
                        mesh=mesh))
    path = os.path.join(ROOT, "profiles", "tsdf_bench.md")
    with open(path, "w") as f:
        f.write("# The TSDF surface map at HDL64E size\n\n")
        f.write(f"`python scripts/tsdf_bench.py --frames {' '.join(str(v) for v in a.frames)}` on {torch.cuda.get_device_name(0)} (torch "
                f"{torch.__version__}): street_scene(2), HDL64E frames one metre apart under their exact poses; voxel {m.voxel_size} m, "
                f"truncation {m.truncation:g} m, step {m.step:g} m, 2^22 slots; device time between two events, median [min, max] ms of "
                f"{a.reps} runs after {a.warmup} warm-up runs: the [min, max] is the run-to-run spread.  A report, not a threshold.\n\n")
        f.write(f"## One whole frame: {rows} rows, {samples} samples into {voxels} voxels of an emptied table\n\n")
        f.write("The two forms of the atomics alternated in one process; their sorted exports were compared: the same bytes.\n\n")
        f.write("| form | dpm_tsdf_integrate, ms |\n|---|---|\n")
        for k, v in frame.items():
            f.write(f"| {k} | {fmt(v)} |\n")
        if len(frame) == 1:
            f.write("\nThe second build of the library was not there: only the shipped form was timed.\n")
        f.write(f"\n| alongside | ms |\n|---|---|\n| dpm_local_map_insert of the same frame (voxel 1 m, 3^3 sub-cells, 2^18 slots, emptied; "
                f"two launches) | {fmt(lm_t)} |\n| dpm_tsdf_init of the 2^22 slots (outside the windows above) | {fmt(clear)} |\n\n")
        f.write(f"## Lists of stored frames ({P} columns a frame, thinned with voxel_sample 0.5), and the extractions on the result\n\n")
        f.write("| frames | stored points | voxels | dpm_tsdf_init + dpm_tsdf_integrate_frames (one launch) | surface records | "
                "dpm_tsdf_surface (count read included) | triangles | dpm_tsdf_mesh (count read included) |\n|---|---|---|---|---|---|---|---|\n")
        for r in out:
            f.write(f"| {r['n']} | {r['points']} | {r['voxels']} | {fmt(r['fuse'])} | {r['records']} | {fmt(r['surface'])} | {r['triangles']} | "
                    f"{fmt(r['mesh'])} |\n")
        f.write("\nNot measured: hardware counters of the new kernels, other sensors, other voxel sizes, a table near its capacity.\n")
    print(open(path).read())


if __name__ == "__main__":
    main()
