"""The TSDF surface map (csrc/tsdf_map.hip) at HDL64E size: frames of lidar_sim.street_scene(2), 64 beams x 2048 columns, one
metre apart along the circuit, under their exact poses; voxel 0.2 m, truncation 0.6 m, step 0.1 m (TsdfMap's defaults).
  integrate          dpm_tsdf_integrate of one whole frame (131072 rows) into an emptied table, in two forms of the atomics,
                     alternating in one process: the shipped library (every lane of a wave walks the samples together, runs of
                     neighbouring lanes with one key are summed by a segmented suffix sum over shuffles, and the first lane of
                     a run adds the run's sum and count) against a second build of it (--other-lib; csrc/build.py --out <lib>)
                     in the plain form, which was written first: a lane leaves the loop's body as soon as its sample is
                     skipped, and every kept sample is one 64-bit and one 32-bit atomic add of its own.  Without that library
                     only the shipped form is timed.  The plane-distance form (dpm_tsdf_integrate_planes, normals from
                     dpm_point_normals within --normals-radius, computed outside the window) alternates with them, into a
                     map of its own.
  local map insert   dpm_local_map_insert of the same frame (voxel 1 m, 3^3 sub-cells) alongside as a yardstick: one point
                     per row against the TSDF's up to 13 samples per row.
  integrate_frames   dpm_tsdf_integrate_frames of 50 and 200 stored frames, thinned as LoopCloser stores them (voxel_sample 0.5,
                     the first 8192 valid rows), in one launch into an emptied table
  surface, mesh      dpm_tsdf_surface and dpm_tsdf_mesh on that result, outputs sized by a counting pass first
  carve              on the map of the first 50 stored frames: dpm_tsdf_carve of the one whole frame and dpm_tsdf_carve_frames of
                     the 50 stored frames (weight 1, margin truncation + voxel), alternating; lookups only, so the map's keys
                     stay and only sums and counts grow from run to run.  A second build whose carve merges equal keys within a
                     wave (--carve-lib) alternates with the shipped one when it is there.
Device time between two events, median [min, max] of --reps runs after --warmup; the spread is the [min, max].  A report, not
a threshold: no time is asserted.  Written to profiles/tsdf_bench.md.

  python scripts/tsdf_bench.py [--frames 50 200] [--reps 21] [--warmup 3] [--other-lib PATH] [--carve-lib PATH]
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
CARVE_OTHER = os.path.join(ROOT, "deeppointmap_amd", "csrc", "build", "libdpm_hip_carve_merged.so")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[50, 200])
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--other-lib", default=OTHER, help="a build of the library whose integrate has the plain form")
    ap.add_argument("--carve-lib", default=CARVE_OTHER, help="a build of the library whose carve merges equal keys within a wave")
    ap.add_argument("--normals-radius", type=float, default=0.5)
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
    # the plane-distance form beside them, into a map of its own (its counts are in other units)
    mp = TsdfMap(max_voxels=1 << 22, max_range=model.max_range, origin=truth[0][:3, 3], device=DEV, distance="plane")
    mp._ready(torch.device(DEV))
    n_first = int(first.count.item())
    one = torch.full((1,), n_first, dtype=torch.int32, device=DEV)
    normals = torch.zeros_like(first.xyz)
    normals[:n_first] = ops.icp_target_normals(first.xyz[:n_first].t().contiguous()[None], one, one[:0], a.normals_radius,
                                               host=([0], [n_first]))[0]
    plane_name = f"plane distance, normals within {a.normals_radius:g} m given (dpm_tsdf_integrate_planes)"
    plane_args = (mp.table.data_ptr(), mp.max_voxels, mp.voxel_size, ctypes.addressof(origin), first.xyz.data_ptr(), normals.data_ptr(),
                  first.count.data_ptr(), first.cap, pose0.data_ptr(), mp.min_range, mp.max_range, mp.truncation, mp.step, 0.0, stream)
    calls = {name: (fn, args, m) for name, fn in forms.items()}
    calls[plane_name] = (_lib.load().dpm_tsdf_integrate_planes, plane_args, mp)
    ms, ref = {name: [] for name in calls}, None
    for rep in range(a.warmup + a.reps):
        for name, (fn, fargs, fm) in calls.items():
            ops.tsdf_clear(fm.table, fm.max_voxels)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(fn(*fargs), "dpm_tsdf_integrate")
            e1.record()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
            if rep == 0 and fm is m:
                got = [x.tobytes() for x in m.check().export()]
                ref = got if ref is None else ref
                assert got == ref, name + ": other bytes"
    frame = {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ms.items()}
    plane_voxels, plane_unusable = len(mp.check().export()[0]), mp.unusable()
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
    # -- carving, on the map of the first 50 stored frames (or of all of them, if there are fewer)
    nc = min(50, F)
    g = TsdfMap(max_voxels=1 << 22, max_range=model.max_range, origin=truth[nc // 2][:3, 3], device=DEV)
    dev_rows, dev_poses = torch.arange(nc, device=DEV, dtype=torch.int32), torch.from_numpy(np.ascontiguousarray(truth[:nc])).to(DEV)
    g.integrate_frames(store, lengths, dev_rows, dev_poses).check()
    g_origin = (ctypes.c_double * 3)(*g.origin)
    margin = g.truncation + g.voxel_size
    head = (g.table.data_ptr(), g.max_voxels, g.voxel_size, ctypes.addressof(g_origin))
    tail = (g.min_range, g.max_range, g.truncation, g.step, 1, margin, stream)
    carve_args = {"dpm_tsdf_carve": head + (first.xyz.data_ptr(), first.count.data_ptr(), first.cap, pose0.data_ptr()) + tail,
                  "dpm_tsdf_carve_frames": head + (store.data_ptr(), lengths.data_ptr(), F, P, dev_rows.data_ptr(), dev_poses.data_ptr(), nc) + tail}
    libs = {"one lane a ray, every lookup its own (shipped)": _lib.load()}
    if os.path.exists(a.carve_lib):
        libs["equal keys of a wave merged before the lookup"] = ctypes.CDLL(a.carve_lib)
    carve_ms = {(lib, entry): [] for lib in libs for entry in carve_args}
    counts0 = g.export()[2].astype(np.int64)
    reached = {}
    for rep in range(a.warmup + a.reps):
        for lib, handle in libs.items():
            for entry, cargs in carve_args.items():
                fn = getattr(handle, entry)
                fn.restype, fn.argtypes = _lib.SIGNATURES[entry]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.check(fn(*cargs), entry)
                e1.record()
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    carve_ms[(lib, entry)].append(e0.elapsed_time(e1))
                if rep == 0:
                    counts1 = g.export()[2].astype(np.int64)
                    reached[(lib, entry)] = (int((counts1 != counts0).sum()), int((counts1 - counts0).sum()))
                    counts0 = counts1
    carve_t = {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in carve_ms.items()}
    for entry in carve_args:
        assert len({reached[(lib, entry)] for lib in libs}) == 1, (entry, reached)     # both forms added the same weight to as many voxels
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
        f.write(f"The plane-distance map of that frame holds {plane_voxels} voxels; {plane_unusable} of the {rows} rows had no usable normal "
                "(none within the radius, or 256 |cos incidence| < 0.5).  The normals are computed outside the window.\n\n")
        f.write(f"## Lists of stored frames ({P} columns a frame, thinned with voxel_sample 0.5), and the extractions on the result\n\n")
        f.write("| frames | stored points | voxels | dpm_tsdf_init + dpm_tsdf_integrate_frames (one launch) | surface records | "
                "dpm_tsdf_surface (count read included) | triangles | dpm_tsdf_mesh (count read included) |\n|---|---|---|---|---|---|---|---|\n")
        for r in out:
            f.write(f"| {r['n']} | {r['points']} | {r['voxels']} | {fmt(r['fuse'])} | {r['records']} | {fmt(r['surface'])} | {r['triangles']} | "
                    f"{fmt(r['mesh'])} |\n")
        f.write(f"\n## Free-space carving into the map of {nc} stored frames ({len(counts0)} voxels; weight 1, margin {margin:g} m)\n\n")
        f.write("Lookups only: the keys stay, sums and counts grow from run to run.  The calls alternated in one process.\n\n")
        f.write("| form | call | voxels reached | samples added | ms |\n|---|---|---|---|---|\n")
        what = {"dpm_tsdf_carve": f"dpm_tsdf_carve of the one whole frame ({rows} rows)",
                "dpm_tsdf_carve_frames": f"dpm_tsdf_carve_frames of the {nc} stored frames ({int(held[:nc].sum())} rows, one launch)"}
        for (lib, entry), t in carve_t.items():
            f.write(f"| {lib} | {what[entry]} | {reached[(lib, entry)][0]} | {reached[(lib, entry)][1]} | {fmt(t)} |\n")
        if len(libs) == 1:
            f.write("\nThe second build of the library was not there: only the shipped form of the carve was timed.\n")
        f.write("\nNot measured: hardware counters of the new kernels, other sensors, other voxel sizes, a table near its capacity.\n")
    print(open(path).read())


if __name__ == "__main__":
    main()
