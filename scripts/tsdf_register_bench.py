"""Scan-to-TSDF registration (csrc/tsdf_map.hip: dpm_tsdf_register, dpm_tsdf_sample) at HDL64E size: one whole frame of
lidar_sim.street_scene(2), 64 beams x 2048 columns, against the plane-distance map of 50 stored frames one metre apart along the
circuit under their exact poses (thinned as LoopCloser stores them: voxel_sample 0.5, the first 8192 valid rows; normals from
dpm_point_normals within --normals-radius); voxel 0.2 m, truncation 0.6 m (TsdfMap's defaults).  The frame is the one taken at
the middle pose; the start is that pose 0.05 m and 0.2 degrees off.
  register x 1, x 10   dpm_tsdf_register with a schedule of 1 and of 10 iterations, tolerances 0 so that no run stops early; one
                       accumulate + solve iteration is (x 10 - x 1) / 9
  sample               dpm_tsdf_sample of the same frame under the start pose
  local map            dpm_local_map_register_planes of the same frame from the same start against the rolling point map of the
                       same 50 stored frames (voxel 1 m, 3^3 sub-cells, planes computed outside the window), x 1 and x 10
  second form          with --other-lib (csrc/build.py --out <lib>): a second build of the library whose field lookup issues the 8
                       first probes before any `sum` / `count` read; its three calls alternate with the shipped ones and the
                       10-iteration poses are compared byte for byte.  Without that library only the shipped form is timed.
All calls alternate in one process; device time between two events, median [min, max] of --reps runs after --warmup.  A report,
not a threshold: no time is asserted.  Written to profiles/tsdf_register_bench.md.

  python scripts/tsdf_register_bench.py [--frames 50] [--reps 21] [--warmup 3] [--other-lib PATH]
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

DEV = "cuda"
OTHER = os.path.join(ROOT, "deeppointmap_amd", "csrc", "build", "libdpm_hip_tsdf_probe_first.so")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--normals-radius", type=float, default=0.5)
    ap.add_argument("--other-lib", default=OTHER, help="a build of the library with the second form of the field lookup")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tsdf_register_bench.py measures on a GPU; none is visible")
    from deeppointmap_amd import _lib, augment, lidar_sim as LS, ops
    from deeppointmap_amd.odometry import LocalMap, _copy, _pose_tensor
    from deeppointmap_amd.tsdf import TsdfMap
    scene, model = LS.street_scene(2), LS.HDL64E
    P = a.points
    truth = LS.circuit(scene, spacing=1.0)[:a.frames]
    F = len(truth)
    mid = F // 2
    sim = LS.LidarSimulator(scene, model, device=DEV)
    store = torch.zeros(F, 3, P, device=DEV)
    lengths = torch.zeros(F, device=DEV, dtype=torch.int32)
    frame = None
    for k, f in enumerate(sim.frames(truth)):
        if k == mid:
            frame = _copy(f)
        work = augment.voxel_sample(_copy(f), 0.5)
        n = min(work.cap, P)
        store[k, :, :n] = work.xyz[:n].t()
        lengths[k:k + 1] = torch.clamp(work.count, min=0, max=n)
    rows_dev = torch.arange(F, device=DEV, dtype=torch.int32)
    poses_dev = torch.from_numpy(np.ascontiguousarray(truth)).to(DEV)
    normals = ops.icp_target_normals(store, lengths, rows_dev, a.normals_radius)
    origin = truth[mid][:3, 3]
    m = TsdfMap(max_voxels=1 << 22, max_range=model.max_range, origin=origin, device=DEV, distance="plane")
    m.integrate_frames(store, lengths, rows_dev, poses_dev, normals=normals).check()
    voxels = ops.tsdf_export(m.table, m.max_voxels, 0)
    lm = LocalMap(voxel_size=1.0, subdivisions=3, max_voxels=1 << 18, max_range=model.max_range, origin=origin, device=DEV)
    lm.insert_frames(store, lengths, rows_dev, poses_dev, stamps=list(range(F)))
    lm.check()
    planes, counts = lm.planes()

    th, d = np.radians(0.2), np.array([0.03, -0.03, 0.0265])
    off = np.eye(4)
    off[:3, :3] = [[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]]
    start = truth[mid].copy()
    start[:3, :3] = off[:3, :3] @ start[:3, :3]
    start[:3, 3] += d
    init = _pose_tensor(start, DEV)
    n_rows = int(frame.count.item())

    def tsdf_reg(iters):
        return ops.tsdf_register(*m._map(), m.truncation, frame.xyz, frame.count, init, [(m.truncation, iters)], 0.0, 0.0, 0.0, m.unit, 0.5)

    def lm_reg(iters):
        return ops.local_map_register_planes(*lm._args(), planes, counts, 5, 0.1, frame.xyz, frame.count, init, [(1.0, iters)], 0.0, 0.0, 0.0)

    calls = {
        "dpm_tsdf_register, 1 iteration": lambda: tsdf_reg(1),
        "dpm_tsdf_register, 10 iterations": lambda: tsdf_reg(10),
        "dpm_tsdf_sample": lambda: ops.tsdf_sample(*m._map(), frame.xyz, frame.count, init, m.unit),
        "dpm_local_map_register_planes, 1 iteration": lambda: lm_reg(1),
        "dpm_local_map_register_planes, 10 iterations": lambda: lm_reg(10),
    }
    # the same three calls through the C ABI of both builds, with outputs and workspace made once
    forms = {"plain, one corner after the other (shipped)": _lib.load()}
    if os.path.exists(a.other_lib):
        forms["the 8 first probes before any sum / count read"] = ctypes.CDLL(a.other_lib)
    o3 = (ctypes.c_double * 3)(*m.origin)
    stream = torch.cuda.current_stream().cuda_stream
    raw_pose = {}
    for form, lib in forms.items():
        reg, smp = lib.dpm_tsdf_register, lib.dpm_tsdf_sample
        reg.restype, reg.argtypes = _lib.SIGNATURES["dpm_tsdf_register"]
        smp.restype, smp.argtypes = _lib.SIGNATURES["dpm_tsdf_sample"]
        pose = torch.zeros(16, dtype=torch.float64, device=DEV)
        f2, i2 = torch.zeros(2, dtype=torch.float32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
        ws = torch.zeros(_lib.load().dpm_tsdf_register_scratch_bytes(frame.cap), dtype=torch.uint8, device=DEV)
        d, g, fl = (torch.zeros(frame.cap, device=DEV), torch.zeros(frame.cap, 3, device=DEV),
                    torch.zeros(frame.cap, dtype=torch.int32, device=DEV))
        raw_pose[form] = pose

        def raw_reg(iters, reg=reg, pose=pose, f2=f2, i2=i2, ws=ws):
            dist, its = (ctypes.c_double * 1)(m.truncation), (ctypes.c_int32 * 1)(iters)
            _lib.check(reg(m.table.data_ptr(), m.max_voxels, m.voxel_size, ctypes.addressof(o3), m.truncation, m.unit, 0.5,
                           frame.xyz.data_ptr(), frame.count.data_ptr(), frame.cap, init.data_ptr(), ctypes.addressof(dist),
                           ctypes.addressof(its), 1, 0.0, 0.0, 0.0, pose.data_ptr(), f2[:1].data_ptr(), f2[1:].data_ptr(),
                           i2[:1].data_ptr(), i2[1:].data_ptr(), None, None, ws.data_ptr(), stream), "dpm_tsdf_register")

        def raw_smp(smp=smp, d=d, g=g, fl=fl):
            _lib.check(smp(m.table.data_ptr(), m.max_voxels, m.voxel_size, ctypes.addressof(o3), frame.xyz.data_ptr(),
                           frame.count.data_ptr(), frame.cap, init.data_ptr(), m.unit, d.data_ptr(), g.data_ptr(), fl.data_ptr(), stream),
                       "dpm_tsdf_sample")
        calls[f"C ABI, {form}: dpm_tsdf_register, 1 iteration"] = lambda r=raw_reg: r(1)
        calls[f"C ABI, {form}: dpm_tsdf_register, 10 iterations"] = lambda r=raw_reg: r(10)
        calls[f"C ABI, {form}: dpm_tsdf_sample"] = raw_smp
    ms = {k: [] for k in calls}
    for rep in range(a.warmup + a.reps):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                ms[name].append(e0.elapsed_time(e1))
    t = {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ms.items()}
    fmt = lambda v: f"{v[0]:.3f} [{v[1]:.3f}, {v[2]:.3f}]"
    per = lambda a_, b_: (t[b_][0] - t[a_][0]) / 9
    # what the two registrations reach from this start in 10 iterations (reported, not judged)
    res_t, res_l = tsdf_reg(10), lm_reg(10)
    flag = ops.tsdf_sample(*m._map(), frame.xyz, frame.count, init, m.unit)[2]
    has = int((flag == 1).sum().item())

    def err(res):
        p = res[0].cpu().numpy()
        return float(np.linalg.norm(p[:3, 3] - truth[mid][:3, 3])), float(res[1].item())
    path = os.path.join(ROOT, "profiles", "tsdf_register_bench.md")
    with open(path, "w") as f:
        f.write("# Scan-to-TSDF registration at HDL64E size\n\n")
        f.write(f"`python scripts/tsdf_register_bench.py --frames {a.frames}` on {torch.cuda.get_device_name(0)} (torch {torch.__version__}): "
                f"street_scene(2), one whole HDL64E frame ({n_rows} rows in a capacity of {frame.cap}) against the plane-distance map of {F} "
                f"stored frames ({int(lengths.sum().item())} points, {voxels} voxels; voxel {m.voxel_size} m, truncation {m.truncation:g} m, 2^22 "
                f"slots), from a start 0.05 m and 0.2 degrees off.  {has} of the rows have a value under the start pose (all 8 corners).  Every "
                f"call alternated in one process; device time between two events, median [min, max] ms of {a.reps} runs after {a.warmup} "
                "warm-up runs: the [min, max] is the run-to-run spread.  Tolerances 0: no run stops early.  A report, not a threshold.\n\n")
        f.write("| call | ms |\n|---|---|\n")
        for k, v in t.items():
            f.write(f"| {k} | {fmt(v)} |\n")
        f.write(f"\nOne accumulate + solve iteration, (10 iterations - 1 iteration) / 9 of the medians: dpm_tsdf_register "
                f"{per('dpm_tsdf_register, 1 iteration', 'dpm_tsdf_register, 10 iterations'):.3f} ms, dpm_local_map_register_planes "
                f"{per('dpm_local_map_register_planes, 1 iteration', 'dpm_local_map_register_planes, 10 iterations'):.3f} ms (the local "
                "map: voxel 1 m, 3^3 sub-cells, 2^18 slots, the same stored frames, planes computed outside the window).\n\n")
        f.write(f"After 10 iterations from this start: dpm_tsdf_register {err(res_t)[0]:.4f} m from the exact pose with fitness {err(res_t)[1]:.3f}, "
                f"dpm_local_map_register_planes {err(res_l)[0]:.4f} m with fitness {err(res_l)[1]:.3f} (one frame, one start: not an accuracy "
                f"claim; the map's normals are dpm_point_normals within {a.normals_radius:g} m of stored frames thinned to 0.5 m, and the "
                "frame itself is one of the stored ones).\n\n")
        names = list(forms)
        if len(names) == 2:
            torch.cuda.synchronize()
            same = raw_pose[names[0]].cpu().numpy().tobytes() == raw_pose[names[1]].cpu().numpy().tobytes()
            it = {n: per(f"C ABI, {n}: dpm_tsdf_register, 1 iteration", f"C ABI, {n}: dpm_tsdf_register, 10 iterations") for n in names}
            slower = max(names, key=lambda n: it[n])
            spread = max(t[f"C ABI, {n}: dpm_tsdf_register, 10 iterations"][2] - t[f"C ABI, {n}: dpm_tsdf_register, 10 iterations"][1] for n in names) / 9
            f.write(f"Two forms of the field lookup, through the C ABI with outputs made once: one iteration {it[names[0]]:.4f} ms "
                    f"({names[0]}) against {it[names[1]]:.4f} ms ({names[1]}).  The slower is \"{slower}\", by "
                    f"{abs(it[names[0]] - it[names[1]]):.4f} ms an iteration, where the run-to-run spread of the 10-iteration calls is "
                    f"{spread:.4f} ms an iteration.  The 10-iteration poses of the two forms have {'the same' if same else 'DIFFERENT'} "
                    "bytes.  The plain form is the one in the source: a second form is kept only when it is measured faster.\n\n")
        else:
            f.write("The second build of the library was not there: only the shipped form was timed.\n\n")
        f.write(f"dpm_tsdf_sample does the same 8 lookups per row in {t['dpm_tsdf_sample'][0]:.3f} ms, so the lookups are not where an "
                "iteration's time goes.  Supposed, not measured: the one-wave solve launch, which adds the blocks' partials in block "
                "order before the Cholesky step in one lane, and the 29 fp64 butterflies of the accumulate kernel.\n\n")
        f.write("The accumulate kernel is the plain form: one lane per row, 256 rows a block, 8 find_slot probes plus the sum / count loads "
                "per row.  The form with a quad per row was not built.  Not measured: hardware counters, other sensors, other voxel sizes, a table near its capacity.\n")
    print(open(path).read())


if __name__ == "__main__":
    main()
