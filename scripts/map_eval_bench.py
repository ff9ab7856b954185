#!/usr/bin/env python3
"""profiles/map_eval_bench.md: what the map-evaluation kernels (csrc/map_eval.hip) cost at sizes a user would run, on one
MI355X: about 10^6 map points against a 2 x 2-block street scene (dpm_scene_distance), cloud to cloud at about 10^6 <-> 10^6
(dpm_cloud_nn, both directions of map_to_map) and the statistics table of 10^6 distances (dpm_distance_stats).  Device time
between two events, median [min, max] of --reps runs after --warmup, the profiler off.  Rates are computed from SHAPES by
the code below (evaluations = primitives x points, or query x target pairs an exhaustive search would visit; bytes = what
the call must read and write once), next to a chunked dense torch formulation of the same quantities on the same GPU (the
neighbour search on --dense-queries queries, scaled).  A report of one run, not a target; nothing depends on its numbers.

  python scripts/map_eval_bench.py [--out profiles/map_eval_bench.md] [--poses 12] [--reps 10] [--warmup 3] [--dense-queries 16384]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

DEV = "cuda:0"
THR = (0.05, 0.1, 0.2, 0.5)
MAX_DIST = 1.0


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


def world_cloud(frames, poses):
    """the frames' returns in the world: moved in float64 on the device, rounded to float32, (3,M)"""
    parts = []
    for pcd, M in zip(frames, poses):
        n = pcd.nbr_point
        R, t = torch.from_numpy(M[:3, :3]).to(DEV), torch.from_numpy(M[:3, 3]).to(DEV)
        parts.append((pcd.xyz[:n].double() @ R.T + t).float().T)
    return torch.cat(parts, dim=1).contiguous()


def torch_scene_distance(q, rec, ground, chunk=1 << 16):
    """the same quantities as dpm_scene_distance on shifted points q (3,M), dense over (chunk, P)"""
    box = rec[:, 8].view(torch.int32) == 0
    out_d, out_s = [], []
    for a in range(0, q.shape[1], chunk):
        p = q[:, a:a + chunk]
        dx, dy, dz = (p[k][:, None] - rec[None, :, k] for k in range(3))
        lx, ly = rec[:, 3] * dx + rec[:, 4] * dy, rec[:, 3] * dy - rec[:, 4] * dx
        ax, ay, az = lx.abs() - rec[:, 5], ly.abs() - rec[:, 6], dz.abs() - rec[:, 7]
        d_box = (torch.sqrt(ax.clamp(min=0) ** 2 + ay.clamp(min=0) ** 2 + az.clamp(min=0) ** 2) + torch.maximum(ax, torch.maximum(ay, az)).clamp(max=0)).abs()
        a0, a1 = torch.sqrt(dx * dx + dy * dy) - rec[:, 5], dz.abs() - rec[:, 6]
        d_cyl = (torch.sqrt(a0.clamp(min=0) ** 2 + a1.clamp(min=0) ** 2) + torch.maximum(a0, a1).clamp(max=0)).abs()
        d = torch.cat([torch.where(box, d_box, d_cyl), (p[2] - ground).abs()[:, None]], dim=1)
        m = d.min(dim=1)
        out_d.append(m.values), out_s.append(m.indices.int())
    return torch.cat(out_d), torch.cat(out_s)


def torch_nn(q, t, max_dist, chunk=512):
    """exhaustive nearest neighbour within max_dist, dense over (chunk, Nt)"""
    out = []
    for a in range(0, q.shape[1], chunk):
        p = q[:, a:a + chunk]
        d2 = (p[0][:, None] - t[0]) ** 2 + (p[1][:, None] - t[1]) ** 2 + (p[2][:, None] - t[2]) ** 2
        m = d2.min(dim=1).values
        out.append(torch.where(m <= max_dist * max_dist, m.sqrt(), torch.full_like(m, float("inf"))))
    return torch.cat(out)


def torch_stats(d, surf, class_id, C, thr, max_dist):
    cls = class_id[surf.long().clamp(min=0)]
    ok = torch.isfinite(d) & (d <= max_dist)
    dd = d.double()
    rows = []
    for c in range(C + 1):
        sel = ok if c == C else ok & (cls == c)
        rest = ~ok if c == C else ~ok & (cls == c)
        v = torch.where(sel, dd, torch.zeros_like(dd))
        rows.append(torch.stack([sel.sum().double(), rest.sum().double(), v.sum(), (v * v).sum(), v.max()] +
                                [(sel & (d <= t)).sum().double() for t in thr]))
    return torch.stack(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_eval_bench.md"))
    ap.add_argument("--poses", type=int, default=12)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dense-queries", type=int, default=16384)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("map_eval_bench.py measures on a GPU; none is visible")
    torch.set_grad_enabled(False)
    from deeppointmap_amd import evaluate as ev, lidar_sim as LS, ops
    scene = LS.street_scene(0, blocks=(2, 2))
    allp = LS.circuit(scene, 2.0)
    poses = allp[np.linspace(0, len(allp) - 1, a.poses).astype(int)]
    shifted = poses.copy()
    shifted[1::2, 0, 3] += 0.3
    sim = LS.LidarSimulator(scene, LS.HDL64E, rng=torch.Generator(device=DEV).manual_seed(0), device=DEV)
    frames = sim.frames(poses)
    ref, est = world_cloud(frames, poses), world_cloud(frames, shifted)
    M, P = ref.shape[1], scene.P
    origin = ev.bounding_box_centre(ref, est)
    rec = torch.from_numpy(ev.scene_records(scene, origin)).to(DEV)
    ground = scene.z0 - origin[2]
    class_id = torch.from_numpy(np.concatenate([scene.class_id, [LS.GROUND]]).astype(np.int32)).to(DEV)
    C = int(class_id.max()) + 1
    shift = lambda c: (c.double() - torch.tensor(origin, device=DEV, dtype=torch.float64)[:, None]).float()
    q_ref, q_est = shift(ref), shift(est)

    dist, surf = ops.scene_distance(est, rec, ground, origin)
    rows = []
    t_k = timed(lambda: ops.scene_distance(est, rec, ground, origin), a.reps, a.warmup)
    t_t = timed(lambda: torch_scene_distance(q_est, rec, float(np.float32(ground))), max(a.reps // 3, 2), 1)
    td, ts = torch_scene_distance(q_est, rec, float(np.float32(ground)))
    agree = f"max |d - d_torch| {float((dist - td).abs().max()):.2e} m, {int((surf != ts).sum())} of {M} ids differ"
    ev_n, by = (P + 1) * M, M * 20 + P * 48
    rows.append(("dpm_scene_distance", f"{M} points x {P} primitives + ground", t_k, ev_n, by, t_t, 1.0, agree))

    d_acc, _ = ops.cloud_nn(est, ref, MAX_DIST, origin)
    t_k = timed(lambda: ops.cloud_nn(est, ref, MAX_DIST, origin), a.reps, a.warmup)
    nd = min(a.dense_queries, M)
    t_t = timed(lambda: torch_nn(q_est[:, :nd], q_ref, MAX_DIST), 2, 1)
    tn = torch_nn(q_est[:, :nd], q_ref, MAX_DIST)
    both = torch.isfinite(tn) & torch.isfinite(d_acc[:nd])
    agree = (f"on the first {nd} queries: {int((torch.isfinite(tn) != torch.isfinite(d_acc[:nd])).sum())} differ in matched / unmatched, "
             f"max |d - d_torch| {float((tn - d_acc[:nd])[both].abs().max()):.2e} m")
    rows.append(("dpm_cloud_nn (one direction)", f"{M} queries x {M} targets, max_dist {MAX_DIST} m", t_k, M * M, M * 12 * 2 + M * 8 + M * 32,
                 t_t, M / nd, agree))

    tab = ops.distance_stats(dist, list(THR), MAX_DIST, surf=surf, class_id=class_id, n_classes=C)
    t_k = timed(lambda: ops.distance_stats(dist, list(THR), MAX_DIST, surf=surf, class_id=class_id, n_classes=C), a.reps, a.warmup)
    t_t = timed(lambda: torch_stats(dist, surf, class_id, C, THR, MAX_DIST), a.reps, a.warmup)
    tt = torch_stats(dist, surf, class_id, C, THR, MAX_DIST)
    agree = f"max relative difference of the tables {float(((tab - tt).abs() / tt.abs().clamp(min=1e-300)).max()):.2e}"
    rows.append(("dpm_distance_stats", f"{M} distances, {C} classes, {len(THR)} thresholds", t_k, M * (C + 1), M * 8 * (C + 1), t_t, 1.0, agree))

    lines = ["# Map evaluation: time per call", "",
             f"`python scripts/map_eval_bench.py --poses {a.poses}` on {torch.cuda.get_device_name(0)} (torch {torch.__version__}): "
             f"`street_scene(0)` of {P} primitives, {a.poses} HDL64E scans with range noise = {M} map points; the estimated map has every "
             "second scan 0.3 m off.  Device time between two events, median [min, max] ms of "
             f"{a.reps} runs after {a.warmup} warm-up runs, the profiler off.  Evaluations and bytes are computed from shapes "
             "(for the neighbour search: the pairs an exhaustive search would visit, which the grid does not visit).  "
             "A report, not a target.", "",
             "| call | shapes | ms | evaluations/s | bytes/s | dense torch, ms (scaled to the same shapes) | agreement |",
             "|---|---|---|---|---|---|---|"]
    for name, shapes, (med, lo, hi), n_ev, n_by, (tm, tlo, thi), scale, agree in rows:
        lines.append(f"| {name} | {shapes} | {med:.3f} [{lo:.3f}, {hi:.3f}] | {n_ev / med * 1e3:.3e} | {n_by / med * 1e3:.3e} | "
                     f"{tm * scale:.1f} [{tlo * scale:.1f}, {thi * scale:.1f}] | {agree} |")
    m2m = ev.map_to_map(est, ref, THR, MAX_DIST, origin=origin)
    lines += ["", f"The dense neighbour search ran on {nd} queries and is scaled by {M / nd:.1f}.  The torch formulations fuse and "
              "reorder arithmetic as torch likes; they are the same quantities, not the same bits.", "",
              f"`map_to_map` of the two clouds: precision {m2m['precision']['0.1']:.4f}, recall {m2m['recall']['0.1']:.4f} at 0.1 m, "
              f"chamfer {m2m['chamfer']:.4f} m.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
