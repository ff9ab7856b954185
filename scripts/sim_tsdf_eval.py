#!/usr/bin/env python3
"""profiles/sim_tsdf_eval.md: what fusing a surface gains over keeping points.  A sensor with --sigma metres of range noise
drives one lap of the circuit of street_scene(2); three maps of the same frames are measured against the scene
(evaluate.map_accuracy, total row):

  raw union        every return under its frame's pose;
  voxel centroids  globalmap.voxel_map at --voxel metres;
  TSDF surface     tsdf.TsdfMap at --voxel metres: the zero crossings of the fused field (TsdfMap.surface), for min_count 1 and
                   --min-count.
  TSDF, plane      the same with distance="plane" (the distance to the tangent plane at the return, weighted by the cosine of
                   the incidence), the normals estimated from each frame alone within --normals-radius metres
                   (dpm_point_normals); under the exact poses only.  min_count is in full-weight samples there.
  TSDF, plane + carve   that map after TsdfMap.carve of every frame at --carve-weight full-weight samples.

once under the EXACT poses on the frames as the sensor delivers them, and once the way a run without ground truth ends:
GeometricSlam over the same frames, GeometricSlam.surface_map under its corrected poses, beside the voxel centroids and the raw
union of the same stored (thinned) frames under the same poses.  A report of one run without an assertion: nobody had measured
how much the fused surface gains over the centroids before this run.

  python scripts/sim_tsdf_eval.py [--spacing 2.0] [--beams 32] [--columns 1024] [--sigma 0.02] [--voxel 0.2] [--min-count 3]
                                  [--normals-radius 1.0] [--carve-weight 1.0]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

DEV = "cuda"


def union(clouds, poses):
    """(3,N_i) sensor-frame clouds under (4,4) poses -> (3,N) float32 world, transformed in float64"""
    out = []
    for c, p in zip(clouds, poses):
        P = torch.from_numpy(np.ascontiguousarray(p)).to(c.device)
        out.append((P[:3, :3] @ c.double() + P[:3, 3:4]).float())
    return torch.cat(out, dim=1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spacing", type=float, default=2.0)
    ap.add_argument("--beams", type=int, default=32)
    ap.add_argument("--columns", type=int, default=1024)
    ap.add_argument("--sigma", type=float, default=0.02)
    ap.add_argument("--voxel", type=float, default=0.2)
    ap.add_argument("--min-count", type=int, default=3)
    ap.add_argument("--normals-radius", type=float, default=1.0)
    ap.add_argument("--carve-weight", type=float, default=1.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sim_tsdf_eval.py runs on a GPU; none is visible")
    from deeppointmap_amd import evaluate, globalmap, lidar_sim as LS
    from deeppointmap_amd.loop_closure import GeometricSlam
    from deeppointmap_amd.tsdf import TsdfMap
    scene = LS.street_scene(2)
    model = LS.LidarModel(np.linspace(10.0, -20.0, a.beams), a.columns, 0.9, 80.0, range_sigma=a.sigma)
    truth = LS.circuit(scene, spacing=a.spacing)
    F = len(truth)
    rng = torch.Generator(device=DEV)
    rng.manual_seed(1)
    sim = LS.LidarSimulator(scene, model, rng=rng if a.sigma > 0 else None, device=DEV)
    frames = sim.frames(truth)
    kw = dict(max_voxels=1 << 23, max_range=model.max_range, min_range=0.0)
    rows = []

    def score(group, name, xyz, origin=None):
        r = evaluate.map_accuracy(xyz, scene, origin=origin)["total"]
        rows.append((group, name, xyz.shape[1], r))
        print(group, name, xyz.shape[1], r, flush=True)

    def tsdf_rows(group, m, name="TSDF surface"):
        m.check()
        for mc in sorted({1, a.min_count}):
            s = m.surface(min_count=mc)
            score(group, f"{name}, min_count {mc}", s.xyz, s.origin)

    # -- exact poses, the frames as delivered
    clouds = [f.points().T.contiguous() for f in frames]
    group = "exact poses"
    score(group, "raw union", union(clouds, truth))
    score(group, f"voxel centroids {a.voxel} m", globalmap.voxel_map(clouds, truth, voxel_size=a.voxel)[0])
    m = TsdfMap(a.voxel, **kw)
    for f, p in zip(frames, truth):
        m.integrate(f, p)
    tsdf_rows(group, m)
    held = len(m.export()[0])
    mp = TsdfMap(a.voxel, distance="plane", **kw)
    for f, p in zip(frames, truth):
        mp.integrate(f, p, normals=a.normals_radius)
    plane = f"TSDF, plane distance, normals within {a.normals_radius:g} m"
    tsdf_rows(group, mp, plane)
    returns, unusable = sum(c.shape[1] for c in clouds), mp.unusable()
    for f, p in zip(frames, truth):
        mp.carve(f, p, weight=a.carve_weight)
    tsdf_rows(group, mp, plane + f", carved at weight {a.carve_weight:g}")

    # -- a run without ground truth: the loop closer's stored frames under the corrected poses
    slam = GeometricSlam(odometry=dict(max_range=model.max_range, first_pose=truth[0], initial_motion=LS.sweep_delta(truth[0], truth[1]),
                                       sample_map=0.25, sample_register=0.75, metric="plane", voxel_size=1.0),
                         loop=dict(capacity=F, points_per_frame=model.rays, sc=dict(max_range=model.max_range, z_offset=LS.SENSOR_HEIGHT)))
    for f in frames:
        slam.step(f)
    lc, use = slam.loop_closer, slam.surface_rows()
    stored = [lc.store[r, :, :lc.counts[r]].contiguous() for r in use]
    group = "GeometricSlam, corrected poses, stored frames"
    ate = evaluate.ate(slam.poses, truth)
    score(group, "raw union", union(stored, slam.poses[use]))
    score(group, f"voxel centroids {a.voxel} m", globalmap.voxel_map(stored, slam.poses[use], voxel_size=a.voxel)[0])
    tsdf_rows(group, slam.surface_map(a.voxel, **kw))

    with open(os.path.join(ROOT, "profiles", "sim_tsdf_eval.md"), "w") as f:
        f.write("# A fused TSDF surface against voxel centroids and raw points\n\n")
        f.write(f"`python scripts/sim_tsdf_eval.py --spacing {a.spacing} --beams {a.beams} --columns {a.columns} --sigma {a.sigma} --voxel "
                f"{a.voxel} --min-count {a.min_count} --normals-radius {a.normals_radius:g} --carve-weight {a.carve_weight:g}` on {torch.cuda.get_device_name(0)} (torch {torch.__version__}): street_scene(2), "
                f"{scene.P} primitives, {F} frames {a.spacing} m apart round one lap of the circuit, {a.beams} beams x {a.columns} columns, "
                f"range noise {a.sigma} m.  TsdfMap(voxel_size={a.voxel}): truncation {m.truncation:g} m, step {m.step:g} m; {held} voxels "
                f"held under the exact poses.  GeometricSlam: {len(slam.loops)} accepted loop edges, {F - len(use)} frames left out, ATE rmse "
                f"{ate['rmse']:.3f} m, max {ate['max']:.3f} m; its stored frames are thinned (voxel_sample {lc.sample} m, at most "
                f"{lc.P} points).  Every map against the scene (evaluate.map_accuracy, total row; distances in metres).  A report of one "
                "run, not a target.\n\n")
        thr = list(rows[0][3]["within"])
        f.write("| poses and frames | map | map points | mean | rmse | max | " + " | ".join(f"within {t} m" for t in thr) + " |\n")
        f.write("|---|---|---|---|---|---|" + "---|" * len(thr) + "\n")
        for group, name, M, r in rows:
            f.write(f"| {group} | {name} | {M} | {r['mean']:.5f} | {r['rmse']:.5f} | {r['max']:.4f} | "
                    + " | ".join(f"{100 * r['within'][t]:.2f} %" for t in thr) + " |\n")
        f.write(f"\nPlane distance: {unusable} of the {returns} returns had no usable normal (no neighbours within the radius, or 256 "
                "|cos incidence| < 0.5) and were left out; min_count counts full-weight samples (256 count units).  The carve ran after "
                f"all integrations, margin {mp.truncation + mp.voxel_size:g} m.  The row with the simulator's true normals was not run: the "
                "cast reports the primitive and the cosine of the incidence of a ray, not the face it met, so the normal is not to be "
                "had from the hit ids without restating the primitives' geometry.\n")
        f.write("\nWhat the table does not say: completeness (how much of the scene each map covers) was not measured, and a surface "
                "point exists only between two voxels that both hold samples.\n")
    print(open(os.path.join(ROOT, "profiles", "sim_tsdf_eval.md")).read())


if __name__ == "__main__":
    main()
