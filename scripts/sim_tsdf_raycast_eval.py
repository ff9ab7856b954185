#!/usr/bin/env python3
"""profiles/sim_tsdf_raycast_eval.md: what a ray-cast of the fused map sees, against what the simulator sees in the scene itself.
A sensor drives one lap of the circuit of street_scene(2); every second pose of the circuit (--spacing metres apart) is fused
under its exact pose, once with distance="ray" and once with distance="plane" (normals estimated from each frame alone within
--normals-radius metres); the map is then ray-cast (TsdfMap.raycast) from --held of the poses in between, which fused nothing,
and the same rays are cast against the scene (lidar_sim.cast_rays) from the same poses.  Reported: the HIT / MISS / BACK table
against the simulator's hit / no hit, and the range error over the rays both call a hit (mean, rmse, worst, and the share within
one voxel).  A report of one run without an assertion.

--accuracy: only turn test_logs/tsdf_raycast.log, which the tests write, into profiles/tsdf_raycast_accuracy.md.

  python scripts/sim_tsdf_raycast_eval.py [--spacing 1.0] [--beams 32] [--columns 1024] [--sigma 0.02] [--voxel 0.2] [--min-count 1]
                                          [--normals-radius 1.0] [--held 16] [--accuracy]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

DEV = "cuda"


def accuracy():
    src = os.path.join(ROOT, "test_logs", "tsdf_raycast.log")
    lines = [l.rstrip("\n") for l in open(src)]
    seen, keep = set(), []
    for l in lines:                       # a test that ran twice logged twice
        if l not in seen:
            seen.add(l)
            keep.append(l)
    with open(os.path.join(ROOT, "profiles", "tsdf_raycast_accuracy.md"), "w") as f:
        f.write("# Ray-casting the TSDF map: observed errors\n\n")
        f.write("Every comparison tests/test_tsdf_raycast_host.py made on the CPU (`host`) and tests/test_gpu_tsdf_raycast.py made on the "
                "GPU (`gpu`), as they logged it; the bounds are derived in those files.  The float32 and float64 forms are the numpy "
                "restatement (tests/tsdf_raycast_restated.py).  The reference has no TSDF: there is nothing else to compare with.\n\n```\n")
        f.write("\n".join(keep) + "\n```\n")
    print(f"wrote profiles/tsdf_raycast_accuracy.md ({len(keep)} lines)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spacing", type=float, default=1.0)
    ap.add_argument("--beams", type=int, default=32)
    ap.add_argument("--columns", type=int, default=1024)
    ap.add_argument("--sigma", type=float, default=0.02)
    ap.add_argument("--voxel", type=float, default=0.2)
    ap.add_argument("--min-count", type=float, default=1)
    ap.add_argument("--normals-radius", type=float, default=1.0)
    ap.add_argument("--held", type=int, default=16)
    ap.add_argument("--accuracy", action="store_true")
    a = ap.parse_args()
    if a.accuracy:
        return accuracy()
    import torch
    if not torch.cuda.is_available():
        sys.exit("sim_tsdf_raycast_eval.py runs on a GPU; none is visible")
    from deeppointmap_amd import lidar_sim as LS
    from deeppointmap_amd.tsdf import BACK, HIT, MISS, TsdfMap
    scene = LS.street_scene(2)
    model = LS.LidarModel(np.linspace(10.0, -20.0, a.beams), a.columns, 0.9, 80.0, range_sigma=a.sigma)
    circuit = LS.circuit(scene, spacing=a.spacing)
    fused = circuit[0::2]
    between = circuit[1::2]
    held = between[np.linspace(0, len(between) - 1, min(a.held, len(between))).astype(int)]
    rng = torch.Generator(device=DEV)
    rng.manual_seed(1)
    sim = LS.LidarSimulator(scene, model, rng=rng if a.sigma > 0 else None, device=DEV)
    frames = sim.frames(fused)
    exact = LS.cast_rays(scene.to_device(DEV), held, model)
    exact.check()
    truth_rng, truth_hit = exact[0], exact[1] >= 0
    kw = dict(max_voxels=1 << 23, max_range=model.max_range, min_range=0.0, device=DEV)
    rows = []
    for distance in ("ray", "plane"):
        m = TsdfMap(a.voxel, distance=distance, **kw)
        for f, p in zip(frames, fused):
            m.integrate(f, p, normals=a.normals_radius if distance == "plane" else None)
        m.check()
        cast = m.raycast(held, model, min_count=a.min_count)
        m.check()
        plain = m.raycast(held, model, min_count=a.min_count, skip=False)
        same = all(bool((x == y).all()) for x, y in zip(cast, plain))
        table = {(name, hit): int(((cast.flag == code) & (truth_hit == hit)).sum()) for name, code in (("HIT", HIT), ("MISS", MISS), ("BACK", BACK))
                 for hit in (True, False)}
        both = (cast.flag == HIT) & truth_hit
        err = (cast.range - truth_rng)[both].double()
        rows.append(dict(distance=distance, voxels=len(m.export()[0]), table=table, n=int(both.sum()), mean=float(err.abs().mean()),
                         bias=float(err.mean()), rmse=float(err.pow(2).mean().sqrt()), worst=float(err.abs().max()),
                         within=float((err.abs() <= a.voxel).double().mean()), same=same))
        print(rows[-1], flush=True)
    path = os.path.join(ROOT, "profiles", "sim_tsdf_raycast_eval.md")
    with open(path, "w") as f:
        f.write("# A ray-cast of the fused TSDF map against the simulator's cast of the scene\n\n")
        f.write(f"`python scripts/sim_tsdf_raycast_eval.py --spacing {a.spacing} --beams {a.beams} --columns {a.columns} --sigma {a.sigma} --voxel "
                f"{a.voxel} --min-count {a.min_count:g} --normals-radius {a.normals_radius:g} --held {a.held}` on {torch.cuda.get_device_name(0)} "
                f"(torch {torch.__version__}): street_scene(2), {scene.P} primitives; {len(fused)} frames {2 * a.spacing:g} m apart round one lap "
                f"of the circuit, {a.beams} beams x {a.columns} columns, range noise {a.sigma} m, fused under their exact poses; "
                f"TsdfMap(voxel_size={a.voxel}): truncation {3 * a.voxel:g} m, step {a.voxel / 2:g} m.  {len(held)} held-out poses half way "
                f"between fused ones, {model.rays} rays each from {model.min_range} to {model.max_range:g} m, cast into the map "
                "(TsdfMap.raycast) and into the scene (lidar_sim.cast_rays, without noise).  A report of one run, not a target.\n\n")
        f.write("| map | voxels | block form = plain form | HIT where the scene is hit | MISS where hit | BACK where hit | HIT where the scene is "
                "not hit | MISS where not | BACK where not |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            t = r["table"]
            f.write(f"| distance=\"{r['distance']}\" | {r['voxels']} | {'the same bytes' if r['same'] else 'DIFFERENT'} | {t[('HIT', True)]} | "
                    f"{t[('MISS', True)]} | {t[('BACK', True)]} | {t[('HIT', False)]} | {t[('MISS', False)]} | {t[('BACK', False)]} |\n")
        f.write("\nRange of the map's HIT minus the scene's range, over the rays both call a hit (metres):\n\n")
        f.write(f"| map | rays | mean of the error | mean of its magnitude | rmse | worst | within one voxel ({a.voxel} m) |\n|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| distance=\"{r['distance']}\" | {r['n']} | {r['bias']:+.4f} | {r['mean']:.4f} | {r['rmse']:.4f} | {r['worst']:.3f} | "
                    f"{100 * r['within']:.2f} % |\n")
        f.write("\nWhat the tables do not say: a MISS where the scene is hit is mostly a surface no fused frame saw, or saw too sparsely for "
                "two samples in a row to have all 8 corners; a large worst error is a ray that passes an edge the map holds and the scene's "
                "ray just misses, or the reverse.  Neither was counted apart.\n")
    print(open(path).read())


if __name__ == "__main__":
    main()
