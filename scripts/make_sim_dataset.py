#!/usr/bin/env python3
"""Write a simulated dataset tree and the config that reads it: street scenes (deeppointmap_amd/lidar_sim.py) ray-cast on the
GPU round their circuits, one scene per seed, with exact poses and exact refined_SE3.pkl tables.

  python scripts/make_sim_dataset.py OUT [--dataset SimCity] [--seeds 0 1] [--blocks 2 2] [--spacing 2.0] [--laps 2]
         [--model hdl64e|small16] [--fmt npz|bin] [--agents 1] [--noise-seed 0 | --clean] [--distance 10.0]

OUT/<dataset>/<seed as two digits>/<agent>/<n>.<fmt>, OUT/<dataset>/<scene>/refined_SE3.pkl, OUT/config.json = the `dataset`
and `train` sections (lidar_sim.tree_config) for dataset.SlamDatasets / loader.EpochLoader / loader.SceneLoader.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--dataset", default="SimCity")
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--blocks", type=int, nargs=2, default=[2, 2])
    ap.add_argument("--spacing", type=float, default=2.0)
    ap.add_argument("--laps", type=int, default=2)
    ap.add_argument("--model", choices=["hdl64e", "small16"], default="hdl64e")
    ap.add_argument("--fmt", choices=["npz", "bin"], default="npz")
    ap.add_argument("--agents", type=int, default=1)
    ap.add_argument("--noise-seed", type=int, default=0)
    ap.add_argument("--clean", action="store_true")
    ap.add_argument("--distance", type=float, default=10.0)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("make_sim_dataset.py ray-casts on a GPU; none is visible")
    from deeppointmap_amd import lidar_sim as LS
    model = LS.HDL64E if a.model == "hdl64e" else LS.SMALL16
    names = []
    for seed in a.seeds:
        scene = LS.street_scene(seed, blocks=tuple(a.blocks))
        poses = LS.circuit(scene, a.spacing, a.laps)
        rng = None if a.clean else torch.Generator(device="cuda").manual_seed(a.noise_seed + seed)
        sim = LS.LidarSimulator(scene, model, rng=rng)
        name = f"{seed:02d}"
        files = LS.write_scene(a.out, a.dataset, name, sim, poses, agents=a.agents, fmt=a.fmt, refined_distance=a.distance)
        names.append(name)
        print(f"{a.dataset}/{name}: {scene.P} primitives, {len(files)} frames of {model.rays} rays", flush=True)
    cfg = LS.tree_config(a.out, {a.dataset: names}, fmt=a.fmt, distance=a.distance)
    with open(os.path.join(a.out, "config.json"), "w") as f:
        json.dump(cfg, f, indent=1)
    print(os.path.join(a.out, "config.json"))


if __name__ == "__main__":
    main()
