#!/usr/bin/env python3
"""profiles/sim_slam_eval.md: a whole run in numbers.  Simulates a street scene's circuit (deeppointmap_amd/lidar_sim.py),
writes it as a dataset tree, runs `SlamSystem` over it through `SceneLoader` with `slam_system.result_maps` on, and calls
`ResultLogger.evaluate` with the scene: trajectory errors against the exact poses, the predicted map against the map of the
same clouds under the exact poses, and the predicted map against the scene's analytic surfaces.

A report without an assertion.  The weights are the PROCEDURAL ones (weights.init_procedural: seeded random numbers, no
training) unless --encoder / --decoder name checkpoints, so the numbers say how bad an untrained model is, not how good
the method is; the file says which weights made them.

  python scripts/sim_slam_eval.py [--out profiles/sim_slam_eval.md] [--seed 2] [--frames 40] [--spacing 2.0]
         [--model small16|hdl64e] [--encoder CKPT --decoder CKPT]
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"


class Args:
    transforms = {"VoxelSample": {"voxel_size": 0.3, "retention": "first"}, "ToGPU": {},
                  "DistanceSample": {"min_dis": 1.0, "max_dis": 60.0},
                  "OutlierFilter": {"nb_neighbors": 10, "std_ratio": 3.0},
                  "LowPassFilter": {"normals_radius": 0.5, "normals_num": 16, "filter_std": 2.0, "flux": 4, "max_remain": -1},
                  "CoordinatesNormalization": {"ratio": 60.0}, "ToCPU": {}, "ToTensor": {"padding_to": -1}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim_slam_eval.md"))
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--spacing", type=float, default=2.0)
    ap.add_argument("--model", choices=["hdl64e", "small16"], default="small16")
    ap.add_argument("--encoder", default=None)
    ap.add_argument("--decoder", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("sim_slam_eval.py runs the SLAM chain on a GPU; none is visible")
    torch.set_grad_enabled(False)
    from deeppointmap_amd import augment, dataset, lidar_sim as LS
    from deeppointmap_amd.config import Cfg, default_args
    from deeppointmap_amd.consumer import default_slam_args
    from deeppointmap_amd.decoder import Decoder
    from deeppointmap_amd.encoder import Encoder
    from deeppointmap_amd.loader import SceneLoader
    from deeppointmap_amd.system import SlamSystem
    from deeppointmap_amd.weights import init_procedural

    cfg = default_args()
    enc, dec = Encoder(cfg), Decoder(cfg)
    if a.encoder and a.decoder:
        enc.load_state_dict(torch.load(a.encoder, map_location="cpu"), strict=True)
        dec.load_state_dict(torch.load(a.decoder, map_location="cpu"), strict=True)
        weights = f"checkpoints `{os.path.basename(a.encoder)}` / `{os.path.basename(a.decoder)}`"
    else:
        init_procedural(enc), init_procedural(dec)
        weights = "PROCEDURAL weights (weights.init_procedural: seeded random numbers, never trained)"
    enc, dec = enc.to(DEV), dec.to(DEV)

    model = LS.HDL64E if a.model == "hdl64e" else LS.SMALL16
    scene = LS.street_scene(a.seed, blocks=(2, 2))
    poses = LS.circuit(scene, a.spacing)[:a.frames]
    with tempfile.TemporaryDirectory() as tmp:
        sim = LS.LidarSimulator(scene, model, rng=torch.Generator(device=DEV).manual_seed(a.seed), device=DEV)
        LS.write_scene(tmp, "SimCity", "00", sim, poses, fmt="npz")
        args = Cfg(dict(cfg))
        args.device, args.slam_system = DEV, Cfg(dict(default_slam_args(), result_maps=True))
        system = SlamSystem(args, enc, dec, system_id=0, logger_dir=os.path.join(tmp, "log"))
        agent = dataset.BasicAgent(os.path.join(tmp, "SimCity", "00", "0"), "auto")
        with SceneLoader(agent, augment.PointCloudTransforms(Args, mode="infer"), group=4, prefetch=2, device=DEV) as ld:
            codes = [system.step(list(item)).name for item in ld]
        out = system.result_logger.evaluate("metrics", scene=scene)
    tally = {c: codes.count(c) for c in sorted(set(codes))}
    lines = ["# A simulated run, evaluated", "",
             f"`python scripts/sim_slam_eval.py --seed {a.seed} --frames {a.frames} --spacing {a.spacing} --model {a.model}` on "
             f"{torch.cuda.get_device_name(0)} (torch {torch.__version__}).", "",
             f"**Weights: {weights}.**  A report without an assertion: with procedural weights the numbers below are bad by "
             "construction and say nothing about the method.", "",
             f"Scene: `street_scene({a.seed})`, {scene.P} primitives; {len(poses)} poses {a.spacing} m apart on its circuit, "
             f"{model.rays} rays a scan with range noise; exit codes of `SlamSystem.step`: {tally}; "
             f"{out['scans']} scans in the graph.", "",
             "`ResultLogger.evaluate(scene=scene)` (definitions: `deeppointmap_amd/evaluate.py`; metres, radians, shares):", "",
             "```json", json.dumps(out, indent=1), "```", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
