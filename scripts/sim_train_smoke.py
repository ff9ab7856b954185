#!/usr/bin/env python3
"""profiles/sim_train_smoke.md: the existing Trainer run for a few dozen registration steps on a SIMULATED tree (a street scene
ray-cast with the small 16-beam model, written by lidar_sim.write_scene with its exact refined_SE3.pkl), reduced model.  It
records the loss of the first and of the last ten steps.  A report only: nothing is asserted and nothing is claimed to
converge -- it shows that simulated scans pass through the reader, the loader, the transforms and the training step.

  python scripts/sim_train_smoke.py [--steps 40] [--out profiles/sim_train_smoke.md]
"""
import argparse
import os
import sys
import tempfile
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch

DEV = "cuda:0"
LOSS = dict(tau=0.1, offset_value="manhattan", eps_positive=1.0, eps_offset=2.0, lambda_p=1.0, lambda_c=1.0, lambda_o=1.0)
CHAIN = {"VoxelSample": {"voxel_size": 0.3, "retention": "first"}, "DistanceSample": {"min_dis": 1.0, "max_dis": 60.0},
         "RandomRT": {}, "RandomDrop": {"max_ratio": 0.2}, "CoordinatesNormalization": {"ratio": 60.0},
         "ToTensor": {"padding_to": 8192, "use_calib": True}}
BATCH = 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim_train_smoke.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sim_train_smoke.py trains on a GPU; none is visible")
    import encoder_train_cases as EC
    from deeppointmap_amd import augment, dataset, lidar_sim as LS
    from deeppointmap_amd.config import reduced_args
    from deeppointmap_amd.decoder import Decoder
    from deeppointmap_amd.encoder import Encoder
    from deeppointmap_amd.loss import RegistrationLoss
    from deeppointmap_amd.train_pipeline import DeepPointModelPipeline
    from deeppointmap_amd.trainer import Trainer
    from deeppointmap_amd.weights import init_procedural
    work = tempfile.mkdtemp(prefix="sim_train_")
    scene = LS.street_scene(0, blocks=(1, 1))
    poses = LS.circuit(scene, 2.0, laps=1)
    sim = LS.LidarSimulator(scene, LS.SMALL16, rng=torch.Generator(device=DEV).manual_seed(0), device=DEV)
    files = LS.write_scene(work, "SimCity", "00", sim, poses, refined_distance=10.0)
    tree = LS.tree_config(work, {"SimCity": ["00"]}, distance=10.0)
    per_epoch = max(len(files) // BATCH, 1)
    epochs = -(-a.steps // per_epoch)
    cfg = reduced_args()
    cfg.loss, cfg.dataset, cfg.transforms = dict(LOSS), tree["dataset"], dict(CHAIN)
    cfg.train = dict(auto_cast=False, log_cycle=BATCH, save_cycle=10 ** 6,
                     registration=dict(tree["train"]["registration"], num_epochs=epochs, batch_size=BATCH,
                                       optimizer=dict(type="AdamW", kwargs=dict(lr=1e-4, weight_decay=1e-2)),
                                       scheduler=dict(type="identity", kwargs={})),
                     loop_detection=dict(tree["train"]["loop_detection"], num_epochs=0, batch_size=BATCH,
                                         optimizer=dict(type="sgd", kwargs=dict(lr=1e-3, momentum=0.9)),
                                         scheduler=dict(type="identity", kwargs={})))
    cfg.loader = dict(rng=7, prefetch=2, capacity=LS.SMALL16.rays, padding_to=8192)
    for k, v in dict(name="SimSmoke", version="V0", yaml_file="configs/sim_smoke.yaml", use_ddp=False, local_rank=0, checkpoint="",
                     weight="", device=DEV, num_workers=2).items():
        cfg[k] = v
    enc = Encoder(cfg)
    enc.load_state_dict(EC.state_dict(cfg), strict=True)
    dec = init_procedural(Decoder(cfg))
    model = DeepPointModelPipeline(cfg, enc.to(DEV).set_train_dense("hip"), dec.to(DEV).set_train_dense("hip"), RegistrationLoss(cfg))
    ds = dataset.SlamDatasets(cfg, data_transforms=augment.PointCloudTransforms(cfg, mode="train"))
    values = []
    writer = SimpleNamespace(add_scalar=lambda tag, value, step: values.append((tag, float(value), int(step))))
    cwd = os.getcwd()
    os.chdir(work)
    try:
        Trainer(cfg, ds, model, writer=writer).run()
    finally:
        os.chdir(cwd)
    tags = sorted({t for t, _, _ in values if t.startswith("train/step_")})
    with open(a.out, "w") as f:
        f.write("# Trainer on a simulated tree: a smoke run\n\n")
        f.write(f"`python scripts/sim_train_smoke.py --steps {a.steps}` on {torch.cuda.get_device_name(0)} (torch {torch.__version__}): "
                f"street_scene(0, blocks=(1, 1)), {len(files)} frames 2 m apart round its circuit, SMALL16 ({LS.SMALL16.rays} rays) with "
                f"2 cm range noise, exact refined_SE3.pkl; reduced model from procedural weights, AdamW lr 1e-4, {epochs} epochs of "
                f"{per_epoch} steps, batches of {BATCH} frames.  A report only: no assertion, and no claim that anything converges.\n\n"
                "| metric | first ten steps | last ten steps |\n|---|---|---|\n")
        for tag in tags:
            series = [v for t, v, _ in values if t == tag]
            cell = lambda xs: " ".join(f"{x:.4f}" for x in xs)
            f.write(f"| {tag[len('train/step_'):]} | {cell(series[:10])} | {cell(series[-10:])} |\n")
        f.write(f"\n{len([1 for t, _, _ in values if t == tags[0]]) if tags else 0} steps were logged.\n")
    print(open(a.out).read())


if __name__ == "__main__":
    main()
