#!/usr/bin/env python3
"""profiles/loader_bench.md: what the batch loader costs on one MI355X, on a synthetic tree (deeppointmap_amd/synthetic.py
scans, 12 frames of 120 000 points per registration batch, `.bin` and `.npz`).  A report of one run, not a target.

(a) staging + ingest per batch (ops.ingest_stage into a pinned slot + ops.ingest_frames, files already read) next to the
    path without them: one PointCloud(filtered array) per frame from pageable memory;
(b) milliseconds the training thread waits for a batch per step, and the step time, at prefetch 0 / 1 / 2 with the reduced
    model's registration step;
(c) launches per batch of the ingest.
Warm-up iterations are dropped; every figure is a median with the 10th / 90th percentile of the kept iterations.

python scripts/loader_bench.py [--out profiles/loader_bench.md] [--points 120000] [--reps 30]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from deeppointmap_amd import augment, dataset, ops, synthetic  # noqa: E402
from deeppointmap_amd.config import reduced_args  # noqa: E402

DEV = "cuda:0"
FRAMES = 24
LOSS = dict(tau=0.1, offset_value="manhattan", eps_positive=1.0, eps_offset=2.0, lambda_p=1.0, lambda_c=1.0, lambda_o=1.0)
CHAIN = {"VoxelSample": {"voxel_size": 1.0, "retention": "first"}, "DistanceSample": {"min_dis": 1.0, "max_dis": 60.0},
         "RandomRT": {}, "RandomDrop": {"max_ratio": 0.2}, "CoordinatesNormalization": {"ratio": 60.0}}


def write_tree(root, kind, points):
    """one dataset, one scene, one agent, FRAMES frames half a metre apart; .bin frames carry an intensity column and a few
    NaN records; frame_dis.npy is written beside them (the reference builds it from .npz files only)"""
    base = synthetic.base_cloud(points)
    d = os.path.join(root, "Synth", "00", "0")
    os.makedirs(d)
    T = []
    for f in range(FRAMES):
        xyz = (synthetic.frame(f, points, base).t() * synthetic.COOR_SCALE).contiguous().numpy()
        P = synthetic.sensor_pose(f).numpy()
        T.append(P[:3, 3].astype(np.float32))
        if kind == "npz":
            np.savez(os.path.join(d, f"{f}.npz"), lidar_pcd=xyz, ego_rotation=P[:3, :3].astype(np.float32),
                     ego_translation=P[:3, 3:].astype(np.float32))
        else:
            rec = np.concatenate([xyz, np.full((points, 1), 0.5, np.float32)], axis=1)
            rec[::997, f % 3] = np.nan
            rec.tofile(os.path.join(d, f"{f}.bin"))
    np.save(os.path.join(root, "Synth", "00", "frame_dis.npy"), dataset.pairwise_frame_dis(np.stack(T)))
    cfg = reduced_args()
    cfg.loss = dict(LOSS)
    cfg.dataset = [{"name": "Carla_Synth", "root": os.path.join(root, "Synth"), "scenes": ["00"], "reader": {"type": kind}}]
    cfg.train = dict(registration=dict(K=6, K_max=12, fill=True, distance=10.0, map_size_max=4, batch_size=1,
                                       optimizer=dict(type="AdamW", kwargs=dict(lr=1e-4)), scheduler=dict(type="identity", kwargs={})),
                     loop_detection=dict(distance=6.0))
    return cfg


def spread(ms):
    ms = np.asarray(ms)
    return f"{np.median(ms):.3f} ({np.percentile(ms, 10):.3f} .. {np.percentile(ms, 90):.3f})"


def timed(fn, reps, warm=5):
    out = []
    for k in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warm:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def bench_ingest(ds, points, reps):
    scene = ds.dataset_list[0].scene_list[0]
    raws = [scene.read_raw(f) for f in range(12)]
    cap = points
    slot = torch.empty(ops.ingest_layout([r[0].shape for r in raws])[1], dtype=torch.uint8, pin_memory=True)

    def new():
        block = ops.ingest_stage([(r[0], r[4]) for r in raws], block=slot)
        return ops.ingest_frames(block, len(raws), cap, device=DEV)

    def stage_only():
        ops.ingest_stage([(r[0], r[4]) for r in raws], block=slot)

    def old():
        return [augment.PointCloud(dataset.filter_rows(r[0], r[4])[:, :3], rotation=r[2], translation=r[3]) for r in raws]
    return timed(new, reps), timed(stage_only, reps), timed(old, reps)


def bench_steps(cfg, ds, prefetch, points):
    import encoder_train_cases as EC
    from deeppointmap_amd.decoder import Decoder
    from deeppointmap_amd.encoder import Encoder
    from deeppointmap_amd.loader import EpochLoader
    from deeppointmap_amd.loss import RegistrationLoss
    from deeppointmap_amd.train_pipeline import DeepPointModelPipeline, TrainStep
    from deeppointmap_amd.weights import init_procedural
    enc = Encoder(cfg)
    enc.load_state_dict(EC.state_dict(cfg), strict=True)
    dec = init_procedural(Decoder(cfg))
    model = DeepPointModelPipeline(cfg, enc.to(DEV).set_train_dense("hip"), dec.to(DEV).set_train_dense("hip"), RegistrationLoss(cfg))
    step = TrainStep(cfg, model)
    waits, steps = [], []
    with EpochLoader(ds, augment.get_transforms(CHAIN), "registration", 1, rng=3, prefetch=prefetch, capacity=points,
                     padding_to=-1, num_workers=4, device=DEV) as ld:
        for ep in (1, 2):
            ld.set_epoch(ep)
            it = iter(ld)
            for k in range(len(ld)):
                t0 = time.perf_counter()
                batch = next(it)
                t1 = time.perf_counter()
                step.step(*batch)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if ep > 1 or k >= 6:           # the first steps warm the allocator and the kernels up
                    waits.append((t1 - t0) * 1e3), steps.append((t2 - t1) * 1e3)
    return waits, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loader_bench.md"))
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    lines = ["# Loader bench", "",
             f"One run on {torch.cuda.get_device_name(0)}; synthetic tree, {FRAMES} frames of {a.points} points, 12 frames per "
             "registration batch.  Milliseconds: median (10th .. 90th percentile).  A report, not a target.", "",
             "## (a) staging + ingest per batch of 12 frames (files already read)", "",
             "| files | ingest_stage + ingest_frames | of which ingest_stage (host copy into the pinned slot) | one PointCloud(array) per frame, pageable |",
             "|---|---|---|---|"]
    steps = []
    with tempfile.TemporaryDirectory() as tmp:
        for kind in ("bin", "npz"):
            cfg = write_tree(os.path.join(tmp, kind), kind, a.points)
            ds = dataset.SlamDatasets(cfg)
            new, stage, old = bench_ingest(ds, a.points, a.reps)
            lines.append(f"| .{kind} | {spread(new)} | {spread(stage)} | {spread(old)} |")
            if kind == "npz":
                for prefetch in (0, 1, 2):
                    w, s = bench_steps(cfg, ds, prefetch, a.points)
                    steps.append(f"| {prefetch} | {spread(w)} | {spread(s)} | {len(w)} |")
    lines += ["", "## (b) the reduced model's registration step, .npz files, 4 reader threads", "",
              "| prefetch | wait for the batch per step | step (forward, backward, optimiser; synchronised) | steps |", "|---|---|---|---|", *steps, "",
              "## (c) launches per batch", "",
              "`dpm_ingest_frames`: 1 asynchronous copy + 3 kernel launches per batch, whatever the number of frames (fixed in "
              "`csrc/ingest.hip`).  `PointCloud(array)` per frame: 1 pageable copy + 4 torch launches (zeros, slice assignment, arange, "
              "full), 12 copies + 48 launches for this batch.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
