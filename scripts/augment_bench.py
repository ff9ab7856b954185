"""The training transforms on the GPU: a batch of 8 and of 16 raw frames of 120 000 points through a representative training
chain,

    GroundFilter -> VoxelSample 'center' -> DistanceSample -> RandomDrop -> RandomShield -> RandomRT -> RandomPosJitter
        -> CoordinatesNormalization -> RandomShuffle -> ToTensor (collate_frames)

in three arms: (a) deeppointmap_amd.augment with a GPU generator (the training mode), (b) the same with rng="reference"
(the reference's draws on the host: one synchronisation per transform whose draw is sized by the point count), (c) the numpy /
torch-CPU restatement (tests/augment_restated.py) replaying arm (b)'s draws, its frames spread over 16 threads.  Per arm: ms per
batch (median [min, max] of --reps after --warmup, a host clock around work that ends in the batch being read back) and the
number of host synchronisations the module issued per batch.  The raw frames are on the GPU (arms a, b) / in host memory (arm c)
before the clock starts.  Reports, not thresholds.  Writes profiles/augment_bench.json and .md.

  python scripts/augment_bench.py [--batches 8,16] [--reps 5] [--warmup 2]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import augment_restated as A
from deeppointmap_amd import augment

SPEC = {"GroundFilter": {"img_len": 400, "img_width": 400, "grid_width": 0.4, "ground_height": 0.3},
        "VoxelSample": {"voxel_size": 0.3, "retention": "center"}, "DistanceSample": {"min_dis": 1.0, "max_dis": 60.0},
        "RandomDrop": {"max_ratio": 0.3, "p": 1.0},
        "RandomShield": {"angle_range": [20.0, 90.0], "dis_range": [5.0, 40.0], "max_num": 4, "p": 1.0},
        "RandomRT": {"r_std": 0.5, "t_std": 1.0, "p": 1.0, "pair": True}, "RandomPosJitter": {"std": 0.02, "p": 1.0},
        "CoordinatesNormalization": {"ratio": 60.0}, "RandomShuffle": {"p": 1.0}}


def raw_frames(n):
    spec = importlib.util.spec_from_file_location("_raw", os.path.join(ROOT, "tests", "golden", "raw_scan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = mod.raw_scan()[:, :3].float()
    out = []
    for k in range(n):                         # the same scene seen under another yaw
        c, s = np.cos(0.37 * k), np.sin(0.37 * k)
        out.append((base @ torch.tensor([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=torch.float32).T).contiguous())
    return out


def timed(fn, reps, warmup):
    ms, syncs = [], None
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        s0, t0 = augment.host_syncs(), time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
            syncs = augment.host_syncs() - s0
    return dict(ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), syncs=syncs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("augment_bench.py measures on a GPU; none is visible")
    torch.set_grad_enabled(False)
    rows = []
    for S in [int(x) for x in a.batches.split(",")]:
        host = raw_frames(S)
        dev = [x.cuda() for x in host]
        gen = torch.Generator(device="cuda")
        gen.manual_seed(1)
        kept = {}

        def gpu(rng, keep=False):
            def run():
                chain = augment.get_transforms(SPEC)
                out = augment.transform_frames([augment.PointCloud(x) for x in dev], chain, rng=rng, return_draws=keep)
                pcds, rec = out if keep else (out, None)   # the draws come back only when asked for
                batch = augment.collate_frames(pcds, -1)
                if keep:
                    kept["records"], kept["shape"] = rec, tuple(batch[0].shape)
            return run
        row = dict(S=S, points=int(host[0].shape[0]), generator=timed(gpu(gen), a.reps, a.warmup),
                   reference=timed(gpu("reference"), a.reps, a.warmup))
        gpu("reference", keep=True)()
        per_frame, cur = [], None
        for name, kw in kept["records"]:
            if name == "frame":
                per_frame.append([])
            else:
                per_frame[-1].append((name, {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}))
        torch.set_num_threads(1)

        def cpu():
            with ThreadPoolExecutor(16) as ex:
                frames = list(ex.map(lambda xr: A.replay(A.Frame(xr[0].numpy()), xr[1]).xyz, zip(host, per_frame)))
            A.pack(frames, -1)
        row["cpu"], row["batch_shape"] = timed(cpu, max(1, a.reps // 2), 1), kept["shape"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    prof = os.path.join(ROOT, "profiles")
    meta = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=a.reps, warmup=a.warmup)
    json.dump(dict(meta=meta, rows=rows), open(os.path.join(prof, "augment_bench.json"), "w"), indent=1)
    cell = lambda d: f"{d['ms']:.1f} [{d['ms_min']:.1f}, {d['ms_max']:.1f}] | {d['syncs']}"   # noqa: E731
    with open(os.path.join(prof, "augment_bench.md"), "w") as f:
        f.write("# Training transforms: a batch of raw frames through a training chain\n\n")
        f.write(f"`python scripts/augment_bench.py` on {meta['device']} (torch {meta['torch']}); median [min, max] ms per batch of "
                f"{a.reps} batches after {a.warmup} warm-up batches, host clock from the raw frames (already on the device / in host "
                "memory) to the packed batch read back; syncs = host synchronisations issued by `deeppointmap_amd.augment` per batch.  "
                "Chain: GroundFilter -> VoxelSample 'center' -> DistanceSample -> RandomDrop -> RandomShield -> RandomRT -> "
                "RandomPosJitter -> CoordinatesNormalization -> RandomShuffle -> ToTensor.  The CPU arm is the numpy / torch restatement "
                "of tests/augment_restated.py on the same draws, frames over 16 threads (it is not the reference's own code, whose "
                "GroundFilter loops over cells in Python).  Reports, not thresholds.\n\n")
        f.write("| frames | raw points | batch | GPU, generator mode ms | syncs | GPU, reference rng ms | syncs | CPU restatement ms | syncs |\n"
                "|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['S']} | {r['points']} | {'x'.join(map(str, r['batch_shape']))} | {cell(r['generator'])} | {cell(r['reference'])} | "
                    f"{cell(r['cpu'])} |\n")


if __name__ == "__main__":
    main()
