#!/usr/bin/env python3
"""profiles/scene_loader_bench.md: the shipped inference chain with the frame's length on the host and in device memory, and
the scene loader's read-ahead, on one MI355X.  A report of one run, not a target; nothing depends on its numbers.

64 frames of raw_scan(120000, seed) written as `.bin`.
(a) per-frame time of the full chain through preprocess_scan(outlier=, lowpass=) -- the synchronous path -- and through the
    device-count path (the class-layer chain + collate_frames), the two sides alternating frame by frame;
(b) host synchronisations per frame on both paths (augment.host_syncs() for the device-count path; the synchronous path's
    are counted from its code: preprocess_scan's status, then one survivor count per filter);
(c) milliseconds the consumer waits for a frame with prefetch 0 / 1 / 2 while a stand-in consumer runs Encoder.forward on it.
Warm-up iterations are dropped; every figure is a median with the 10th / 90th percentile of the kept iterations.

python scripts/scene_loader_bench.py [--out profiles/scene_loader_bench.md] [--frames 64] [--points 120000]
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

from raw_scan import raw_scan  # noqa: E402

from deeppointmap_amd import augment, dataset  # noqa: E402
from deeppointmap_amd.config import default_args  # noqa: E402
from deeppointmap_amd.preprocess import preprocess_scan  # noqa: E402

DEV = "cuda:0"
OUTLIER, LOWPASS = (10, 3.0), (0.5, 16, 2.0, 4)
SYNC_PATH_SYNCS = 3      # preprocess_scan: the status read-back, then _stat_filter's survivor count once per filter


class Args:
    transforms = {"VoxelSample": {"voxel_size": 0.3, "retention": "first"}, "ToGPU": {},
                  "DistanceSample": {"min_dis": 1.0, "max_dis": 60.0},
                  "OutlierFilter": {"nb_neighbors": OUTLIER[0], "std_ratio": OUTLIER[1]},
                  "LowPassFilter": {"normals_radius": LOWPASS[0], "normals_num": LOWPASS[1], "filter_std": LOWPASS[2],
                                    "flux": LOWPASS[3], "max_remain": -1},
                  "CoordinatesNormalization": {"ratio": 60.0}, "ToCPU": {}, "ToTensor": {"padding_to": -1}}


def spread(ms):
    ms = np.asarray(ms)
    return f"{np.median(ms):.3f} ({np.percentile(ms, 10):.3f} .. {np.percentile(ms, 90):.3f})"


def write_scene(d, frames, points):
    scans = []
    for k in range(frames):
        xyz = raw_scan(points, 100 + k)
        scans.append(xyz)
        torch.cat([xyz, torch.full((points, 1), 0.5)], dim=1).numpy().astype(np.float32).tofile(os.path.join(d, f"{k}.bin"))
    return scans


def bench_chain(scans, warm=4):
    chain = augment.get_transforms({k: v for k, v in Args.transforms.items() if k != "ToTensor"})
    sync_ms, dc_ms, dc_syncs = [], [], []

    def sync_side(xyz):
        return preprocess_scan(xyz, outlier=OUTLIER, lowpass=LOWPASS)[0]

    def dc_side(xyz):
        return augment.collate_frames(augment.transform_frames([augment.PointCloud(xyz)], chain, streams=1), -1)[0]

    for k, xyz in enumerate(scans):
        xyz = xyz.to(DEV)
        sides = (("sync", sync_side), ("dc", dc_side)) if k % 2 == 0 else (("dc", dc_side), ("sync", sync_side))
        outs = {}
        for name, fn in sides:                      # the two sides alternate, the order swapped every frame
            before = augment.host_syncs()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[name] = fn(xyz)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if k >= warm:
                (sync_ms if name == "sync" else dc_ms).append(ms)
                if name == "dc":
                    dc_syncs.append(augment.host_syncs() - before)
        assert torch.equal(outs["sync"][0], outs["dc"][0]), f"frame {k}: the two paths disagree"
    return sync_ms, dc_ms, dc_syncs


def bench_wait(d, prefetch, warm=8):
    from deeppointmap_amd.encoder import Encoder
    from deeppointmap_amd.loader import SceneLoader
    from deeppointmap_amd.weights import init_procedural
    enc = init_procedural(Encoder(default_args())).to(DEV)
    agent = dataset.BasicAgent(d, "auto")
    waits, steps = [], []
    with SceneLoader(agent, augment.PointCloudTransforms(Args, mode="infer"), group=4, prefetch=prefetch, device=DEV) as ld:
        it = iter(ld)
        for k in range(len(ld)):
            t0 = time.perf_counter()
            pts, R, T, pad, original = next(it)
            t1 = time.perf_counter()
            enc(pts, pad)                           # the stand-in consumer
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if k >= warm:
                waits.append((t1 - t0) * 1e3), steps.append((t2 - t1) * 1e3)
    return waits, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_loader_bench.md"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--points", type=int, default=120000)
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    with tempfile.TemporaryDirectory() as d:
        scans = write_scene(d, a.frames, a.points)
        sync_ms, dc_ms, dc_syncs = bench_chain(scans)
        rows = []
        for prefetch in (0, 1, 2):
            w, s = bench_wait(d, prefetch)
            rows.append(f"| {prefetch} | {spread(w)} | {spread(s)} | {len(w)} |")
    lines = ["# Scene loader bench", "",
             f"One run on {torch.cuda.get_device_name(0)}; {a.frames} `.bin` frames of raw_scan({a.points}, seed).  Milliseconds: "
             "median (10th .. 90th percentile).  A report, not a target.", "",
             "## (a), (b) the full shipped chain per frame, the two paths alternating (equal bytes asserted per frame)", "",
             "| path | per frame, synchronised | host synchronisations per frame |", "|---|---|---|",
             f"| preprocess_scan(outlier=, lowpass=): the length on the host | {spread(sync_ms)} | {SYNC_PATH_SYNCS} (from its code) |",
             f"| class-layer chain + collate_frames: the length in device memory | {spread(dc_ms)} | {max(dc_syncs)} (counted) |", "",
             "## (c) SceneLoader(group=4), Encoder.forward as the stand-in consumer", "",
             "| prefetch | the consumer's wait per frame | Encoder.forward, synchronised | frames |", "|---|---|---|---|", *rows, ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
