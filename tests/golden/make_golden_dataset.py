#!/usr/bin/env python3
"""dataset_draws.json / dataset_ref.npz: THE REFERENCE's dataset tree (dataloader/body.py, dataloader/heads/*) on the tree
of tests/dataset_tree.py, run on the CPU.  Needs a checkout of the reference:
`python make_golden_dataset.py <reference checkout>` (see make_golden.py for the rules); `colorlog` / `open3d` /
`pytorch3d` are stubbed as in make_golden_augment.py; `easydict` is replaced by the project's own attribute dict.

For seeds {1, 2, 3} x all 48 indices x both stages, with a transform that returns the frame id (`lidar_pcd[0, 0]`):
  registration    S, num_map, dsf_index, the refined-file paths relative to the tree, the ordered frame ids read
  loop detection  the pair of frame ids
(`random.seed(seed)` once per seed and stage, the indices 0..47 drawn in order.)  dataset_ref.npz holds the bytes of the
three scenes' frame_dis.npy as the reference wrote them and the reference readers' (xyz, R, T) for one .npz, one .npy and
one .bin file.  The reference works on a copy of the tree in a temporary directory (it writes frame_dis.npy into it).
"""
import json
import logging
import os
import random
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.modules["colorlog"] = logging
sys.modules.setdefault("open3d", types.ModuleType("open3d"))
for name in ("pytorch3d", "pytorch3d.ops"):
    sys.modules[name] = types.ModuleType(name)
ops_mod = sys.modules["pytorch3d.ops"]
ops_mod.knn_points = ops_mod.sample_farthest_points = ops_mod.ball_query = ops_mod.knn_gather = None
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "dataloader")):
    sys.exit("usage: make_golden_dataset.py <reference checkout>")
sys.path.insert(0, sys.argv[1])
sys.path.insert(1, ROOT)
sys.path.insert(2, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import dataset_tree  # noqa: E402
from deeppointmap_amd.config import Cfg  # noqa: E402
from dataloader.body import BinReader, NPYReader, NPZReader, SlamDatasets  # noqa: E402

SEEDS = (1, 2, 3)


def frame_id(pcd):
    return (torch.tensor(float(pcd.xyz[0, 0])),)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        tree = os.path.join(tmp, "tree")
        dataset_tree.write_tree(tree)
        ds = SlamDatasets(Cfg(dataset_tree.tree_config(tree)), data_transforms=frame_id)
        n = int(len(ds))
        assert n == dataset_tree.N_FRAMES
        draws = {"seeds": list(SEEDS), "n": n, "registration": {}, "loop_detection": {}}
        for seed in SEEDS:
            ds.registration()
            random.seed(seed)
            rows = []
            for index in range(n):
                frames, info = ds[index]
                S = len(frames) // info["num_map"]
                rows.append({"S": S, "num_map": int(info["num_map"]),
                             "dsf_index": [[int(v) for v in t] for t in info["dsf_index"]],
                             "refined_SE3_file": [os.path.relpath(p, tree) if p else "" for p in info["refined_SE3_file"]],
                             "frames": [int(f[0]) for f in frames]})
            draws["registration"][str(seed)] = rows
            ds.loop_detection()
            random.seed(seed)
            draws["loop_detection"][str(seed)] = [[int(v) for v in ds[index]] for index in range(n)]
        ref = {}
        for name, scene in (("KITTI_00", ("KITTI", "00")), ("KITTI_01", ("KITTI", "01")), ("Carla_Town_00", ("Carla_Town", "00"))):
            ref["frame_dis_" + name] = np.load(os.path.join(tree, *scene, "frame_dis.npy"))
        files = dataset_tree.write_reader_files(os.path.join(tmp, "readers"))
        for kind, reader in (("npz", NPZReader()), ("npy", NPYReader()), ("bin", BinReader())):
            pcd = reader(files[kind])
            ref[kind + "_xyz"], ref[kind + "_R"], ref[kind + "_T"] = pcd.xyz.numpy(), pcd.R.numpy(), pcd.T.numpy()
    with open(os.path.join(HERE, "dataset_draws.json"), "w") as f:
        json.dump(draws, f, separators=(",", ":"))
    np.savez_compressed(os.path.join(HERE, "dataset_ref.npz"), **ref)
    print("wrote dataset_draws.json, dataset_ref.npz:", {k: v.shape for k, v in ref.items()})


if __name__ == "__main__":
    main()
