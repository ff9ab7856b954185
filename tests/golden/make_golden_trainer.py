#!/usr/bin/env python3
"""trainer_trace.json: THE REFERENCE's Trainer.run() (pipeline/modules/trainer.py) on the CPU over the stubs of
tests/trainer_stub.py, in a temporary working directory, num_workers=0.  Needs a checkout of the reference:
`python make_golden_trainer.py <reference checkout>` (see make_golden.py for the rules).  `colorlog` / `open3d` /
`pytorch3d` are stubbed as in make_golden_augment.py, `easydict` is replaced by the project's own attribute dict, and
`torch.utils.tensorboard` by a writer that records its calls.

Recorded per run: every add_scalar call as [tag, step, value] (the value only for the runtime/* tags, else null), the files
below the working directory, and the `epoch` / `step` stored in each .ckpt.  Three runs: "fresh"; "resume2" from the fresh
run's epoch-2 checkpoint; "resume3" from an epoch-3 checkpoint -- the stage boundary, where optimiser and scheduler state
are not restored (trainer.py:289) --, which an unrecorded run with save_cycle=1 writes (save_cycle=2 never saves epoch 3).
"""
import argparse
import copy
import json
import logging
import os
import shutil
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.modules["colorlog"] = logging
sys.modules.setdefault("open3d", types.ModuleType("open3d"))
for name in ("pytorch3d", "pytorch3d.ops"):
    sys.modules[name] = types.ModuleType(name)
ops_mod = sys.modules["pytorch3d.ops"]
ops_mod.knn_points = ops_mod.sample_farthest_points = ops_mod.ball_query = ops_mod.knn_gather = None
if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "pipeline")):
    sys.exit("usage: make_golden_trainer.py <reference checkout>")
sys.path.insert(0, sys.argv[1])
sys.path.insert(1, ROOT)
sys.path.insert(2, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

CALLS = []


class RecordingWriter:
    def __init__(self, *a, **kw):
        pass

    def add_scalar(self, tag, value, step):
        CALLS.append([tag, int(step), float(value) if tag.startswith("runtime/") else None])


tb = types.ModuleType("torch.utils.tensorboard")
tb.SummaryWriter = RecordingWriter
sys.modules["torch.utils.tensorboard"] = tb

import trainer_stub  # noqa: E402
from deeppointmap_amd.config import Cfg  # noqa: E402
from pipeline.modules.trainer import Trainer  # noqa: E402  (reference)


def one_run(checkpoint="", save_cycle=None):
    cfg = copy.deepcopy(trainer_stub.train_config())
    if save_cycle is not None:
        cfg["save_cycle"] = save_cycle
    args = argparse.Namespace(train=Cfg(cfg), **trainer_stub.args_dict(checkpoint))
    torch.manual_seed(0)
    CALLS.clear()
    Trainer(args, trainer_stub.StubDataset(), trainer_stub.StubPipeline()).run()
    return [list(c) for c in CALLS]


def listing():
    out = []
    for d, _, files in os.walk("."):
        out += [os.path.relpath(os.path.join(d, f), ".") for f in files]
    return sorted(out)


def checkpoints():
    out = {}
    for f in listing():
        if f.endswith(".ckpt"):
            state = torch.load(f, map_location="cpu")
            out[os.path.basename(f)] = {"epoch": int(state["epoch"]), "step": int(state["step"]), "keys": sorted(state)}
        if f.endswith(".pth"):
            out[os.path.basename(f)] = {"keys": sorted(torch.load(f, map_location="cpu"))}
    return out


def recorded(tmp, name, checkpoint="", **kw):
    work = os.path.join(tmp, name)
    os.makedirs(work)
    os.chdir(work)
    scalars = one_run(checkpoint, **kw)
    return {"scalars": scalars, "files": listing(), "checkpoints": checkpoints()}


def main():
    cwd = os.getcwd()
    trace = {}
    with tempfile.TemporaryDirectory() as tmp:
        try:
            trace["fresh"] = recorded(tmp, "fresh")
            ckpt_dir = os.path.join(tmp, "fresh", os.path.dirname([f for f in trace["fresh"]["files"] if f.endswith("_epoch2.ckpt")][0]))
            ckpt2 = os.path.join(tmp, "epoch2.ckpt")
            shutil.copy(os.path.join(ckpt_dir, "StubV1_epoch2.ckpt"), ckpt2)
            every = recorded(tmp, "every_epoch", save_cycle=1)
            ckpt3 = os.path.join(tmp, "epoch3.ckpt")
            shutil.copy(os.path.join(tmp, "every_epoch", [f for f in every["files"] if f.endswith("_epoch3.ckpt")][0]), ckpt3)
            trace["resume2"] = recorded(tmp, "resume2", ckpt2)
            trace["resume3"] = recorded(tmp, "resume3", ckpt3)
        finally:
            os.chdir(cwd)
    with open(os.path.join(HERE, "trainer_trace.json"), "w") as f:
        json.dump(trace, f, indent=0)
    for k, v in trace.items():
        print(k, len(v["scalars"]), "scalars;", v["files"], v["checkpoints"])


if __name__ == "__main__":
    main()
