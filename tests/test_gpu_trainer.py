"""GPU: the Trainer.  (a) its bookkeeping against the reference's Trainer.run() on the stubs of tests/trainer_stub.py
(tests/golden/trainer_trace.json, made by tests/golden/make_golden_trainer.py); (b) an end-to-end run of the reduced model
on the tree of tests/dataset_tree.py through EpochLoader: finite losses, loadable weights, identical bytes when repeated and
when stopped after epoch 1 and resumed from its checkpoint."""
import copy
import json
import math
import os
import sys
from types import SimpleNamespace

import pytest
import torch

import dataset_tree
import trainer_stub
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS = dict(tau=0.1, offset_value="manhattan", eps_positive=1.0, eps_offset=2.0, lambda_p=1.0, lambda_c=1.0, lambda_o=1.0)
CHAIN = {"VoxelSample": {"voxel_size": 0.3, "retention": "first"}, "ToGPU": {}, "DistanceSample": {"min_dis": 1.0, "max_dis": 60.0},
         "RandomRT": {}, "RandomDrop": {"max_ratio": 0.2}, "CoordinatesNormalization": {"ratio": 60.0}, "ToCPU": {},
         "ToTensor": {"padding_to": 2048, "use_calib": True}}


class Recording:
    def __init__(self):
        self.calls = []

    def add_scalar(self, tag, value, step):
        self.calls.append([tag, int(step), float(value) if tag.startswith("runtime/") else None])


# ---------------------------------------------------------------------------------------------------------------- the trace
class StubLoader:
    def __init__(self, steps, batch_size):
        self.steps, self.batch_size = steps, batch_size

    def set_epoch(self, ep):
        pass

    def __len__(self):
        return self.steps

    def __iter__(self):
        for _ in range(self.steps):
            yield (torch.zeros(self.batch_size, 1, device=DEV),)

    def close(self):
        pass


class StubDataset(trainer_stub.StubDataset):
    def epoch_loader(self, stage, batch_size, rank, world):
        return StubLoader(len(self) // batch_size, batch_size)


def stub_run(work, checkpoint="", save_cycle=None):
    from deeppointmap_amd.config import Cfg
    from deeppointmap_amd.trainer import Trainer
    os.makedirs(work)
    cwd = os.getcwd()
    os.chdir(work)
    try:
        cfg = copy.deepcopy(trainer_stub.train_config())
        if save_cycle is not None:
            cfg["save_cycle"] = save_cycle
        args = Cfg(train=cfg, **trainer_stub.args_dict(checkpoint, DEV))
        writer = Recording()
        Trainer(args, StubDataset(), trainer_stub.StubPipeline(), writer=writer).run()
        files = sorted(os.path.relpath(os.path.join(d, f), ".") for d, _, fs in os.walk(".") for f in fs)
        ckpts = {}
        for f in files:
            if f.endswith((".ckpt", ".pth")):
                state = torch.load(f, map_location="cpu", weights_only=False)
                ckpts[os.path.basename(f)] = ({"epoch": state["epoch"], "step": state["step"], "keys": sorted(state)}
                                              if f.endswith(".ckpt") else {"keys": sorted(state)})
    finally:
        os.chdir(cwd)
    return {"scalars": writer.calls, "files": files, "checkpoints": ckpts}


def test_trainer_reproduces_the_reference_trace(tmp_path):
    with open(os.path.join(GOLDEN, "trainer_trace.json")) as f:
        want = json.load(f)
    tmp = str(tmp_path)
    got = {"fresh": stub_run(os.path.join(tmp, "fresh"))}
    every = stub_run(os.path.join(tmp, "every"), save_cycle=1)          # save_cycle=2 never writes the epoch-3 checkpoint
    log = "log_train/StubV1_config=stub.yaml"
    got["resume2"] = stub_run(os.path.join(tmp, "resume2"), os.path.join(tmp, "fresh", log, "StubV1_epoch2.ckpt"))
    got["resume3"] = stub_run(os.path.join(tmp, "resume3"), os.path.join(tmp, "every", log, "StubV1_epoch3.ckpt"))
    assert every["checkpoints"]["StubV1_epoch3.ckpt"]["epoch"] == 3
    for run in ("fresh", "resume2", "resume3"):
        w, g = want[run], got[run]
        assert [c[:2] for c in g["scalars"]] == [c[:2] for c in w["scalars"]], run        # tags and steps, in order
        assert g["scalars"] == w["scalars"], run                                            # and the runtime/* values
        assert g["files"] == [f for f in w["files"] if not f.endswith("codes.zip")], run    # codes.zip is left out on purpose
        assert g["checkpoints"] == w["checkpoints"], run
    assert os.path.exists(os.path.join(tmp, "fresh", log, "settings.yaml"))


def test_default_writer_and_refusals(tmp_path):
    from deeppointmap_amd.config import Cfg
    from deeppointmap_amd.trainer import JsonlWriter, Trainer, default_writer
    w = default_writer(str(tmp_path / "log_tb" / "x"))
    w.add_scalar("runtime/K", 2, 1)
    w.add_scalar("train/step_loss", 0.5, 3)
    if isinstance(w, JsonlWriter):
        w.close()
        lines = [json.loads(line) for line in open(tmp_path / "log_tb" / "x" / "scalars.jsonl")]
        assert lines == [{"tag": "runtime/K", "value": 2.0, "step": 1}, {"tag": "train/step_loss", "value": 0.5, "step": 3}]
    cfg = trainer_stub.train_config()
    cfg["auto_cast"] = True
    with pytest.raises(NotImplementedError):
        Trainer(Cfg(train=cfg, **trainer_stub.args_dict("", DEV)), StubDataset(), trainer_stub.StubPipeline())
    assert Trainer.remove_module(Trainer.add_module({"a": 1, "module.b": 2})) == {"a": 1, "b": 2}


# ---------------------------------------------------------------------------------------------------------------- end to end
def e2e_args(root, checkpoint="", reg_epochs=2, loop_epochs=1):
    from deeppointmap_amd.config import reduced_args
    cfg = reduced_args()
    tree = dataset_tree.tree_config(root)
    cfg.loss = dict(LOSS)
    cfg.dataset = tree["dataset"]
    cfg.transforms = dict(CHAIN)
    cfg.train = dict(
        auto_cast=False, log_cycle=12, save_cycle=1,
        registration=dict(tree["train"]["registration"], num_epochs=reg_epochs, batch_size=12, K_0=2, K_mult=2, mult_epoch=[2],
                          optimizer=dict(type="AdamW", kwargs=dict(lr=1e-4, weight_decay=1e-2)),
                          scheduler=dict(type="cosine", kwargs=dict(T_max=10))),
        loop_detection=dict(tree["train"]["loop_detection"], num_epochs=loop_epochs, batch_size=12,
                            optimizer=dict(type="sgd", kwargs=dict(lr=1e-3, momentum=0.9)),
                            scheduler=dict(type="identity", kwargs={})))
    cfg.loader = dict(rng=7, prefetch=2, capacity=2048, padding_to=2048)
    for k, v in dict(name="E2E", version="V0", yaml_file="configs/e2e.yaml", use_ddp=False, local_rank=0, checkpoint=checkpoint,
                     weight="", device=DEV, num_workers=2).items():
        cfg[k] = v
    return cfg


def e2e_run(root, work, checkpoint="", stop_after=None):
    """-> (trainer, recorded scalars with their values); stop_after: leave the loop after that epoch (its checkpoint is written)"""
    import encoder_train_cases as EC
    from deeppointmap_amd import augment, dataset
    from deeppointmap_amd.decoder import Decoder
    from deeppointmap_amd.encoder import Encoder
    from deeppointmap_amd.loss import RegistrationLoss
    from deeppointmap_amd.train_pipeline import DeepPointModelPipeline
    from deeppointmap_amd.trainer import Trainer
    from deeppointmap_amd.weights import init_procedural
    os.makedirs(work, exist_ok=True)
    cwd = os.getcwd()
    os.chdir(work)
    try:
        cfg = e2e_args(root, checkpoint)
        enc = Encoder(cfg)
        enc.load_state_dict(EC.state_dict(cfg), strict=True)
        dec = init_procedural(Decoder(cfg))
        model = DeepPointModelPipeline(cfg, enc.to(DEV).set_train_dense("hip"), dec.to(DEV).set_train_dense("hip"), RegistrationLoss(cfg))
        ds = dataset.SlamDatasets(cfg, data_transforms=augment.PointCloudTransforms(cfg, mode="train"))
        values = []
        writer = SimpleNamespace(add_scalar=lambda tag, value, step: values.append((tag, float(value), int(step))))
        trainer = Trainer(cfg, ds, model, writer=writer)
        if stop_after is not None:
            class Stop(Exception):
                pass
            save = trainer.save

            def save_and_stop(finish=False):
                save(finish)
                if trainer.epoch == stop_after:
                    raise Stop
            trainer.save = save_and_stop
            with pytest.raises(Stop):
                trainer.run()
        else:
            trainer.run()
    finally:
        os.chdir(cwd)
    return trainer, values


def weight_bytes(path):
    state = torch.load(path, map_location="cpu", weights_only=False)
    return {f"{part}.{k}": v.numpy().tobytes() for part in ("encoder", "decoder") for k, v in state[part].items()}


def test_end_to_end_training_on_the_tree(tmp_path):
    import threading
    sys.path.insert(0, GOLDEN)
    from deeppointmap_amd.decoder import Decoder
    from deeppointmap_amd.encoder import Encoder
    root = str(tmp_path / "tree")
    dataset_tree.write_tree(root, 2048)
    dataset_tree.write_refined_tables(root)
    log = os.path.join("log_train", "E2EV0_config=e2e.yaml")
    trainer, values = e2e_run(root, str(tmp_path / "a"))
    assert trainer.epoch == 4 and trainer.step == 1 + 3 * 4                 # 48 // 12 steps in each of the three epochs
    assert len(trainer.dataloader) == 4
    losses = [(t, v) for t, v, _ in values if t.startswith("train/")]
    assert {t for t, _ in losses} >= {"train/epoch_loss_regis", "train/step_loss_regis", "train/epoch_top1_acc"}
    assert {t for t, _, s in values if t.startswith("train/epoch_") and s == 3} >= {"train/epoch_loss_loop"}   # the third epoch is loop detection
    assert all(math.isfinite(v) for _, v in losses), [x for x in losses if not math.isfinite(x[1])]
    assert [v for t, v, _ in values if t == "runtime/K"] == [2.0, 4.0]
    pth = os.path.join(str(tmp_path / "a"), log, "E2EV0.pth")
    state = torch.load(pth, map_location="cpu", weights_only=False)
    cfg = e2e_args(root)
    Encoder(cfg).load_state_dict(state["encoder"], strict=True), Decoder(cfg).load_state_dict(state["decoder"], strict=True)
    first = weight_bytes(pth)
    start = weight_bytes(os.path.join(str(tmp_path / "a"), log, "E2EV0_epoch1.ckpt"))
    assert sum(first[k] != start[k] for k in first) > 100                    # training moved the weights after epoch 1
    # repeated: identical weight bytes
    e2e_run(root, str(tmp_path / "b"))
    assert weight_bytes(os.path.join(str(tmp_path / "b"), log, "E2EV0.pth")) == first
    # stopped after epoch 1, resumed from its checkpoint: the same final weight bytes
    e2e_run(root, str(tmp_path / "c"), stop_after=1)
    ckpt = os.path.join(str(tmp_path / "c"), log, "E2EV0_epoch1.ckpt")
    resumed, _ = e2e_run(root, str(tmp_path / "d"), checkpoint=ckpt)
    assert resumed.epoch == 4 and resumed.step == 13
    assert weight_bytes(os.path.join(str(tmp_path / "d"), log, "E2EV0.pth")) == first
    assert not [t for t in threading.enumerate() if t.name == "deeppointmap-loader"]
