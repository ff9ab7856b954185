"""The stub configuration, dataset and pipeline that tests/golden/make_golden_trainer.py runs THE REFERENCE's Trainer on and
tests/test_gpu_trainer.py runs this project's Trainer on: what is compared is the bookkeeping of the loop (scalar tags and
steps, learning rates, files, checkpoint counters), not a model.

8 items; registration: 3 epochs of 4 steps (batch_size 2), K_0=2, K_mult=2, mult_epoch=[2,3]; loop detection: 2 epochs of 2
steps (batch_size 4); save_cycle=2; log_cycle=4, so log_interval is 2 in the registration stage and 1 in the other.  The
schedulers are cosine ones (the reference's factory knows identity | cosine | cosine_restart): the learning rate differs
from epoch to epoch, so a resumed run shows whether the scheduler state came back.
"""
import torch
from torch import nn

N_ITEMS = 8


def train_config():
    return {
        "auto_cast": False, "log_cycle": 4, "save_cycle": 2,
        "registration": {"num_epochs": 3, "batch_size": 2, "K": 2, "K_0": 2, "K_mult": 2, "mult_epoch": [2, 3],
                         "optimizer": {"type": "AdamW", "kwargs": {"lr": 1e-3, "weight_decay": 0.0}},
                         "scheduler": {"type": "cosine", "kwargs": {"T_max": 3, "eta_min": 1e-5}}},
        "loop_detection": {"num_epochs": 2, "batch_size": 4,
                           "optimizer": {"type": "SGD", "kwargs": {"lr": 1e-2}},
                           "scheduler": {"type": "cosine", "kwargs": {"T_max": 2}}},
    }


def args_dict(checkpoint="", device="cpu"):
    return dict(name="Stub", version="V1", yaml_file="configs/stub.yaml", use_ddp=False, local_rank=0, checkpoint=checkpoint,
                weight="", device=device, num_workers=0)


class StubDataset(torch.utils.data.Dataset):
    def __init__(self):
        self.collate_fn = None
        self.registration()

    def __len__(self):
        return N_ITEMS

    def __getitem__(self, item):
        return torch.tensor([float(item)])

    def registration(self):
        self.collate_fn = lambda batch: (torch.stack(batch),)

    def loop_detection(self):
        self.collate_fn = None


class StubPipeline(nn.Module):
    """`.encoder` / `.decoder` of one parameter each; the metrics are a fixed function of the call count"""

    def __init__(self):
        super().__init__()
        self.encoder = nn.Linear(1, 1, bias=False)
        self.decoder = nn.Linear(1, 1, bias=False)
        self.calls = 0
        self.stage = None
        self.registration()

    def registration(self):
        self.stage = "registration"

    def loop_detection(self):
        self.stage = "loop_detection"

    def forward(self, *data, **kw):
        self.calls += 1
        loss = self.encoder.weight.sum() + self.decoder.weight.sum()
        return loss, {"loss": 1.0 / self.calls, "acc": 0.5 * self.calls}
