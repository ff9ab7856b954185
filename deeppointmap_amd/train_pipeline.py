"""The training step of the reference on the MI355X: `DeepPointModelPipeline` (pipeline/modules/model_pipeline.py) over this
project's Encoder, Decoder and losses, and `TrainStep`, the part of pipeline/modules/trainer.py that takes a step.

What the reference's `_train_registration` does between the encoder and the decoder -- split the B x S encoded frames into a
source map and a target map, compose every frame's pose into its map's first frame from a pickled table of refined SE3s (with
calibration matrices, a "bridge" frame, and the global poses wherever the table has no answer), move the key points and
interleave (B,S,C,N) into (B,C,S*N) -- is a Python loop over the frames there.  Here the host only answers "which entries does
the table have" (`icp_table`, numpy, no device work), sends that in one non-blocking copy, and csrc/map_assemble.hip does the
rest in two launches (`ops.map_poses`, `ops.map_assemble`).

A singular `calib` is not supported: the reference would take the global poses through its bare `except`, the host here never
sees the matrix, and the kernel's inverse returns Inf / NaN.
"""
from __future__ import annotations

import pickle
import random
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from . import ops
from .loss import LoopDetectionLoss
from .optim import Optimizer, Scheduler

METRIC_KEYS = ("loss_regis", "loss_p", "loss_c", "loss_o", "top1_acc", "offset_err")


def refined_pose(table: Dict[Tuple[int, int], np.ndarray], s, d, bridge=None) -> Optional[np.ndarray]:
    """The refined pose of frame s in frame d as the reference's get_SE3_from_dict (model_pipeline.py:285-298) finds it, float64
    4x4, or None where that function fails (which the reference's caller answers with the global poses).  The table is keyed
    (smaller frame, larger frame) and holds the pose of the larger in the smaller: s == d is the identity, s > d the entry
    (d, s), s < d the inverse of the entry (s, d); a pair without an entry goes over the bridge frame, (bridge -> d) @ (s ->
    bridge), each leg looked up directly -- without a bridge, or with a leg missing, there is no pose."""
    def direct(a, b):
        if a == b:
            return np.eye(4)
        if a < b:
            M = table.get((a, b))
            return None if M is None else np.linalg.inv(M)
        return table.get((b, a))
    try:
        M = direct(s, d)
        if M is None:
            if bridge is None:
                return None
            first, second = direct(s, bridge), direct(bridge, d)
            if first is None or second is None:
                return None
            M = second @ first
        M = np.asarray(M, np.float64)
        return M if M.shape == (4, 4) else None
    except Exception:   # a singular entry, a malformed value: the reference's bare `except`
        return None


def icp_table(pcd_index: np.ndarray, tables, S1: int):
    """pcd_index (B,S) frame numbers, tables: per map its refined-SE3 dictionary or None -> icp (F+B,16) float32, has_icp (F+B,)
    uint8 for ops.map_poses.  Entry b*S + s: frame (b,s) into the first frame of its map (the bridge of a target-map frame is
    the source map's first frame, model_pipeline.py:88-94; the other two call sites pass none); entry F + b: map b's
    source-first into its target-first.  float64 lookup, then float32, as the reference's `.float()`."""
    B, S = pcd_index.shape
    F = B * S
    icp = np.zeros((F + B, 16), np.float32)
    has = np.zeros(F + B, np.uint8)
    for b in range(B):
        table = tables[b]
        if table is None:
            continue
        idx = [int(i) for i in pcd_index[b]]
        todo = [(F + b, idx[0], idx[S1], None)]
        todo += [(b * S + s, idx[s], idx[0], None) for s in range(1, S1)]
        todo += [(b * S + s, idx[s], idx[S1], idx[0]) for s in range(S1 + 1, S)]
        for e, s, d, bridge in todo:
            M = refined_pose(table, s, d, bridge)
            if M is not None:
                icp[e], has[e] = M.reshape(16), 1
    return icp, has


def draw_s1(S: int, map_size_max: int, rng=random) -> int:
    """how many of a map's S frames form the source map: the reference's draws in the reference's order
    (model_pipeline.py:52-59), so that a seeded run picks the reference's S1"""
    if S <= map_size_max:
        if rng.random() < 0.5:
            return 1
        return rng.randint(1, S - 1)
    return rng.randint(S - map_size_max, map_size_max)


class DeepPointModelPipeline(nn.Module):
    """The reference's class: constructor (args, encoder, decoder, criterion), forward(*args) -> (loss, metric_dict),
    registration() / loop_detection() to switch the stage, refined_SE3_cache.  encoder and decoder are this project's modules;
    both stage methods also tell them the stage (`set_train_stage`), which survives the trainer's `model.train()`."""

    def __init__(self, args, encoder: nn.Module, decoder: nn.Module, criterion: nn.Module):
        super().__init__()
        self.args = args
        self.encoder = encoder
        self.decoder = decoder
        self.criterion = criterion
        self.loop_criterion = None
        self._forward_method = None
        self.registration()
        self.refined_SE3_cache = dict()

    def forward(self, *args, **kwargs) -> Tuple[Tensor, dict]:
        return self._forward_method(*args, **kwargs)

    def _set_stage(self, stage: str, trains) -> None:
        for name, param in self.named_parameters():
            param.requires_grad = trains(name)
        self.encoder.set_train_stage(stage)
        self.decoder.set_train_stage(stage)

    def registration(self):
        self._forward_method = self._train_registration
        self._set_stage("registration", lambda name: "loop" not in name)

    def loop_detection(self):
        self._forward_method = self._train_loop_detection
        self.loop_criterion = LoopDetectionLoss(self.args)
        self._set_stage("loop_detection", lambda name: "loop" in name)

    def _load_refined_SE3(self, file):
        """the dictionary of a file, loaded once; '' = none (the whole map takes the global poses)"""
        if file not in self.refined_SE3_cache:
            table = None
            if file != "":
                with open(file, "rb") as f:
                    table = pickle.load(f)
            self.refined_SE3_cache[file] = table
        return self.refined_SE3_cache[file]

    def _train_registration(self, pcd: Tensor, R: Tensor, T: Tensor, padding_mask: Tensor, calib: Tensor, info: dict,
                            s1: Optional[int] = None) -> Tuple[Tensor, dict]:
        coor, fea, mask = self.encoder(pcd, padding_mask)
        F, _, N = coor.shape
        B = info["num_map"]
        S = F // B
        dev = fea.device
        S1 = draw_s1(S, self.args.train.registration.map_size_max) if s1 is None else int(s1)
        pcd_index = np.asarray([i[2] for i in info["dsf_index"]]).reshape(B, S)
        icp, has = icp_table(pcd_index, [self._load_refined_SE3(f) for f in info["refined_SE3_file"]], S1)
        # one pinned buffer, one non-blocking copy: the poses' bytes, then the flags
        host = torch.from_numpy(np.concatenate([icp.reshape(-1).view(np.uint8), has])).pin_memory()
        sent = host.to(dev, non_blocking=True)
        icp_d, has_d = sent[:icp.nbytes].view(torch.float32).view(F + B, 16), sent[icp.nbytes:]
        f32 = lambda t, *shape: t.detach().to(dev, torch.float32).reshape(*shape).contiguous()   # noqa: E731
        rel, gt = ops.map_poses(f32(R, F, 3, 3), f32(T, F, 3, 1), f32(calib, F, 4, 4), icp_d, has_d, S, S1)
        src_desc, dst_desc, src_mask, dst_mask, src_global, dst_global = ops.map_assemble(
            coor.detach().contiguous(), fea, mask.contiguous(), rel, gt, S, S1, self.args.slam_system.coor_scale)
        gt = gt.view(B, 3, 4)
        src_pairing_fea, dst_pairing_fea, src_coarse_pairing_fea, dst_coarse_pairing_fea, src_offset_res, dst_offset_res = \
            self.decoder(src_desc, dst_desc, src_padding_mask=src_mask, dst_padding_mask=dst_mask,
                         gt_Rt=(gt[:, :, :3], gt[:, :, 3:]))
        loss, top1_pairing_acc, loss_pairing, loss_coarse_pairing, loss_offset = self.criterion(
            src_global_coor=src_global, dst_global_coor=dst_global, src_padding_mask=src_mask, dst_padding_mask=dst_mask,
            src_pairing_fea=src_pairing_fea, dst_pairing_fea=dst_pairing_fea,
            src_coarse_pairing_fea=src_coarse_pairing_fea, dst_coarse_pairing_fea=dst_coarse_pairing_fea,
            src_offset_res=src_offset_res, dst_offset_res=dst_offset_res)
        offset_err = (torch.norm(src_offset_res.detach(), p=2, dim=1).mean() +
                      torch.norm(dst_offset_res.detach(), p=2, dim=1).mean()) / 2
        scalar = lambda v: torch.as_tensor(v, dtype=torch.float32, device=dev).detach().reshape(())   # noqa: E731
        values = torch.stack([scalar(loss), scalar(loss_pairing), scalar(loss_coarse_pairing), scalar(loss_offset),
                              scalar(offset_err)]).tolist()   # the metrics leave the device in one copy
        metric_dict = dict(zip(METRIC_KEYS, (*values[:4], top1_pairing_acc, values[4])))
        return loss, metric_dict

    def _train_loop_detection(self, src_pcd: Tensor, src_R: Tensor, src_T: Tensor, src_mask: Tensor, src_calib: Tensor,
                              dst_pcd: Tensor, dst_R: Tensor, dst_T: Tensor, dst_mask: Tensor, dst_calib: Tensor
                              ) -> Tuple[Tensor, dict]:
        B = src_pcd.shape[0]
        coor, fea, mask = self.encoder(torch.cat([src_pcd, dst_pcd], dim=0), torch.cat([src_mask, dst_mask], dim=0))
        coor = coor * self.args.slam_system.coor_scale
        loop_pred = self.decoder.loop_detection_forward(
            src_descriptor=torch.cat([fea[:B], coor[:B]], dim=1), dst_descriptor=torch.cat([fea[B:], coor[B:]], dim=1),
            src_padding_mask=mask[:B], dst_padding_mask=mask[B:])
        return self.loop_criterion(loop_pred, src_T, dst_T)


class TrainStep:
    """What pipeline/modules/trainer.py does around one optimiser step, without its DataLoader and tensorboard (its DDP: data_parallel.DataParallelTrainStep): the model,
    and the optimiser and scheduler that deeppointmap_amd.optim's factories build from `args.train.<stage>.optimizer` /
    `.scheduler` over the parameters the stage trains.  Epochs count from 1, as there."""

    STAGES = ("registration", "loop_detection")

    def __init__(self, args, model: DeepPointModelPipeline, stage: str = "registration"):
        self.args = args
        self.train_cfg = args.train
        self.model = model
        self.epoch = 1
        self.step_count = 0
        self._entered = False
        self._enter(stage)

    def _enter(self, stage: str) -> None:
        if stage not in self.STAGES:
            raise ValueError(f"stage must be one of {self.STAGES}, got {stage!r}")
        self.stage = stage
        getattr(self.pipeline, stage)()
        cfg = self.train_cfg[stage] if isinstance(self.train_cfg, dict) else getattr(self.train_cfg, stage)
        self.optimizer = Optimizer(cfg.optimizer)(filter(lambda p: p.requires_grad, self.model.parameters()))
        self.scheduler = Scheduler(cfg.scheduler)(self.optimizer)
        self._entered = False

    @property
    def pipeline(self) -> DeepPointModelPipeline:
        """the DeepPointModelPipeline itself (`self.model` may be a wrapper around it: data_parallel.DataParallelTrainStep)"""
        return self.model

    def step(self, *data) -> dict:
        """model.train() once per epoch, forward, zero_grad, backward, optimizer.step() (trainer.py:159, 174-178)"""
        if not self._entered:
            self.model.train()
            self._entered = True
        with torch.enable_grad():
            loss, metric = self.model(*data)
            self.optimizer.zero_grad()
            loss.backward()
        self.optimizer.step()
        self.step_count += 1
        return metric

    def epoch_end(self) -> None:
        """scheduler.step(), the next epoch, and for a registration epoch the K_0 / K_mult / mult_epoch rule (trainer.py:107,
        115, 130-140): K = K_0 * K_mult ** (number of mult_epoch entries the epoch has reached)"""
        self.scheduler.step()
        self.epoch += 1
        self._entered = False
        if self.stage == "registration":
            cfg = self.train_cfg.registration
            if "K_0" in cfg.keys():
                cfg["K"] = cfg["K_0"] * (cfg["K_mult"] ** sum(1 for e in cfg["mult_epoch"] if self.epoch >= e))

    def next_stage(self) -> None:
        """registration -> loop detection with a new optimiser and scheduler over the parameters that stage trains
        (trainer.py:313-336 without the loaders)"""
        self._enter("loop_detection")

    def state_dict(self) -> dict:
        """the reference's .ckpt layout"""
        return {"encoder": self.pipeline.encoder.state_dict(), "decoder": self.pipeline.decoder.state_dict(),
                "optimizer": self.optimizer.state_dict(), "scheduler": self.scheduler.state_dict(),
                "epoch": self.epoch, "step": self.step_count}

    def load_state_dict(self, state: dict) -> None:
        self.pipeline.encoder.load_state_dict(state["encoder"])
        self.pipeline.decoder.load_state_dict(state["decoder"])
        self.optimizer.load_state_dict(state["optimizer"])
        self.scheduler.load_state_dict(state["scheduler"])
        self.epoch, self.step_count = state["epoch"], state["step"]

    def weights(self) -> dict:
        """the reference's .pth layout"""
        return {"encoder": self.pipeline.encoder.state_dict(), "decoder": self.pipeline.decoder.state_dict()}
