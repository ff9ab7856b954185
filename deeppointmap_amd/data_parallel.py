"""Data-parallel training over a torch.distributed process group: what the reference gets from wrapping its model in
`torch.nn.parallel.DistributedDataParallel` (pipeline/modules/trainer.py:239-243, 280-284, 316-321), rebuilt in the optimiser's
table-driven, one-launch style.

After `backward()` a step has three parts:
  pack       ONE launch copies every trainable gradient of the stage into one flat fp32 buffer (`dpm_flat_pack`); each tensor at
             a fixed offset that is a multiple of 4 elements, padding zero, a gradient that is None on this rank zeros -- every
             rank always enters the same collective with the same layout;
  exchange   ONE collective on that buffer: `mode="ordered"` all-gathers it into a (W, L) buffer, `mode="allreduce"` sums it in
             place.  Over RCCL nothing synchronises the host; under gloo (the dry-run backend) the buffer goes through the host;
  update     ONE launch per parameter group (`dpm_optim_step_synced`): g = slice_0[i]; g = g + slice_r[i] for r = 1 .. W - 1 in
             rank order; g = g / W; then the AdamW / Adam / SGD element rule of csrc/optim.hip, the same code.

In ordered mode the averaged gradient is the same bytes on every rank, on every run and for every topology, so all ranks hold
bit-identical parameters for ever; the price is W - 1 received slices per rank where an all-reduce moves 2 (W - 1) / W.  Neither
mode reproduces torch DDP's bytes (its bucketed ring all-reduce fixes neither the order of the sum nor its independence of the
topology), and neither tries to.  After a step `p.grad` still holds the LOCAL gradient: the average is not written back.

Not here: overlap of the exchange with the backward (buckets, gradient hooks), a DistributedSampler (torch's works unchanged),
bf16.  Nothing between two devices has been run: the GPU tests fold two ranks onto one GPU over gloo and run RCCL on one rank.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Tuple

import torch
import torch.distributed as dist
from torch import nn

from . import _lib
from .optim import _MAX_PLANS, _Plan
from .train_pipeline import DeepPointModelPipeline, TrainStep

__all__ = ["flat_layout", "GradSync", "DataParallel", "DataParallelTrainStep", "MODES"]

MODES = ("ordered", "allreduce")


def flat_layout(numels: Iterable[int]) -> Tuple[List[int], int]:
    """offsets, L: tensor k occupies [offsets[k], offsets[k] + numels[k]) of the flat buffer; every offset and L are multiples
    of 4 elements (16 bytes: an aligned tensor moves as float4), the up to 3 elements behind a tensor are padding"""
    offsets, at = [], 0
    for n in numels:
        offsets.append(at)
        at += (int(n) + 3) // 4 * 4
    return offsets, at


class GradSync:
    """The flat gradient buffer of a set of parameters and its exchange.  `params`: the `requires_grad` ones, in iteration
    order, form the layout (`trainable_only=False`: all of them -- the broadcast of a whole model).  Inert -- `active` False,
    `pack()` and `exchange()` do nothing -- without a process group (`process_group` None and torch.distributed not
    initialised) or with one rank, unless `force=True` issues the collective anyway (the only way to execute the RCCL call path
    on one GPU).  `plan_builds` counts how often the device tables were (re)built: only when an address changed."""

    def __init__(self, params, process_group=None, mode: str = "ordered", force: bool = False, trainable_only: bool = True):
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        self.mode = mode
        self.params = [p for p in params if p.requires_grad or not trainable_only]
        for p in self.params:
            if p.dtype != torch.float32:
                raise ValueError(f"parameters must be fp32, got {p.dtype}")
        self.numels = [p.numel() for p in self.params]
        self.offsets, self.length = flat_layout(self.numels)
        self._offset = {id(p): o for p, o in zip(self.params, self.offsets)}
        if process_group is None and dist.is_available() and dist.is_initialized():
            process_group = dist.group.WORLD
        self.group = process_group
        self.world = dist.get_world_size(process_group) if process_group is not None else 1
        self.rank = dist.get_rank(process_group) if process_group is not None else 0
        self.active = process_group is not None and (self.world > 1 or force) and len(self.params) > 0
        self.plan_builds = 0
        self._plans: Dict[tuple, _Plan] = {}
        self.flat: Optional[torch.Tensor] = None
        self.gathered: Optional[torch.Tensor] = None

    def offset_of(self, p) -> Optional[int]:
        """element offset of parameter `p` in a slice, None if the layout does not hold it"""
        return self._offset.get(id(p))

    # ---- buffers and tables ----------------------------------------------------------------------------------------------
    def _buffers(self) -> torch.Tensor:
        if self.flat is None:
            dev = self.params[0].device
            if dev.type != "cuda":
                raise _lib.DpmError(f"parameters and gradients must be on the GPU, got {dev} (no CPU fallback)")
            self.flat = torch.zeros(self.length, dtype=torch.float32, device=dev)
            if self.mode == "ordered":
                self.gathered = torch.zeros(self.world, self.length, dtype=torch.float32, device=dev)
        return self.flat

    def _plan(self, addresses: List[int]) -> _Plan:
        key = tuple(addresses)
        plan = self._plans.get(key)
        if plan is None:
            if len(self._plans) >= _MAX_PLANS:
                self._plans.clear()
            rows = [[a, o, n] for a, o, n in zip(addresses, self.offsets, self.numels)]
            plan = self._plans[key] = _Plan(rows, _lib.load().dpm_optim_chunk(), self.flat.device)
            self.plan_builds += 1
        return plan

    def _copy(self, tensors: list, unpack: bool) -> None:
        """tensors: per layout entry an fp32 GPU tensor or None (pack: zeros; unpack: skipped)"""
        flat, lib = self._buffers(), _lib.load()
        keep = []   # a tensor made contiguous for this call: freed on return, handed out again only in stream order
        for t, n in zip(tensors, self.numels):
            if t is None:
                keep.append(None)
                continue
            if t.device != flat.device or t.dtype != torch.float32 or t.is_sparse or t.numel() != n:
                raise ValueError(f"expected a dense fp32 tensor of {n} elements on {flat.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
            if not t.is_contiguous():
                if unpack:
                    raise ValueError("parameters must be contiguous (a view at an offset is fine, a strided one is not)")
                t = t.contiguous()
            keep.append(t)
        plan = self._plan([0 if t is None else t.data_ptr() for t in keep])
        fn, what = (lib.dpm_flat_unpack, "dpm_flat_unpack") if unpack else (lib.dpm_flat_pack, "dpm_flat_pack")
        stream = torch.cuda.current_stream(flat.device)
        _lib.check(fn(plan.tensors_ptr, plan.chunks_ptr, plan.n_chunks, flat.data_ptr(), self.length, stream.cuda_stream), what)

    def _through_host(self) -> bool:
        return dist.get_backend(self.group) == "gloo"   # the dry-run backend moves host tensors only (shard.py does the same)

    # ---- the step --------------------------------------------------------------------------------------------------------
    def pack(self) -> None:
        """every gradient into the flat buffer in one launch; a gradient that is None contributes zeros"""
        if self.active:
            self._copy([p.grad for p in self.params], unpack=False)

    def exchange(self) -> None:
        """the step's one collective on the flat buffer, on the current stream's behalf: all_gather_into_tensor (ordered) or
        all_reduce(SUM) in place (allreduce)"""
        if not self.active:
            return
        flat = self._buffers()
        if self._through_host():
            host = flat.cpu()
            if self.mode == "ordered":
                out = torch.empty(self.world, self.length, dtype=torch.float32)
                dist.all_gather(list(out.unbind(0)), host, group=self.group)
                self.gathered.copy_(out)
            else:
                dist.all_reduce(host, op=dist.ReduceOp.SUM, group=self.group)
                flat.copy_(host)
        elif self.mode == "ordered":
            dist.all_gather_into_tensor(self.gathered, flat, group=self.group)
        else:
            dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group)

    def slices(self) -> Tuple[torch.Tensor, int, int, float]:
        """(buffer, n_slices, slice_stride, divisor) of dpm_optim_step_synced after `exchange()`"""
        self._buffers()
        if self.mode == "ordered":
            return self.gathered, self.world, self.length, float(self.world)
        return self.flat, 1, self.length, float(self.world)

    def broadcast_parameters(self, src: int = 0) -> None:
        """every rank takes rank `src`'s values of the layout's tensors: pack -> broadcast -> unpack (`src`: rank in the group)"""
        if not self.active:
            return
        with torch.no_grad():
            values = [p.data for p in self.params]
            self._copy(values, unpack=False)
            flat, root = self.flat, dist.get_global_rank(self.group, src)
            if self._through_host():
                host = flat.cpu()
                dist.broadcast(host, src=root, group=self.group)
                flat.copy_(host)
            else:
                dist.broadcast(flat, src=root, group=self.group)
            self._copy(values, unpack=True)
            for p in self.params:   # an in-place update torch did not see (optim.py does the same)
                torch.autograd.graph.increment_version(p)


class DataParallel(nn.Module):
    """`DistributedDataParallel`'s place in the reference's trainer: an nn.Module that holds the model as `.module` (state-dict
    keys carry the `module.` prefix, `self.model.module.encoder.state_dict()` works) and forwards every call to it.
    Construction makes every rank start from rank 0's parameters.  The gradients are NOT exchanged by the backward: the
    optimiser does it (`optim.AdamW.attach_grad_sync(GradSync(...))`; `DataParallelTrainStep` wires it up)."""

    def __init__(self, module: nn.Module, process_group=None, mode: str = "ordered", force: bool = False):
        super().__init__()
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        self.module = module
        self.process_group, self.mode, self.force = process_group, mode, force
        GradSync(module.parameters(), process_group, mode, force, trainable_only=False).broadcast_parameters(0)

    def forward(self, *args, **kwargs):
        return self.module(*args, **kwargs)

    def grad_sync(self) -> GradSync:
        """a GradSync over the parameters that require a gradient NOW (a stage change needs a new one)"""
        return GradSync(self.module.parameters(), self.process_group, self.mode, self.force)


class DataParallelTrainStep(TrainStep):
    """`TrainStep` under a process group: the model wrapped in `DataParallel`, and per stage the optimiser with a `GradSync`
    over the same parameters attached -- so `step()` is forward, zero_grad, backward and the synced optimiser step.  The
    metrics returned are this rank's own (the reference logs rank 0's); `state_dict()` / `weights()` are the reference's
    layout, taken from `.module`, and load into a plain `TrainStep` and back."""

    def __init__(self, args, model, stage: str = "registration", process_group=None, mode: str = "ordered", force: bool = False):
        if not isinstance(model, DataParallel):
            model = DataParallel(model, process_group, mode, force)
        self.sync: Optional[GradSync] = None
        super().__init__(args, model, stage)

    @property
    def pipeline(self) -> DeepPointModelPipeline:
        return self.model.module

    def _enter(self, stage: str) -> None:
        super()._enter(stage)   # the stage's requires_grad flags, then the optimiser over the parameters it trains
        self.sync = self.model.grad_sync()
        self.optimizer.attach_grad_sync(self.sync)

    @property
    def is_main_process(self) -> bool:
        return self.sync.rank == 0

