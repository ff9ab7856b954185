"""Optimisers, schedulers and the small training utilities of the reference's pipeline/modules/utils.py for the MI355X.

`AdamW`, `Adam` and `SGD` are torch.optim.Optimizer subclasses with torch's keyword arguments, torch's update rule and torch's
state keys (`step`, `exp_avg`, `exp_avg_sq`, `momentum_buffer`), so their state dicts load into torch.optim's classes and back:
a checkpoint of the reference resumes here and one written here resumes there.  What differs is how a step runs:
csrc/optim.hip updates a whole parameter group in ONE launch (torch walks the 110 + 82 tensors of the model one by one, or
in foreach lists).  Two small tables in device memory list the group's tensors and the chunks of the launch grid; they are
rebuilt only when an address changes (a gradient re-allocated after `zero_grad()`, a loaded state dict).  `lr` is read from
`param_groups` on every step, so torch's schedulers drive these classes unchanged.  `step()` never waits for the device: the
step counters are CPU tensors, as in torch's default (non-capturable) optimisers.

Data-parallel training: `attach_grad_sync(sync)` (a `data_parallel.GradSync`) makes `step()` pack the gradients into one flat
buffer, exchange it in one collective and run the same update rule on the rank-ordered mean in the same launch.  Not attached,
nothing changes.

Not supported, `ValueError`: `amsgrad=True`, `maximize=True`, parameters that are not fp32 or not on the GPU, sparse gradients.
`foreach`, `fused`, `capturable` and `differentiable` are accepted and stored for state-dict compatibility; they select nothing.
"""
from __future__ import annotations

import logging
from typing import Dict, List

import numpy as np
import torch

from . import _lib

logger = logging.getLogger(__name__)

ADAMW, ADAM, SGD_ = 0, 1, 2   # include/dpm_hip.h: DPM_OPTIM_*
_MAX_PLANS = 8


def chunk_table(numels, chunk: int) -> np.ndarray:
    """(n_chunks,2) int32 [tensor, chunk]: row k covers elements [chunk * CHUNK, min(numel, (chunk + 1) * CHUNK)) of its tensor"""
    counts = (np.asarray(numels, np.int64) + chunk - 1) // chunk
    which = np.repeat(np.arange(len(counts), dtype=np.int32), counts)
    first = np.cumsum(counts) - counts
    within = (np.arange(int(counts.sum()), dtype=np.int64) - np.repeat(first, counts)).astype(np.int32)
    return np.stack([which, within], axis=1)


def _addr(g) -> int:
    """column 1 of a table row: a gradient's address, or the offset that stands in for it in a synced step"""
    return g if isinstance(g, int) else g.data_ptr()


class _Plan:
    """the two device tables of one launch (and the pinned host copy they were sent from, which must outlive the transfer);
    rows: one list of int64 per tensor, the last entry its numel"""

    def __init__(self, rows: List[List[int]], chunk: int, device):
        tensors = np.asarray(rows, np.int64).reshape(len(rows), -1)
        chunks = chunk_table(tensors[:, -1], chunk)
        self.n_chunks = len(chunks)
        blob = np.concatenate([tensors.reshape(-1).view(np.int32), chunks.reshape(-1)])
        self.host = torch.from_numpy(blob).pin_memory()
        self.dev = self.host.to(device, non_blocking=True)
        self.tensors_ptr = self.dev.data_ptr()
        self.chunks_ptr = self.tensors_ptr + tensors.nbytes


class _GroupStep(torch.optim.Optimizer):
    """shared machinery: collect the tensors of a group that have a gradient, find or build their plan, launch"""

    def __init__(self, params, defaults):
        if defaults.get("amsgrad"):
            raise ValueError("amsgrad=True is not supported by the one-launch optimisers (torch.optim has it)")
        if defaults.get("maximize"):
            raise ValueError("maximize=True is not supported by the one-launch optimisers (torch.optim has it)")
        super().__init__(params, defaults)
        self._plans: Dict[tuple, _Plan] = {}
        self.plan_builds = 0   # how often the device tables were (re)built: only when an address changed
        self._sync = None      # a data_parallel.GradSync: attach_grad_sync()
        for group in self.param_groups:
            for p in group["params"]:
                self._check_param(p)

    @staticmethod
    def _check_param(p):
        if p.dtype != torch.float32:
            raise ValueError(f"parameters must be fp32, got {p.dtype}")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        for p in self.param_groups[-1]["params"]:
            self._check_param(p)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize"):
                raise ValueError("the loaded state dict asks for amsgrad / maximize, which are not supported")
        for st in self.state.values():   # a fused / capturable torch optimiser keeps `step` on the device: bring it home once
            if torch.is_tensor(st.get("step")):
                st["step"] = st["step"].detach().to("cpu", torch.float32)
        self._plans.clear()

    def attach_grad_sync(self, sync) -> None:
        """Data-parallel steps: from now on `step()` packs the local gradients into `sync`'s flat buffer, runs its one collective
        and updates EVERY tensor of its layout from the exchanged buffer in one launch per parameter group -- also a tensor whose
        gradient is None on this rank (it contributes zeros, the other ranks' gradients still move it: all ranks stay identical).
        State keys, step counting, `lr` from `param_groups` and the version bump are those of the plain step.  `p.grad` keeps the
        LOCAL gradient: the average is never written back.  An inert `sync` (no process group, or one rank and no force) leaves
        the plain step in place."""
        ids = {id(p) for group in self.param_groups for p in group["params"]}
        missing = [i for i, p in enumerate(sync.params) if id(p) not in ids]
        if missing:
            raise ValueError(f"{len(missing)} tensors of the GradSync layout are not parameters of this optimiser")
        self._sync = sync
        self._plans.clear()

    def detach_grad_sync(self) -> None:
        self._sync = None
        self._plans.clear()

    def _synced(self) -> bool:
        return self._sync is not None and self._sync.active

    def _items(self, group):
        """(parameter, gradient) of the tensors of `group` that this step updates: those with a gradient -- or, with a grad
        sync attached, (parameter, element offset into a slice) of those the layout holds"""
        for p in group["params"]:
            if self._synced():
                off = self._sync.offset_of(p)
                if off is not None:
                    self._check_device(p)
                    yield p, off
            elif p.grad is not None:
                yield p, self._grad(p)

    @staticmethod
    def _check_device(p):
        if not p.is_cuda:
            raise _lib.DpmError(f"parameters and gradients must be on the GPU, got {p.device} (no CPU fallback)")
        if not p.is_contiguous():
            raise ValueError("parameters must be contiguous (a view at an offset is fine, a strided one is not)")

    def _grad(self, p):
        g = p.grad
        if g.is_sparse:
            raise ValueError("sparse gradients are not supported")
        if not p.is_cuda or not g.is_cuda:
            raise _lib.DpmError(f"parameters and gradients must be on the GPU, got {p.device} (no CPU fallback)")
        if g.dtype != torch.float32:
            raise ValueError(f"gradients must be fp32, got {g.dtype}")
        if not p.is_contiguous():
            raise ValueError("parameters must be contiguous (a view at an offset is fine, a strided one is not)")
        return g if g.is_contiguous() else g.contiguous()

    def _launch(self, algo, params, rows, device, **scalars):
        """rows: [param, grad, state0, state1, numel] per tensor of `params`.  A gradient made contiguous for this call is freed on return;
        the caching allocator hands its memory out again only in stream order, after the kernel."""
        lib = _lib.load()
        key = (self._synced(), *map(tuple, rows))
        plan = self._plans.get(key)
        if plan is None:
            if len(self._plans) >= _MAX_PLANS:
                self._plans.clear()
            plan = self._plans[key] = _Plan(rows, lib.dpm_optim_chunk(), device)
            self.plan_builds += 1
        a = dict(lr=0.0, beta1=0.0, beta2=0.0, eps=0.0, weight_decay=0.0, step=0.0, momentum=0.0, dampening=0.0, nesterov=0,
                 first=0)
        a.update(scalars)
        stream = torch.cuda.current_stream(device)
        common = (algo, plan.tensors_ptr, plan.chunks_ptr, plan.n_chunks, a["lr"], a["beta1"], a["beta2"], a["eps"],
                  a["weight_decay"], a["step"], a["momentum"], a["dampening"], int(a["nesterov"]), int(a["first"]))
        if self._synced():   # rows hold offsets into a slice of the exchanged buffer instead of gradient addresses
            slices, n_slices, stride, divisor = self._sync.slices()
            _lib.check(lib.dpm_optim_step_synced(*common, slices.data_ptr(), n_slices, stride, float(divisor), stream.cuda_stream),
                       "dpm_optim_step_synced")
        else:
            _lib.check(lib.dpm_optim_step(*common, stream.cuda_stream), "dpm_optim_step")
        for p in params:   # an in-place update torch did not see: the derived-weight caches and captured graphs key on this
            torch.autograd.graph.increment_version(p)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._synced():
            self._sync.pack()
            self._sync.exchange()
        for group in self.param_groups:
            self._step_group(group)
        return loss


class Adam(_GroupStep):
    """torch.optim.Adam's arguments, update rule and state dict; one launch per parameter group (csrc/optim.hip)"""

    DECOUPLED = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None):
        if torch.is_tensor(lr):
            raise ValueError("a tensor lr is not supported")
        if lr < 0 or eps < 0 or weight_decay < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1:
            raise ValueError(f"invalid hyper-parameters: lr {lr}, betas {betas}, eps {eps}, weight_decay {weight_decay}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                                      foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused,
                                      decoupled_weight_decay=self.DECOUPLED))

    def _step_group(self, group):
        by_step: Dict[float, list] = {}
        for p, g in self._items(group):
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["step"] += 1
            by_step.setdefault(float(st["step"]), []).append((p, g, st))
        algo = ADAMW if group.get("decoupled_weight_decay", self.DECOUPLED) else ADAM
        for step, items in by_step.items():   # one launch unless earlier steps skipped some tensors (`grad is None`)
            rows = [[p.data_ptr(), _addr(g), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()]
                    for p, g, st in items]
            self._launch(algo, [i[0] for i in items], rows, items[0][0].device, lr=group["lr"], beta1=group["betas"][0],
                         beta2=group["betas"][1], eps=group["eps"], weight_decay=group["weight_decay"],
                         step=step)


class AdamW(Adam):
    """torch.optim.AdamW's arguments (weight_decay defaults to 1e-2, decoupled), update rule and state dict"""

    DECOUPLED = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, maximize=maximize, foreach=foreach, capturable=capturable,
                         differentiable=differentiable, fused=fused)


class SGD(_GroupStep):
    """torch.optim.SGD's arguments (momentum, dampening, nesterov, weight_decay), update rule and state dict"""

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, *, maximize=False,
                 foreach=None, differentiable=False, fused=None):
        if torch.is_tensor(lr):
            raise ValueError("a tensor lr is not supported")
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError(f"invalid hyper-parameters: lr {lr}, momentum {momentum}, weight_decay {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                      maximize=maximize, foreach=foreach, differentiable=differentiable, fused=fused))

    def _step_group(self, group):
        old, new = [], []
        for p, g in self._items(group):
            buf = None
            if group["momentum"] != 0:
                st = self.state[p]
                buf = st.get("momentum_buffer")
                if buf is None:
                    buf = st["momentum_buffer"] = torch.empty_like(p, memory_format=torch.preserve_format)
                    new.append((p, g, buf))
                    continue
            old.append((p, g, buf))
        for first, items in ((1, new), (0, old)):
            if not items:
                continue
            rows = [[p.data_ptr(), _addr(g), 0 if buf is None else buf.data_ptr(), 0, p.numel()]
                    for p, g, buf in items]
            self._launch(SGD_, [i[0] for i in items], rows, items[0][0].device, lr=group["lr"],
                         weight_decay=group["weight_decay"], momentum=group["momentum"], dampening=group["dampening"],
                         nesterov=group["nesterov"], first=first)


# ---- the reference's factories (pipeline/modules/utils.py:86-125) over these classes and torch's schedulers ------------------
class Optimizer:
    """Optimizer(args)(parameters): args.type in adamw | adam | sgd (any case), args.kwargs the constructor's keywords"""

    def __init__(self, args):
        self.name = args.type.lower()
        self.kwargs = args.kwargs
        try:
            self.optimizer = {"adamw": AdamW, "adam": Adam, "sgd": SGD}[self.name]
        except KeyError:
            raise NotImplementedError(f"optimizer type {args.type!r}") from None

    def __call__(self, parameters):
        return self.optimizer(parameters, **self.kwargs)


class IdentityScheduler(torch.nn.Module):
    def __init__(self, *args, **kwargs):
        super().__init__()

    def step(self):
        pass


class Scheduler:
    """Scheduler(args)(optimizer): args.type in identity | cosine | cosine_restart (any case)"""

    def __init__(self, args):
        self.name = args.type.lower()
        self.kwargs = args.kwargs
        try:
            self.scheduler = {"identity": IdentityScheduler, "cosine": torch.optim.lr_scheduler.CosineAnnealingLR,
                              "cosine_restart": torch.optim.lr_scheduler.CosineAnnealingWarmRestarts}[self.name]
        except KeyError:
            raise NotImplementedError(f"scheduler type {args.type!r}") from None

    def __call__(self, optimizer):
        return self.scheduler(optimizer=optimizer, **self.kwargs)


class Recorder:
    """metric lists by key with the reference's reductions (min | max | mean | best | none) and `tostring`"""

    def __init__(self):
        self.record_dict: Dict[str, list] = {}
        self.reduction_func = {"min": self.min, "max": self.max, "mean": self.mean, "best": self.best,
                               "none": lambda: self.record_dict}

    def add_dict(self, metric_dict: dict):
        for key, value in metric_dict.items():
            self.add_item(key, value)

    def add_item(self, key: str, value):
        self.record_dict.setdefault(key, []).append(value)

    def _reduce(self, fn) -> dict:
        return {k: fn(v) for k, v in self.record_dict.items() if len(v) > 0}

    def mean(self) -> dict:
        return self._reduce(lambda v: sum(v) / len(v))

    def max(self) -> dict:
        return self._reduce(max)

    def min(self) -> dict:
        return self._reduce(min)

    def best(self) -> dict:
        """per key the minimum if the series went down from its first to its last value, else the maximum"""
        return self._reduce(lambda v: min(v) if v[0] > v[-1] else max(v))

    def tostring(self, reduction="best") -> str:
        assert reduction in self.reduction_func
        lines = [f"\t{k:<20s}: ({v if isinstance(v, list) else format(v, '4.5f')})\n" for k, v in self.reduction_func[reduction]().items()]
        return "\n" + "".join(lines) if lines else ""

    def clear(self):
        self.record_dict.clear()


def try_load_state_dict(model, state_dict, name="model", log=True):
    """load_state_dict that reports instead of raising: strict when the key sets agree, otherwise non-strict with the missing
    and unexpected keys in a warning; any failure of the load itself is a warning too (the reference's behaviour)"""
    model_keys, file_keys = model.state_dict().keys(), state_dict.keys()
    say = (lambda level, msg: logger.log(level, msg)) if log else (lambda level, msg: None)
    same = model_keys == file_keys
    try:
        model.load_state_dict(state_dict) if same else model.load_state_dict(state_dict, strict=False)
    except Exception:
        say(logging.WARNING, f"{name} loaded failed.")
        return
    if same:
        say(logging.INFO, f"{name} loaded successfully.")
        return
    missing, unexpected = model_keys - file_keys, file_keys - model_keys
    msg = f"{name} loaded with {len(model_keys)} in model, {len(file_keys)} in file.\n"
    if missing:
        msg += f"{len(missing)} missing parameters (in model):\n" + ", ".join(sorted(missing)) + "\n"
    if unexpected:
        msg += f"{len(unexpected)} unexpected parameters (in file):\n" + ", ".join(sorted(unexpected)) + "\n"
    say(logging.WARNING, msg)
