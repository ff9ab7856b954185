"""The training loop (reference pipeline/modules/trainer.py) over `TrainStep` and `EpochLoader`.

`Trainer(args, dataset, model, writer=None)`, `run()`, `train_one_epoch()`, `save(finish=False)`, `load_checkpoint`,
`load_weight`, `init_scratch`, `_next_stage`, `add_module` / `remove_module` are the reference's.  The step itself is
`train_pipeline.TrainStep` (`data_parallel.DataParallelTrainStep` when `args.use_ddp`: the gradient exchange is fused into
the optimiser; `torch.nn.parallel.DistributedDataParallel` is not used), the batches come from `loader.EpochLoader`.

Kept from the reference: `stage_epoch`; the counters (`self.epoch` and `self.step` start at 1, a checkpoint stores `step` as
it stands and resuming continues at `epoch + 1`); the K_0 / K_mult / mult_epoch rule at the start of every registration
epoch; log_interval = max(int((log_cycle / world) // batch_size), 1); the `add_scalar` tags and their step arguments
(`runtime/K` and `runtime/learning_rate` by epoch, `train/step_<metric>` = the mean of the last log_interval steps by
`self.step`, `train/epoch_<metric>` by epoch); `save_cycle`; the files `<name><version>_epoch<E>.ckpt` and
`<name><version>.pth` under `log_train/<log>` in the layouts `TrainStep` produces; the rule that optimiser and scheduler
state are NOT restored when resuming exactly at the stage boundary (trainer.py:289); `settings.yaml`.

Left out: `codes.zip` (the sources are not copied next to the weights), the tqdm progress bars, and `auto_cast=True`, which
raises NotImplementedError: the dense kernels are fp32.  The reference's CUDA_LAUNCH_BLOCKING setting has no
counterpart: no module of this package touches the process environment.

`writer` is any object with `add_scalar(tag, value, step)`; the default is `torch.utils.tensorboard.SummaryWriter` when it
imports, else `JsonlWriter`, one JSON object per line in `log_tb/<log>/scalars.jsonl`.

The loader's settings come from `args.loader` (all optional): `rng` (an int seed, default 42; or 'reference'), `prefetch`
(2; 0 with 'reference'), `streams` (4), `capacity` (131072 rows per frame), `padding_to` (default: the `padding_to` of the
chain's trailing ToTensor, else -1).  The chain is `dataset.data_transforms` without its trailing ToTensor.  A dataset may
bring a loader of its own: `dataset.epoch_loader(stage, batch_size, rank, world)` -> an object with `set_epoch`, `__len__`,
`__iter__` and `close`.
"""
from __future__ import annotations

import json
import logging
import os
import time
from collections import OrderedDict

import torch

from . import augment
from .loader import EpochLoader
from .optim import Recorder, try_load_state_dict
from .train_pipeline import TrainStep

logger = logging.getLogger(__name__)


class JsonlWriter:
    """add_scalar(tag, value, step) -> one line {"tag", "value", "step"} of <log_dir>/scalars.jsonl"""

    def __init__(self, log_dir: str):
        os.makedirs(log_dir, exist_ok=True)
        self.path = os.path.join(log_dir, "scalars.jsonl")
        self._file = open(self.path, "a", encoding="utf-8")

    def add_scalar(self, tag, value, step):
        self._file.write(json.dumps({"tag": tag, "value": float(value), "step": int(step)}) + "\n")
        self._file.flush()

    def close(self):
        self._file.close()


def default_writer(log_dir: str):
    try:
        from torch.utils.tensorboard import SummaryWriter
    except Exception:   # tensorboard is optional
        return JsonlWriter(log_dir)
    return SummaryWriter(log_dir)


def split_chain(transform):
    """dataset.data_transforms -> (the chain without its trailing ToTensor, that ToTensor's padding_to or None)"""
    chain = transform.transforms if isinstance(transform, augment.PointCloudTransforms) else transform
    if isinstance(chain, augment.Compose) and chain.transforms and isinstance(chain.transforms[-1], augment.ToTensor):
        return augment.Compose(chain.transforms[:-1]), chain.transforms[-1].padding_to
    return chain, None


class Trainer:

    def __init__(self, args, dataset, model, writer=None):
        self.args = args
        self.train_cfg = args.train
        self.dataset = dataset
        self.pipeline = model
        self.stage_epoch = (self.train_cfg.registration.num_epochs, self.train_cfg.loop_detection.num_epochs)

        self.train_step = None
        self.dataloader = None
        self.writer = writer
        self.log_interval = None
        self.epoch = 1
        self.step = 1
        if self.train_cfg.get('auto_cast', False):
            raise NotImplementedError('auto_cast=True: the dense kernels are fp32, there is no mixed-precision step')
        self.log = f'{self.args.name}{self.args.version}_config={os.path.split(self.args.yaml_file)[1]}'
        self.save_root = os.path.join('log_train', self.log)
        self.use_ddp = bool(getattr(self.args, 'use_ddp', False))
        self.is_main_process = not (self.use_ddp and self.args.local_rank != 0)
        self.world = int(getattr(self.args, 'word_size', 1)) if self.use_ddp else 1      # `word_size`: the reference's spelling
        self.rank = int(self.args.local_rank) if self.use_ddp else 0

        if args.checkpoint != '':
            self.load_checkpoint(args.checkpoint)
        elif args.weight != '':
            self.load_weight(args.weight)
        else:
            self.init_scratch()

        if self.is_main_process:
            os.makedirs(self.save_root, exist_ok=True)
            logger.info(f'save root = \'{self.save_root}\'')
            items = args._get_kwargs() if hasattr(args, '_get_kwargs') else args.items()
            with open(os.path.join(self.save_root, 'settings.yaml'), 'w+', encoding='utf-8') as arg_file:
                for k, v in sorted(items):
                    arg_file.write(f'{k}: {v}\n')
        s = f'Initialization completed, device = \'{self.args.device}\''
        if self.is_main_process:
            s += ' [MAIN PROCESS]'
        logger.info(s)

    # ---- what the reference keeps as attributes of its own
    @property
    def model(self):
        return self.train_step.model

    @property
    def optimizer(self):
        return self.train_step.optimizer

    @property
    def scheduler(self):
        return self.train_step.scheduler

    def _make_step(self, stage: str):
        self.pipeline.to(self.args.device)
        if self.use_ddp:
            from .data_parallel import DataParallelTrainStep
            return DataParallelTrainStep(self.args, self.pipeline, stage)
        return TrainStep(self.args, self.pipeline, stage)

    def _make_loader(self, stage: str):
        batch_size = self.train_cfg[stage].batch_size
        if hasattr(self.dataset, 'epoch_loader'):
            return self.dataset.epoch_loader(stage, batch_size, self.rank, self.world)
        cfg = self.args.get('loader', {}) if hasattr(self.args, 'get') else getattr(self.args, 'loader', {})
        cfg = cfg or {}
        rng = cfg.get('rng', 42)
        chain, padding_to = split_chain(self.dataset.data_transforms)
        return EpochLoader(self.dataset, chain, stage, batch_size, rng=rng,
                           prefetch=cfg.get('prefetch', 0 if rng == 'reference' else 2), streams=cfg.get('streams', 4),
                           rank=self.rank, world=self.world, capacity=cfg.get('capacity', 131072),
                           padding_to=cfg.get('padding_to', -1 if padding_to is None else padding_to),
                           num_workers=int(getattr(self.args, 'num_workers', 0) or 0), device=self.args.device)

    def _set_loader(self, stage: str):
        if self.dataloader is not None:
            self.dataloader.close()
        getattr(self.dataset, stage)()
        self.dataloader = self._make_loader(stage)

    # ---- the loop
    def run(self):
        self._set_loader('registration' if self.epoch <= self.stage_epoch[0] else 'loop_detection')
        if self.is_main_process:
            if self.writer is None:
                self.writer = default_writer(os.path.join('log_tb', self.log))
            train_record = Recorder()

        try:
            start_epoch = self.epoch
            for ep in range(start_epoch, sum(self.stage_epoch) + 1):
                self._epoch_begin(ep)

                train_metric = self.train_one_epoch()

                self.scheduler.step()

                if self.is_main_process:
                    train_record.add_dict(train_metric)

                    if ep % self.train_cfg.save_cycle == 0:
                        self.save()

                self.epoch += 1
        finally:
            self.dataloader.close()

        if self.is_main_process:
            self.save(finish=True)
            logger.info(train_record.tostring())

    def _epoch_begin(self, ep):
        if ep == self.stage_epoch[0] + 1:
            self._next_stage()

        if ep <= self.stage_epoch[0]:
            registration_cfg = self.train_cfg.registration
            if 'K_0' in registration_cfg.keys():
                K_0 = registration_cfg['K_0']
                K_mult = registration_cfg['K_mult']
                mult_epoch = registration_cfg['mult_epoch']
                times = 0
                for i in mult_epoch:
                    if ep >= i:
                        times += 1
                registration_cfg['K'] = K_0 * (K_mult ** times)
            batch_size = registration_cfg.batch_size
            if self.is_main_process:
                self.writer.add_scalar("runtime/K", registration_cfg['K'], ep)
        else:
            batch_size = self.train_cfg.loop_detection.batch_size

        if self.is_main_process:
            self.writer.add_scalar("runtime/learning_rate", self.optimizer.param_groups[0]['lr'], ep)

        self.dataloader.set_epoch(ep)
        self.train_step.epoch = ep
        log_interval = (self.train_cfg.log_cycle / self.world) // batch_size
        self.log_interval = int(max(log_interval, 1))

    def train_one_epoch(self):
        start_time = time.time()
        self.model.train()
        step_count = 0
        log_interval = self.log_interval
        epoch_metrics = dict()

        for data in self.dataloader:
            step_count += 1
            metric = self.train_step.step(*data)

            if self.is_main_process:
                for metric_name, metric_value in metric.items():
                    epoch_metrics.setdefault(metric_name, []).append(metric_value)

                if step_count % log_interval == 0:
                    for label, metric_list in epoch_metrics.items():
                        self.writer.add_scalar(f"train/step_{label}", sum(metric_list[-log_interval:]) / log_interval,
                                               self.step)
            self.step += 1

        # Epoch ends
        if not self.is_main_process:
            return None

        summary_str = ''
        summary_metric = {}
        for label, metric_list in epoch_metrics.items():
            self.writer.add_scalar(f"train/epoch_{label}", sum(metric_list) / len(metric_list), self.epoch)
            summary_str += f'{label} = {sum(metric_list) / len(metric_list):6.4f} | '
            summary_metric[label] = sum(metric_list) / len(metric_list)

        cost_time = time.time() - start_time
        cost_m, cost_s = divmod(cost_time, 60)
        cost_h, cost_m = divmod(cost_m, 60)
        logger.info(f'Train Epoch {self.epoch:>4d} | ' + summary_str +
                    f'Time = {int(cost_h)}h:{int(cost_m):02d}m:{cost_s:04.1f}s')
        return summary_metric

    def save(self, finish=False):
        if not finish:
            state = self.train_step.state_dict()
            state['epoch'], state['step'] = self.epoch, self.step
            file_path = os.path.join(self.save_root, f'{self.args.name}{self.args.version}_epoch{self.epoch}.ckpt')
        else:
            state = self.train_step.weights()
            file_path = os.path.join(self.save_root, f'{self.args.name}{self.args.version}.pth')
        torch.save(state, file_path)

    def init_scratch(self):
        self.train_step = self._make_step('registration')
        if self.is_main_process:
            logger.info('Training from scratch')

    def load_checkpoint(self, checkpoint: str):
        if not os.path.exists(checkpoint):
            raise FileNotFoundError(f'checkpoint file \'{checkpoint}\' is not found.')
        checkpoint_file_path = checkpoint
        checkpoint = torch.load(checkpoint, map_location=self.args.device, weights_only=False)

        self.epoch = checkpoint['epoch'] + 1
        self.step = checkpoint['step']
        if self.is_main_process:
            logger.info(f"Load epoch, current = {self.epoch}")
            logger.info(f"Load step, current = {self.step}")
        try_load_state_dict(self.pipeline.encoder, checkpoint['encoder'], 'encoder', log=self.is_main_process)
        try_load_state_dict(self.pipeline.decoder, checkpoint['decoder'], 'decoder', log=self.is_main_process)

        self.train_step = self._make_step('registration' if self.epoch <= self.stage_epoch[0] else 'loop_detection')

        if self.epoch != self.stage_epoch[0] + 1:
            try_load_state_dict(self.optimizer, checkpoint['optimizer'], 'optimizer', log=self.is_main_process)
            try_load_state_dict(self.scheduler, checkpoint['scheduler'], 'scheduler', log=self.is_main_process)
        if self.is_main_process:
            logger.info(f'Load checkpoint done. \'{checkpoint_file_path}\'')

    def load_weight(self, weight: str):
        if not os.path.exists(weight):
            raise FileNotFoundError(f'weight file \'{weight}\' is not found.')
        weight_file_path = weight
        weight = torch.load(weight, map_location=self.args.device, weights_only=False)
        try_load_state_dict(self.pipeline.encoder, weight['encoder'], 'encoder', log=self.is_main_process)
        try_load_state_dict(self.pipeline.decoder, weight['decoder'], 'decoder', log=self.is_main_process)
        self.init_scratch()
        if self.is_main_process:
            logger.info(f'Load specific weight from \'{weight_file_path}\'')

    def _next_stage(self):
        self.train_step.next_stage()
        self._set_loader('loop_detection')
        if self.is_main_process:
            logger.info('Convert the training stage from registration to loop-detection')

    @staticmethod
    def add_module(state_dict):
        new_state_dict = OrderedDict()
        for k, v in state_dict.items():
            if not k.startswith('module.'):
                k = 'module.' + k
            new_state_dict[k] = v
        return new_state_dict

    @staticmethod
    def remove_module(state_dict):
        new_state_dict = OrderedDict()
        for k, v in state_dict.items():
            if k.startswith('module.'):
                k = k[7:]
            new_state_dict[k] = v
        return new_state_dict
