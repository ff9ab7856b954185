"""The batch loader of training: dataset plans -> file reads -> one staging block -> frames on the GPU -> the transforms ->
the batch `DeepPointModelPipeline.forward` takes.  Stands where the reference puts `torch.utils.data.DataLoader`
(pipeline/modules/trainer.py:87-95), whose workers run the transforms on the CPU in child processes; here the transforms
are HIP kernels on frames whose length lives in device memory, so they run in the training process: one background THREAD
reads ahead and queues a batch's device work on a stream of its own while the current step runs.  No child processes.

Per batch the device sees ONE copy of the pinned staging block and three launches (ops.ingest_frames), then the chain
(augment.transform_frames, without its ToTensor) and the packing (augment.collate_frames, whose read-back is the one host
synchronisation, in the loader's thread).  An event is recorded on the loader's stream and handed over with the batch;
the consumer's stream waits on it, and every tensor of the batch is `record_stream`ed on the consumer's stream.

Index order: torch's own samplers (RandomSampler / DistributedSampler + BatchSampler(drop_last=True)); an epoch has
len(dataset) // batch_size steps (per rank when world > 1).

REGISTRATION keeps only the first item of a batch: the reference's `map_collate_fn` (dataloader/body.py:155-161) builds all
`batch_size` items and throws all but `batch[0]` away; this loader builds only the kept one.  Consequence: the discarded
items' draws are not made, so a run seeded like the reference replays it only at batch_size = 1 with num_workers = 0.
LOOP DETECTION yields the reference's ten tensors, one pair per item.

Two random modes:

* rng="reference": Python's global `random`, torch's default generator (the DataLoader's base seed and the sampler's seed
  are drawn from it as `DataLoader(shuffle=True)` draws them) and DrawSource("reference").  Synchronous -- the draws
  interleave with the step's `draw_s1` as in a num_workers=0 reference run --, so it requires prefetch=0.
* rng=<int seed>: every generator is private and a function of (seed, epoch, rank): a `random.Random` for the dataset
  draws (and for `s1`, which the loader draws itself and appends to the registration batch, so that the step consumes no
  global random state), a `torch.Generator(device="cuda")` for the transforms, a torch CPU generator for the sampler.
  The bytes of every batch are then a function of (seed, epoch, position in the epoch) only, whatever `prefetch`, timing
  or thread scheduling.

Failures never hang: every blocking wait has a timeout and raises RuntimeError when it expires, an exception in the
loader's thread is re-raised by the consumer's `next()`, `close()` / `__exit__` stop and join the thread.
"""
from __future__ import annotations

import queue
import random as _pyrandom
import threading
import time
from concurrent.futures import ThreadPoolExecutor
from typing import List

import torch
from torch.utils.data import BatchSampler, RandomSampler, SequentialSampler
from torch.utils.data.distributed import DistributedSampler

from . import augment, ops
from .train_pipeline import draw_s1

STAGES = ("registration", "loop_detection")
_MASK = (1 << 62) - 1


def derive_seed(seed: int, epoch: int, rank: int, salt: int) -> int:
    """the private generators' seeds: a fixed mix of (seed, epoch, rank) per use (salt)"""
    x = (int(seed) * 0x9E3779B97F4A7C15 + int(epoch) * 0xBF58476D1CE4E5B9 + int(rank) * 0x94D049BB133111EB + salt * 0xD6E8FEB86659FD93)
    x ^= x >> 31
    return x & _MASK


def sampler_seed(seed: int) -> int:
    """the base seed of the index order of a seeded loader (the epoch is added to it, as DistributedSampler adds it)"""
    return derive_seed(seed, 0, 0, 3) & 0x7FFFFFFF


def epoch_indices(n: int, batch_size: int, epoch: int, seed=None, rank: int = 0, world: int = 1, shuffle: bool = True) -> List[List[int]]:
    """the batches of one epoch as torch's samplers give them.  seed None = the reference mode: world 1 draws the
    permutation's seed from torch's default generator (RandomSampler), world > 1 is DistributedSampler(seed=0) after
    set_epoch(epoch), as the reference builds it.  A seeded loader permutes with generator seed sampler_seed(seed) + epoch
    in both cases (at world 1 the same permutation DistributedSampler(num_replicas=1) makes)."""
    source = range(int(n))
    if world > 1:
        sampler = DistributedSampler(source, num_replicas=world, rank=rank, shuffle=shuffle,
                                     seed=0 if seed is None else sampler_seed(seed))
        sampler.set_epoch(epoch)
    elif not shuffle:
        sampler = SequentialSampler(source)
    elif seed is None:
        sampler = RandomSampler(source)
    else:
        sampler = RandomSampler(source, generator=torch.Generator().manual_seed(sampler_seed(seed) + int(epoch)))
    return [list(b) for b in BatchSampler(sampler, batch_size=int(batch_size), drop_last=True)]


class _Slot:
    """a pinned staging block and the event of its last copy"""

    def __init__(self):
        self.block = None
        self.event = None

    def take(self, nbytes, timeout):
        if self.event is not None:          # reused only after its copy has completed
            deadline = time.monotonic() + timeout
            while not self.event.query():
                if time.monotonic() > deadline:
                    raise RuntimeError(f"the copy of a staging slot did not complete within {timeout} s")
                time.sleep(0.0002)
            self.event = None
        if self.block is None or self.block.numel() < nbytes:
            self.block = torch.empty(int(nbytes * 1.25) + 64, dtype=torch.uint8, pin_memory=True)
        return self.block


class _ReadAhead:
    """What EpochLoader and SceneLoader share: the background thread that builds work units ahead on a stream of its own,
    the bounded queue and the event hand-over to the consumer's stream, the pinned staging slots, the thread pool of the
    file readers, and the failure handling (every wait has a timeout, an exception of the thread is re-raised by next(),
    close() stops and joins).  A subclass gives `_build(unit, slot)` and starts an iteration with `_start(units)`."""

    def __init__(self, prefetch, num_workers, timeout, device):
        self.prefetch, self.timeout = int(prefetch), float(timeout)
        self._device = None if device is None else torch.device(device)     # None: the current device at first use
        self._workers = min(int(num_workers), 16)
        self._pool = ThreadPoolExecutor(max_workers=min(int(num_workers), 16)) if num_workers > 0 else None
        self._slots = [_Slot() for _ in range(max(self.prefetch, 1))]
        self._stream = None
        self._thread = None
        self._stop = threading.Event()
        self._queue = None
        self._batches = None
        self._pos = 0

    @property
    def device(self):
        if self._device is None:
            self._device = torch.device("cuda", torch.cuda.current_device())
        return self._device

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _start(self, units):
        self._batches = units
        self._pos = 0
        if self.prefetch > 0:
            if self._stream is None:
                self._stream = torch.cuda.Stream(device=self.device)
            self._stop = threading.Event()
            self._queue = queue.Queue(maxsize=self.prefetch)
            self._thread = threading.Thread(target=self._run, args=(self._batches, self._queue, self._stop),
                                            name="deeppointmap-loader", daemon=True)
            self._thread.start()
        return self

    def _next_unit(self):
        """the next built unit; its tensors are safe to use on the consumer's current stream"""
        if self._batches is None:
            raise RuntimeError("iterate the loader (iter(loader)) before calling next()")
        if self.prefetch == 0:
            if self._pos >= len(self._batches):
                raise StopIteration
            with torch.cuda.device(self.device):
                batch = self._build(self._batches[self._pos], self._slots[0])
            self._pos += 1
            return batch
        deadline = time.monotonic() + self.timeout
        while True:
            try:
                kind, payload, event = self._queue.get(timeout=0.05)
                break
            except queue.Empty:
                if not self._thread.is_alive() and self._queue.empty():
                    raise RuntimeError("the loader thread ended without handing over a batch") from None
                if time.monotonic() > deadline:
                    raise RuntimeError(f"no batch arrived within {self.timeout} s") from None
        if kind == "end":
            self._join()
            raise StopIteration
        if kind == "error":
            self._join()
            raise payload
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(event)
        for t in self._tensors(payload):
            t.record_stream(cur)
        return payload

    @staticmethod
    def _tensors(payload):
        for t in payload:
            if isinstance(t, torch.Tensor):
                if t.is_cuda:
                    yield t
            elif isinstance(t, (list, tuple)):
                yield from _ReadAhead._tensors(t)

    # ---- the loader's thread
    def _run(self, batches, q, stop):
        def put(item):
            deadline = time.monotonic() + self.timeout
            while not stop.is_set():
                try:
                    q.put(item, timeout=0.05)
                    return True
                except queue.Full:
                    if time.monotonic() > deadline:
                        raise RuntimeError(f"the consumer took no batch within {self.timeout} s") from None
            return False
        try:
            with torch.cuda.device(self.device), torch.cuda.stream(self._stream):
                for k, indices in enumerate(batches):
                    if stop.is_set():
                        return
                    batch = self._build(indices, self._slots[k % len(self._slots)])
                    event = torch.cuda.Event()
                    event.record(self._stream)
                    if not put(("batch", batch, event)):
                        return
            put(("end", None, None))
        except BaseException as e:   # handed to the consumer, which re-raises it
            try:
                put(("error", e, None))
            except RuntimeError:
                pass

    def _halt(self):
        if self._thread is not None:
            self._stop.set()
            self._join()

    def _join(self):
        t, self._thread = self._thread, None
        if t is not None:
            t.join(self.timeout)
            if t.is_alive():
                raise RuntimeError(f"the loader thread did not end within {self.timeout} s")

    def close(self):
        """stop and join the loader's thread and the file readers"""
        self._halt()
        self._batches = None
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None

    def _map(self, fn, keys):
        """fn over keys, in order, on the readers' thread pool when there is one"""
        if self._pool is None:
            return [fn(k) for k in keys]
        return list(self._pool.map(fn, keys, timeout=self.timeout))

    def _ingest(self, raws, names, slot, capacity):
        """raws: per frame (rows, stride, R, T, drop_nan) -> stage into the pinned slot, one copy, ops.ingest_frames on the
        current stream: xyz (F,capacity,3), idx (F,capacity), count (F,).  A frame with more records than the capacity
        raises ValueError (naming it) before anything is queued."""
        for (rows, *_), name in zip(raws, names):
            if rows.shape[0] > capacity:
                raise ValueError(f"frame {name} has {rows.shape[0]} records, more than the capacity {capacity}")
        _, nbytes = ops.ingest_layout([r[0].shape for r in raws])
        block = ops.ingest_stage([(r[0], r[4]) for r in raws], block=slot.take(nbytes, self.timeout))
        xyz, idx, count = ops.ingest_frames(block, len(raws), capacity, device=self.device)
        slot.event = torch.cuda.Event()
        slot.event.record(torch.cuda.current_stream(self.device))
        return xyz, idx, count


class EpochLoader(_ReadAhead):
    """for ep in epochs: loader.set_epoch(ep); for batch in loader: step(*batch)      (module docstring)

    dataset: dataset.SlamDatasets; transform: the chain WITHOUT its ToTensor; stage: 'registration' | 'loop_detection';
    capacity: rows of every frame's buffer (a file with more records raises ValueError before anything is queued);
    padding_to: the ToTensor padding (-1: the longest frame of the batch); num_workers: threads that read files (at most
    16; 0 reads in the loader's thread); timeout: seconds any single wait may take."""

    def __init__(self, dataset, transform, stage, batch_size, *, rng, prefetch=2, streams=4, rank=0, world=1, shuffle=True,
                 capacity, padding_to, num_workers=0, timeout=300.0, device=None):
        if stage not in STAGES:
            raise ValueError(f"stage must be one of {STAGES}, got {stage!r}")
        self.reference = isinstance(rng, str)
        if self.reference and rng != "reference":
            raise ValueError("rng is 'reference' or an int seed")
        if not self.reference and (isinstance(rng, bool) or not isinstance(rng, int)):
            raise ValueError("rng is 'reference' or an int seed")
        if self.reference and prefetch != 0:
            raise ValueError("rng='reference' draws from the global generators in step order: it requires prefetch=0")
        if prefetch < 0 or batch_size < 1 or capacity < 1:
            raise ValueError("prefetch >= 0, batch_size >= 1, capacity >= 1")
        _ReadAhead.__init__(self, prefetch, num_workers, timeout, device)
        self._device = self.device      # resolved here: the device current when the loader is made
        self.dataset, self.transform, self.stage, self.batch_size = dataset, transform, stage, int(batch_size)
        self.seed = None if self.reference else int(rng)
        self.streams, self.rank, self.world, self.shuffle = int(streams), int(rank), int(world), shuffle
        self.capacity, self.padding_to = int(capacity), int(padding_to)
        self.epoch = 1
        self._py = self._gen = None
        n = len(dataset)
        self._steps = (n if world == 1 else -(-n // world)) // self.batch_size

    # ---- the epoch
    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def __len__(self) -> int:
        return self._steps

    def __iter__(self):
        self._halt()
        getattr(self.dataset, self.stage)()
        if self.reference:
            # DataLoader.__iter__ draws its base seed from the default generator before the sampler draws its own
            torch.empty((), dtype=torch.int64).random_()
            self._py, self._gen = _pyrandom, "reference"
        else:
            self._py = _pyrandom.Random(derive_seed(self.seed, self.epoch, self.rank, 1))
            self._gen = torch.Generator(device=self.device).manual_seed(derive_seed(self.seed, self.epoch, self.rank, 2))
        return self._start(epoch_indices(len(self.dataset), self.batch_size, self.epoch, self.seed, self.rank, self.world,
                                         self.shuffle))

    def __next__(self):
        return self._next_unit()

    # ---- one batch
    def _read(self, keys):
        """keys: (dataset, scene, frame) -> per frame (rows, stride, R, T, drop_nan)"""
        def one(key):
            d, s, f = key
            return self.dataset.dataset_list[d].scene_list[s].read_raw(f)
        return self._map(one, keys)

    def _frames(self, keys, slot):
        """read, stage, copy, ingest -> the frames of the batch, every one of capacity `capacity`"""
        raws = self._read(keys)
        xyz, idx, count = self._ingest(raws, keys, slot, self.capacity)
        return [augment.PointCloud.from_buffers(xyz[f], idx[f], count[f:f + 1], R, T, host_n=None if drop else rows.shape[0])
                for f, (rows, _, R, T, drop) in enumerate(raws)]

    def _build(self, indices, slot):
        if self.stage == "registration":
            plan = self.dataset.plan_registration(indices[0], rng=self._py)
            keys = [(d, s, f) for d, s, f, _ in plan["frames"]]
        else:
            plans = [self.dataset.plan_loop_detection(i, rng=self._py) for i in indices]
            keys = []
            for p in plans:
                ds = self.dataset.dataset_list[p["dataset_id"]]
                for item in p["items"]:
                    scene_id, offset = ds.get_frame_order(item)
                    keys.append((p["dataset_id"], scene_id, offset))
        frames = self._frames(keys, slot)
        frames = augment.transform_frames(frames, self.transform, streams=self.streams, rng=self._gen)
        pcd, R, T, padding, calib = augment.collate_frames(frames, self.padding_to)
        if self.stage == "registration":
            if self.reference:
                return pcd, R, T, padding, calib, plan["info"]
            s1 = draw_s1(plan["S"], self.dataset.args.train.registration.map_size_max, rng=self._py)
            return pcd, R, T, padding, calib, plan["info"], s1
        src, dst = slice(0, None, 2), slice(1, None, 2)
        return tuple(t[half].contiguous() for half in (src, dst) for t in (pcd, R, T, padding, calib))


# ------------------------------------------------------------------------------------------------------------
# inference: the frames of one scene, in file order
# ------------------------------------------------------------------------------------------------------------
def scene_groups(n: int, group: int) -> List[List[int]]:
    """the frames 0..n-1 in consecutive groups of `group`; the last one may be short"""
    if n < 0 or group < 1:
        raise ValueError("n >= 0, group >= 1")
    return [list(range(a, min(a + group, n))) for a in range(0, n, group)]


def split_chain(transform):
    """PointCloudTransforms / Compose -> (the chain without its ToTensor, that ToTensor's padding_to or -1)"""
    chain = getattr(transform, "transforms", None)
    if isinstance(chain, augment.Compose):      # PointCloudTransforms holds the Compose
        chain = chain.transforms
    if not isinstance(chain, (list, tuple)):
        raise ValueError("transform is an augment.PointCloudTransforms or an augment.Compose")
    body = [t for t in chain if not isinstance(t, augment.ToTensor)]
    heads = [t for t in chain if isinstance(t, augment.ToTensor)]
    if len(heads) > 1 or (heads and chain[-1] is not heads[0]):
        raise ValueError("ToTensor may only end the chain")
    if heads and heads[0].use_calib:
        raise ValueError("the inference item carries no calib: ToTensor(use_calib=True) is a training setting")
    return augment.Compose(body), (int(heads[0].padding_to) if heads else -1)


class SceneLoader(_ReadAhead):
    """for pcd, R, T, padding, original in SceneLoader(agent, PointCloudTransforms(args, mode='infer')): system.step(...)

    Stands where the reference's infer.py puts DataLoader(agent.set_independent(transforms), batch_size=1, shuffle=False,
    num_workers=8) (pipeline/infer.py:85-98).  `agent`: a dataset.BasicAgent, whose file_list is the frame order.
    `transform`: the inference chain; it runs without its ToTensor, whose padding_to decides P (-1: every frame keeps its
    own length).  A background thread reads `group` consecutive frames ahead (readers' read_raw on a pool of at most 16
    threads), stages them into one pinned slot and queues ops.ingest_frames, augment.transform_frames and the packing on
    a stream of its own; every length of the group -- the ingest counts `original` needs and every deferred error flag
    with them -- comes back in ONE host synchronisation.  Items are yielded frame by frame, each what the reference's loop
    receives: [points (1,3,P), R (1,3,3), T (1,3,1), padding (1,P) bool, original (1,N,3)], on the GPU; `original` is the
    frame as read, after the reader's NaN filter.  The consumer's stream waits on the group's event.  The bytes of frame i
    do not depend on group, prefetch, streams or timing.

    capacity: rows of every frame's buffer; None = the largest record count of the group (known from the staging headers
    before anything is queued); a file with more records than a fixed capacity raises ValueError naming it.  prefetch 0
    builds each group in the caller's thread.  A reader's exception is re-raised by next() with the file's name."""

    def __init__(self, agent, transform, *, group=4, prefetch=2, streams=4, capacity=None, device=None, timeout=300.0):
        if isinstance(group, bool) or not isinstance(group, int) or group < 1:
            raise ValueError("group is an int >= 1")
        if isinstance(prefetch, bool) or not isinstance(prefetch, int) or prefetch < 0:
            raise ValueError("prefetch is an int >= 0")
        if not isinstance(streams, int) or streams < 1:
            raise ValueError("streams is an int >= 1")
        if capacity is not None and (not isinstance(capacity, int) or capacity < 1):
            raise ValueError("capacity is None or an int >= 1")
        if not timeout > 0:
            raise ValueError("timeout > 0")
        if not hasattr(agent, "file_list") or not hasattr(agent, "reader"):
            raise ValueError("agent is a dataset.BasicAgent (file_list, reader)")
        self.chain, self.padding_to = split_chain(transform)
        _ReadAhead.__init__(self, prefetch, min(group, 16), timeout, device)    # touches no device
        self.agent, self.group, self.streams, self.capacity = agent, group, streams, capacity
        self.files = list(agent.file_list)
        self.groups = scene_groups(len(self.files), group)
        self._pending, self._done = [], False

    def __len__(self) -> int:
        return len(self.files)

    def __iter__(self):
        self._halt()
        self._pending, self._done = [], False
        if self._pool is None:      # closed before: it can be iterated again
            self._pool = ThreadPoolExecutor(max_workers=self._workers)
        return self._start(self.groups)

    def __next__(self):
        if self._done:
            raise StopIteration
        if not self._pending:
            try:
                self._pending = list(self._next_unit())
            except StopIteration:
                self._done = True
                raise
        return self._pending.pop(0)

    def close(self):
        self._pending, self._done = [], False
        _ReadAhead.close(self)

    def _read_one(self, k):
        path = self.files[k]
        try:
            return self.agent.reader.read_raw(path)
        except Exception as e:
            raise RuntimeError(f"reading {path} failed: {type(e).__name__}: {e}") from e

    def _build(self, indices, slot):
        raws = self._map(self._read_one, indices)
        names = [self.files[k] for k in indices]
        cap = self.capacity if self.capacity is not None else max(max(r[0].shape[0] for r in raws), 1)
        xyz, idx, count = self._ingest(raws, names, slot, cap)
        original = xyz.clone()      # the chain may act in place on the ingest arena
        frames = [augment.PointCloud.from_buffers(xyz[f], idx[f], count[f:f + 1], R, T, host_n=None if drop else rows.shape[0])
                  for f, (rows, _, R, T, drop) in enumerate(raws)]
        frames = augment.transform_frames(frames, self.chain, streams=self.streams)
        try:
            packed, _, n_in = augment.collate_each(frames, self.padding_to, extra=count)
        except (ValueError, RuntimeError) as e:
            raise type(e)(f"{e} (frames {', '.join(names)})") from e
        dev = self.device
        return [[pts.unsqueeze(0), fr.R.unsqueeze(0).to(dev), fr.T.unsqueeze(0).to(dev), pad.unsqueeze(0),
                 original[f, :n].unsqueeze(0)]
                for f, ((pts, pad), fr, n) in enumerate(zip(packed, frames, n_in))]
