"""GPU: data-parallel training steps (deeppointmap_amd/data_parallel.py) on the one GPU of the test box.

* two ranks folded onto the GPU over gloo (spawned as tests/test_gpu_multirank.py does): both end with identical bytes, equal to
  a single process that computes the two gradients one after the other, combines them as (g0 + g1) / 2 and steps the unattached
  optimiser -- and different from a lone TrainStep on rank 0's batch;
* one rank over RCCL in a child process under a timeout: pack -> all_gather_into_tensor / all_reduce -> synced step equal the
  plain TrainStep step byte for byte, without a host synchronisation;
* the stage change and a checkpoint round trip with a plain TrainStep.
Nothing here runs between two devices.
"""
import datetime
import io
import os
import pickle
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
for _p in (ROOT, GOLDEN):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOSS = dict(tau=0.1, offset_value="manhattan", eps_positive=1.0, eps_offset=2.0, lambda_p=1.0, lambda_c=1.0, lambda_o=1.0)
FRAMES = ((0, 3, 5, 9), (1, 4, 6, 11))   # rank r's map
STEPS = 2


def _args():
    import loop_train_cases as LC
    from deeppointmap_amd.config import reduced_args
    cfg = reduced_args()
    cfg.loss = dict(LOSS)
    cfg.train = dict(
        registration=dict(map_size_max=8, optimizer=dict(type="AdamW", kwargs=dict(lr=1e-4, weight_decay=1e-2)),
                          scheduler=dict(type="cosine", kwargs=dict(T_max=10)), K_0=2, K_mult=2, mult_epoch=[2, 4]),
        loop_detection=dict(distance=LC.DISTANCE, optimizer=dict(type="sgd", kwargs=dict(lr=1e-3, momentum=0.9)),
                            scheduler=dict(type="identity", kwargs={})))
    return cfg


def _pipeline(cfg, perturb=0.0):
    """the model in "hip" dense mode (a whole step gives identical bytes twice); `perturb` moves every weight"""
    import encoder_train_cases as EC
    from deeppointmap_amd.decoder import Decoder
    from deeppointmap_amd.encoder import Encoder
    from deeppointmap_amd.loss import RegistrationLoss
    from deeppointmap_amd.train_pipeline import DeepPointModelPipeline
    from deeppointmap_amd.weights import init_procedural
    enc = Encoder(cfg)
    enc.load_state_dict(EC.state_dict(cfg), strict=True)
    dec = init_procedural(Decoder(cfg))
    model = DeepPointModelPipeline(cfg, enc.to(DEV).set_train_dense("hip"), dec.to(DEV).set_train_dense("hip"), RegistrationLoss(cfg))
    if perturb:
        with torch.no_grad():
            for p in model.parameters():
                p.add_(perturb)
    return model


def _batch(tmp, frames, N=4096):
    """one map of four synthetic frames with their global poses, a calibration, and a dictionary that covers one pair"""
    import train_step_cases as C
    from deeppointmap_amd import synthetic
    base = synthetic.base_cloud(N, seed=4)
    pcd = torch.stack([synthetic.frame(f, N, base) for f in frames]).float()
    P = torch.stack([synthetic.sensor_pose(f) for f in frames]).float()
    calib = torch.eye(4).repeat(len(frames), 1, 1)
    path = os.path.join(str(tmp), "refined_%d.pkl" % frames[0])
    a, b = frames[0], frames[1]
    with open(path, "wb") as f:   # frame b in frame a, refined: the pipeline must take this, not the global poses
        pickle.dump({(a, b): synthetic.relative_pose(b, a).numpy() @ np.array(C._se3(np.random.default_rng(2), 0.002, 0.02))}, f)
    info = {"num_map": 1, "dsf_index": [(0, 0, f) for f in frames], "refined_SE3_file": [path]}
    return (pcd.to(DEV), P[:, :3, :3].contiguous().to(DEV), P[:, :3, 3:].contiguous().to(DEV),
            torch.zeros(len(frames), N, dtype=torch.bool, device=DEV), calib.to(DEV), info)


def _result(model, optimizer):
    """every parameter and every optimiser state tensor as bytes, by name"""
    out = {}
    for k, p in model.named_parameters():
        out["p/" + k] = p.detach().cpu().numpy().tobytes()
        for s, v in optimizer.state.get(p, {}).items():
            out[f"{s}/{k}"] = v.detach().cpu().numpy().tobytes() if torch.is_tensor(v) else v
    return out


def _worker(rank, world, port, q, tmp):
    import torch.distributed as dist
    from deeppointmap_amd.data_parallel import DataParallelTrainStep
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    torch.set_grad_enabled(False)
    cfg = _args()
    model = _pipeline(cfg, perturb=0.01 * rank)        # rank 1 starts elsewhere: the constructor's broadcast has to bring it back
    ts = DataParallelTrainStep(cfg, model)
    assert ts.sync.active and ts.sync.world == world and ts.is_main_process == (rank == 0)
    batch = _batch(tmp, FRAMES[rank])
    for _ in range(STEPS):
        random.seed(100 + rank)
        ts.step(*batch)
    torch.cuda.synchronize()
    q.put((rank, _result(ts.pipeline, ts.optimizer), ts.sync.plan_builds, ts.optimizer.plan_builds))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_equal_the_single_process_emulation(tmp_path):
    import torch.multiprocessing as mp
    from deeppointmap_amd import optim
    from deeppointmap_amd.train_pipeline import TrainStep
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + os.getpid() % 200
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, str(tmp_path))) for r in range(world)]
    got = {}
    try:
        for p in procs:
            p.start()
        for _ in range(world):
            rank, result, sync_builds, opt_builds = q.get(timeout=300)
            got[rank] = result
            # tables follow addresses, not steps: a gradient re-allocated after zero_grad() costs at most one rebuild per step, and
            # the synced launch's table holds no gradient address at all
            assert 1 <= sync_builds <= STEPS and opt_builds == 1, (sync_builds, opt_builds)
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    # (1) both ranks hold the same bytes: parameters and optimiser state
    assert sorted(got) == [0, 1] and sorted(got[0]) == sorted(got[1])
    assert all(got[0][k] == got[1][k] for k in got[0])
    # (2) one process: both gradients from the same weights, (g0 + g1) / 2, the unattached optimiser
    cfg = _args()
    model = _pipeline(cfg)
    model.train()
    params = [p for p in model.parameters() if p.requires_grad]
    opt = optim.AdamW(params, **cfg.train["registration"]["optimizer"]["kwargs"])
    batches = [_batch(tmp_path, f) for f in FRAMES]
    for _ in range(STEPS):
        grads = []
        for rank, batch in enumerate(batches):
            random.seed(100 + rank)
            model.zero_grad(set_to_none=True)
            with torch.enable_grad():
                loss, _ = model(*batch)
                loss.backward()
            assert all(p.grad is not None for p in params)
            grads.append([p.grad.clone() for p in params])
        for p, g0, g1 in zip(params, *grads):
            p.grad = (g0 + g1) / 2
        opt.step()
    want = _result(model, opt)
    assert sorted(want) == sorted(got[0])
    wrong = [k for k in want if want[k] != got[0][k]]
    assert not wrong, (len(wrong), wrong[:5])
    # (3) the exchange did something: a lone TrainStep on rank 0's batch ends elsewhere
    cfg = _args()
    lone = TrainStep(cfg, _pipeline(cfg))
    for _ in range(STEPS):
        random.seed(100)
        lone.step(*batches[0])
    alone = _result(lone.model, lone.optimizer)
    assert sum(alone[k] != got[0][k] for k in alone if k.startswith("p/")) >= 150


CHILD = r"""
import os, random, sys, torch
sys.path.insert(0, os.environ["DPMTEST_ROOT"])
sys.path.insert(0, os.path.join(os.environ["DPMTEST_ROOT"], "tests"))
import torch.distributed as dist
import test_gpu_data_parallel as T
from deeppointmap_amd.data_parallel import DataParallelTrainStep, GradSync
from deeppointmap_amd.train_pipeline import TrainStep

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=dev)
assert dist.get_backend() == "nccl"
torch.set_grad_enabled(False)
batch = T._batch(os.environ["DPMTEST_TMP"], T.FRAMES[0])

def run(make):
    cfg = T._args()
    ts = make(cfg, T._pipeline(cfg))
    for _ in range(T.STEPS):
        random.seed(100)
        ts.step(*batch)
    torch.cuda.synchronize()
    return ts, T._result(ts.pipeline, ts.optimizer)

_, want = run(lambda cfg, model: TrainStep(cfg, model))
assert not GradSync(torch.nn.Linear(2, 2).parameters()).active   # without force a one-rank group is inert
for mode in ("ordered", "allreduce"):
    ts, got = run(lambda cfg, model: DataParallelTrainStep(cfg, model, mode=mode, force=True))
    sync = ts.sync
    assert sync.active and sync.world == 1 and len(sync.params) == 184 and sync.length % 4 == 0
    assert (sync.gathered is not None and tuple(sync.gathered.shape) == (1, sync.length)) == (mode == "ordered")
    wrong = [k for k in want if want[k] != got[k]]
    assert sorted(got) == sorted(want) and not wrong, (mode, len(wrong), wrong[:5])
    # the flat buffer holds the local gradients at their offsets, zeros in the padding
    flat = sync.flat.cpu()
    used = torch.zeros(sync.length, dtype=torch.bool)
    for p, o in zip(sync.params, sync.offsets):
        assert torch.equal(flat[o:o + p.numel()], p.grad.reshape(-1).cpu())
        used[o:o + p.numel()] = True
    assert not flat[~used].any()
    # a further synced optimiser step with the gradients in place: no call that synchronises the host
    builds = (sync.plan_builds, ts.optimizer.plan_builds)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ts.optimizer.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert (sync.plan_builds, ts.optimizer.plan_builds) == builds   # no address changed: no table rebuilt
    # a gradient that is None on this rank travels as zeros, and its tensor is still updated (weight decay, moments)
    p0 = sync.params[0]
    before = p0.detach().clone()
    p0.grad = None
    ts.optimizer.step()
    o = sync.offsets[0]
    assert not sync.flat[o:o + p0.numel()].any() and not torch.equal(p0.detach(), before)

# GradSync alone, forced: broadcast_parameters from the only rank leaves the values as they are
lin = torch.nn.Linear(5, 3).to(dev)
keep = [p.detach().clone() for p in lin.parameters()]
GradSync(lin.parameters(), force=True).broadcast_parameters(0)
assert all(torch.equal(a, b) for a, b in zip(keep, lin.parameters()))
torch.cuda.synchronize()
dist.destroy_process_group()
print("DATA_PARALLEL_RCCL_OK")
"""


def test_one_rank_over_rccl_equals_the_plain_step(tmp_path):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29100 + os.getpid() % 200),
               HSA_ENABLE_IPC_MODE_LEGACY="0", DPMTEST_ROOT=ROOT, DPMTEST_TMP=str(tmp_path))
    env.pop("RANK", None), env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0 and "DATA_PARALLEL_RCCL_OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


def test_stage_change_and_checkpoint_round_trip(tmp_path):
    import loop_train_cases as LC
    from deeppointmap_amd import optim
    from deeppointmap_amd.data_parallel import DataParallel, DataParallelTrainStep
    from deeppointmap_amd.train_pipeline import TrainStep
    batch = _batch(tmp_path, FRAMES[0])
    cfg = _args()
    dp = DataParallelTrainStep(cfg, _pipeline(cfg))
    assert isinstance(dp.model, DataParallel) and dp.pipeline is dp.model.module and dp.is_main_process
    assert type(dp.optimizer) is optim.AdamW and len(dp.sync.params) == 110 + 74
    assert [id(p) for p in dp.sync.params] == [id(p) for p in dp.optimizer.param_groups[0]["params"]]
    random.seed(0)
    dp.step(*batch)
    saved = dp.state_dict()
    assert sorted(saved) == ["decoder", "encoder", "epoch", "optimizer", "scheduler", "step"] and saved["step"] == 1
    assert not any(k.startswith("module.") for k in list(saved["encoder"]) + list(saved["decoder"]))   # the reference's layout
    assert sorted(dp.weights()) == ["decoder", "encoder"]
    blob = io.BytesIO()
    torch.save(saved, blob)
    # into a plain TrainStep, one step there and one here: the same bytes; and the plain one's checkpoint comes back
    cfg2 = _args()
    plain = TrainStep(cfg2, _pipeline(cfg2, perturb=0.5))
    plain.load_state_dict(torch.load(io.BytesIO(blob.getvalue()), weights_only=False))
    for ts in (dp, plain):
        random.seed(1)
        ts.step(*batch)
    assert _result(plain.model, plain.optimizer) == _result(dp.pipeline, dp.optimizer)
    blob = io.BytesIO()
    torch.save(plain.state_dict(), blob)
    cfg3 = _args()
    back = DataParallelTrainStep(cfg3, _pipeline(cfg3, perturb=0.5))
    back.load_state_dict(torch.load(io.BytesIO(blob.getvalue()), weights_only=False))
    assert back.step_count == 2 and _result(back.pipeline, back.optimizer) == _result(dp.pipeline, dp.optimizer)
    # the stage change: a new optimiser and a new layout over exactly the eight loop_head tensors
    dp.next_stage()
    names = {id(p): k for k, p in dp.pipeline.named_parameters()}
    assert type(dp.optimizer) is optim.SGD and dp.optimizer._sync is dp.sync
    assert sorted(names[id(p)] for p in dp.sync.params) == sorted("decoder." + k for k in LC.HEAD)
    assert len(dp.sync.offsets) == 8 and dp.sync.length == sum((p.numel() + 3) // 4 * 4 for p in dp.sync.params)
    assert dp.pipeline.decoder.train_stage == "loop_detection"
