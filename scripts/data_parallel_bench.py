"""What data-parallel training (deeppointmap_amd/data_parallel.py) costs, as far as ONE GPU can show it.  Nothing here runs
between two devices: the gathered buffers are synthetic, and the process group is one rank over RCCL with the collectives forced.

On the full-size model's registration group (184 tensors):
  pack         dpm_flat_pack of every gradient into the flat buffer
  synced       dpm_optim_step_synced (AdamW) at W = 1, 2, 4, 8 slices of a synthetic gathered buffer, with the bytes the kernel
               has to move ((W + 3) reads + 3 writes of 4 bytes per element) over its time, next to the float4-copy rate and the
               peak of the HBM (MI355X: 6.29 and 8.0 TB/s)
  plain        optim.AdamW.step() on the same group: the baseline of a step without an exchange (4 reads + 3 writes)
and on a registration step of --maps x --frames frames of --points points, `set_train_dense("hip")`:
  TrainStep, DataParallelTrainStep(force=True) in both modes, and torch.nn.parallel.DistributedDataParallel around the same
  pipeline with the same optimiser, all on the same one-rank group; and pack + exchange alone as a share of the step.
Times: kernels by device events around --launches back-to-back launches (median of --reps such windows after a warm-up window),
steps by a host clock around work that ends in a device synchronise (median [min, max] of --reps after --warmup).  Reports, not
thresholds.  Writes profiles/data_parallel_bench.md.

  python scripts/data_parallel_bench.py [--maps 8] [--frames 2] [--points 16384] [--reps 10] [--warmup 3] [--launches 50]
"""
import argparse
import os
import pickle
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.distributed as dist

DEV = "cuda"
LOSS = dict(tau=0.1, offset_value="manhattan", eps_positive=1.0, eps_offset=2.0, lambda_p=1.0, lambda_c=1.0, lambda_o=1.0)
HBM_COPY, HBM_PEAK = 6.29e12, 8.0e12   # bytes/s: measured float4 copy, specification
INFINITY_CACHE = 256 << 20


def kernel_us(launch, launches, reps):
    """median over `reps` windows of (device time of `launches` back-to-back launches) / launches, after one warm-up window"""
    out = []
    for k in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            launch()
        b.record()
        b.synchronize()
        if k:
            out.append(a.elapsed_time(b) * 1e3 / launches)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def step_ms(step, reps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


class Slices:
    """an attached GradSync whose exchange already happened: a synthetic (W, L) buffer"""

    def __init__(self, sync, W):
        self.active, self.params, self.offset_of = True, sync.params, sync.offset_of
        self.buffer = torch.randn(W, sync.length, device=DEV) * 1e-3
        self.W, self.length = W, sync.length

    def pack(self):
        pass

    exchange = pack

    def slices(self):
        return self.buffer, self.W, self.length, float(self.W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--port", type=int, default=29870)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("data_parallel_bench.py measures on a GPU; none is visible")
    from deeppointmap_amd import _lib, optim, synthetic
    from deeppointmap_amd.config import default_args
    from deeppointmap_amd.data_parallel import DataParallelTrainStep, GradSync
    from deeppointmap_amd.decoder import Decoder
    from deeppointmap_amd.encoder import Encoder
    from deeppointmap_amd.loss import RegistrationLoss
    from deeppointmap_amd.train_pipeline import DeepPointModelPipeline, TrainStep
    from deeppointmap_amd.weights import init_procedural
    dev = torch.device(DEV, 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{a.port}", rank=0, world_size=1, device_id=dev)
    torch.set_grad_enabled(False)
    kw = dict(lr=1e-5, weight_decay=1e-2)

    def args():
        cfg = default_args()
        cfg.loss = dict(LOSS)
        cfg.train = dict(registration=dict(map_size_max=8, optimizer=dict(type="AdamW", kwargs=dict(kw)),
                                           scheduler=dict(type="identity", kwargs={})))
        return cfg

    def pipeline(cfg):
        enc = init_procedural(Encoder(cfg)).to(DEV).set_train_dense("hip")
        dec = init_procedural(Decoder(cfg)).to(DEV).set_train_dense("hip")
        return DeepPointModelPipeline(cfg, enc, dec, RegistrationLoss(cfg))

    B, S, N = a.maps, a.frames, a.points
    F = B * S
    base = synthetic.base_cloud(N, seed=4)
    ids = [3 * b + s for b in range(B) for s in range(S)]
    pcd = torch.stack([synthetic.frame(f, N, base) for f in ids]).float().to(DEV)
    P = torch.stack([synthetic.sensor_pose(f) for f in ids]).float()
    table = {(ids[b * S], ids[b * S + s]): synthetic.relative_pose(ids[b * S + s], ids[b * S]).numpy() for b in range(B) for s in range(1, S)}
    path = os.path.join(tempfile.mkdtemp(), "refined.pkl")
    with open(path, "wb") as f:
        pickle.dump(table, f)
    data = (pcd, P[:, :3, :3].contiguous().to(DEV), P[:, :3, 3:].contiguous().to(DEV), torch.zeros(F, N, dtype=torch.bool, device=DEV),
            torch.eye(4).repeat(F, 1, 1).to(DEV), {"num_map": B, "dsf_index": [(0, 0, f) for f in ids], "refined_SE3_file": [path] * B})

    # ---- kernels on the registration group ------------------------------------------------------------------------------------
    cfg = args()
    model = pipeline(cfg)
    trained = [p for p in model.parameters() if p.requires_grad]
    for p in trained:
        p.grad = torch.randn_like(p) * 1e-3
    sync = GradSync(trained, force=True)
    n, L = sum(sync.numels), sync.length
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    hyper = (kw["lr"], 0.9, 0.999, 1e-8, kw["weight_decay"], 2.0, 0.0, 0.0, 0, 0)   # the scalars of dpm_optim_step, step 2

    def the_plan(owner):   # the tables the Python layer built for its one launch
        (plan,) = owner._plans.values()
        return plan

    def direct(name, fn, *args_):   # the C entry point itself: the Python layer's walk over 184 tensors stays outside the window
        def launch():
            _lib.check(fn(*args_), name)
        return launch
    lines = []
    sync.pack()
    plan = the_plan(sync)
    us = kernel_us(direct("dpm_flat_pack", lib.dpm_flat_pack, plan.tensors_ptr, plan.chunks_ptr, plan.n_chunks, sync.flat.data_ptr(), L, stream),
                   a.launches, a.reps)
    lines.append(("dpm_flat_pack", us, 8 * n))
    host = [("GradSync.pack()", kernel_us(sync.pack, a.launches, a.reps))]
    opt = optim.AdamW(trained, **kw)
    opt.step()
    plan = the_plan(opt)
    us = kernel_us(direct("dpm_optim_step", lib.dpm_optim_step, optim.ADAMW, plan.tensors_ptr, plan.chunks_ptr, plan.n_chunks, *hyper, stream),
                   a.launches, a.reps)
    lines.append(("dpm_optim_step (AdamW, plain: the baseline)", us, 28 * n))
    host.append(("optim.AdamW.step(), plain", kernel_us(opt.step, a.launches, a.reps)))
    for W in (1, 2, 4, 8):
        opt = optim.AdamW(trained, **kw)
        fixed = Slices(sync, W)
        opt.attach_grad_sync(fixed)
        opt.step()
        plan = the_plan(opt)
        us = kernel_us(direct("dpm_optim_step_synced", lib.dpm_optim_step_synced, optim.ADAMW, plan.tensors_ptr, plan.chunks_ptr,
                              plan.n_chunks, *hyper, fixed.buffer.data_ptr(), W, L, float(W), stream), a.launches, a.reps)
        lines.append((f"dpm_optim_step_synced (AdamW), W = {W}", us, 4 * (W + 6) * n))
        if W == 8:
            host.append(("optim.AdamW.step(), attached, W = 8 (pack and exchange stubbed)", kernel_us(opt.step, a.launches, a.reps)))
        del opt, fixed
    for r in lines + host:
        print(r, flush=True)

    # ---- whole steps on the one-rank group -------------------------------------------------------------------------------------
    steps = []

    def ddp_step():
        cfg = args()
        net = torch.nn.parallel.DistributedDataParallel(pipeline(cfg), device_ids=[0])
        net.train()
        opt = optim.AdamW([p for p in net.parameters() if p.requires_grad], **kw)

        def step():
            with torch.enable_grad():
                loss, _ = net(*data)
                opt.zero_grad()
                loss.backward()
            opt.step()
        return step

    def train_step(cls, **more):
        def make():
            cfg = args()
            ts = cls(cfg, pipeline(cfg), **more)
            return lambda: ts.step(*data)
        return make

    arms = (("TrainStep (no exchange)", train_step(TrainStep)),
            ("DataParallelTrainStep(mode=\"ordered\", force=True)", train_step(DataParallelTrainStep, force=True)),
            ("DataParallelTrainStep(mode=\"allreduce\", force=True)", train_step(DataParallelTrainStep, mode="allreduce", force=True)),
            ("torch DistributedDataParallel + optim.AdamW", ddp_step))
    for name, make in arms:
        try:
            steps.append((name, step_ms(make(), a.reps, a.warmup)))
        except Exception as e:   # an arm that does not run is reported, not hidden
            steps.append((name, f"did not run: {type(e).__name__}: {str(e)[:200]}"))
        print(steps[-1], flush=True)
    # pack + exchange alone, on the gradients a step left behind
    cfg = args()
    ts = DataParallelTrainStep(cfg, pipeline(cfg), force=True)
    for _ in range(a.warmup):
        ts.step(*data)

    def exchange():
        ts.sync.pack()
        ts.sync.exchange()
    ex = kernel_us(exchange, a.launches, a.reps)
    whole = next(v for k, v in steps if k.startswith("DataParallelTrainStep(mode=\"ordered\""))
    dist.destroy_process_group()

    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "data_parallel_bench.md"), "w") as f:
        f.write("# Data-parallel training: what one GPU can show of its cost\n\n")
        f.write(f"`python scripts/data_parallel_bench.py --maps {B} --frames {S} --points {N}` on {torch.cuda.get_device_name(0)} (torch "
                f"{torch.__version__}).  **Nothing between two devices has been run or timed**: the gathered buffers below are "
                "synthetic, and the process group is ONE rank over RCCL with the collectives forced.  What `ordered` costs against "
                "`allreduce` at W = 8 (7 received slices per rank against 1.75) is therefore **not measured**.\n\n")
        f.write(f"## Kernels on the registration group ({len(trained)} tensors, {n} elements, flat length {L})\n\n"
                f"Device events around {a.launches} back-to-back launches of the C entry point on the tables the Python layer built; median "
                f"[min, max] of {a.reps} windows after a warm-up window.  Bytes: what the kernel has "
                "to move, from the shapes.  A working set below the 256 MiB Infinity Cache can be served from it between launches, so its "
                "rate is not an HBM rate; the column says which rows that concerns.\n\n"
                "| what | us per launch | bytes moved | GB/s | of the float4-copy rate (6.29 TB/s) | of the HBM peak (8 TB/s) | working set |\n|---|---|---|---|---|---|---|\n")
        for name, (med, lo, hi), nbytes in lines:
            rate = nbytes / (med * 1e-6)
            fits = "fits the Infinity Cache" if nbytes <= INFINITY_CACHE else "larger than the Infinity Cache"
            f.write(f"| {name} | {med:.1f} [{lo:.1f}, {hi:.1f}] | {nbytes / 1e6:.1f} MB | {rate / 1e9:.0f} | {rate / HBM_COPY:.2f} | "
                    f"{rate / HBM_PEAK:.2f} | {nbytes / 2 ** 20:.0f} MiB, {fits} |\n")
        f.write("\nThe same through the Python layer (its walk over the tensors, the table look-up, the version bumps): when this is the "
                "larger number, the call is bound by the host, not by the kernel.\n\n| call | us per call |\n|---|---|\n")
        for name, (med, lo, hi) in host:
            f.write(f"| {name} | {med:.1f} [{lo:.1f}, {hi:.1f}] |\n")
        f.write(f"\n## A registration step, {B} maps of {S} frames of {N} points, on the one-rank RCCL group\n\n"
                f"Host clock around a step that ends in a device synchronise; median [min, max] ms of {a.reps} after {a.warmup} warm-up "
                "steps.  DistributedDataParallel wraps the same pipeline and steps the same one-launch optimiser.\n\n| arm | ms |\n|---|---|\n")
        for name, v in steps:
            f.write(f"| {name} | {v if isinstance(v, str) else '%.3f [%.3f, %.3f]' % v} |\n")
        f.write(f"\npack + all_gather_into_tensor alone (device events, {a.launches} back-to-back): {ex[0]:.1f} [{ex[1]:.1f}, {ex[2]:.1f}] us")
        if not isinstance(whole, str):
            f.write(f" = {ex[0] * 1e-3 / whole[0] * 100:.2f} % of the ordered step above")
        f.write(".  On one rank the collective is a copy on the device; between devices it is not, and that share is not measured.\n")
    print(open(os.path.join(ROOT, "profiles", "data_parallel_bench.md")).read())


if __name__ == "__main__":
    main()
