"""The encoder's training step on the GPU: (a) one grouping layer, ops.group_train forward + backward against autograd over the
dense formula in fp32 torch (tests/encoder_train_restated.py::group_layer), (b) Encoder.train().forward -> backward of a seeded
cotangent against the dense plain-torch restatement of the whole encoder on the module's own geometry, with the shipped config
at B x N = 2 x 8192 and 8 x 16 384; the HIP step both with and without per-stage recomputation (Encoder.train_checkpoint_rows).
Per row and side: ms per step (median, min and max of --reps after --warmup; a host clock around work that ends in a device
synchronise) and peak device memory (torch.cuda.max_memory_allocated) above what is allocated before the step.
Writes encoder_train_bench.json and .md into --out-dir (default profiles/).

  python scripts/encoder_train_bench.py [--shapes 2x8192,8x16384] [--reps 10] [--warmup 3] [--out-dir profiles]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import encoder_train_restated as R
from deeppointmap_amd import ops, synthetic
from deeppointmap_amd.config import default_args
from deeppointmap_amd.encoder import Encoder
from deeppointmap_amd.weights import init_procedural

DEV = "cuda"


def timed(step, reps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    peak = torch.cuda.max_memory_allocated() - base
    times.sort()
    return dict(ms=times[len(times) // 2], ms_min=times[0], ms_max=times[-1], peak_mib=peak / 2**20)


def guarded(fn):
    try:
        return fn()
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        return None


def frames(B, N):
    base = synthetic.base_cloud(N, seed=9)
    pts = torch.stack([synthetic.frame(2 * b, N, base) for b in range(B)]).float()
    return pts, torch.zeros(B, N, dtype=torch.bool)


def layer_row(B, N, S, K, Cout, radius, reps, warmup, dense):
    """the first SetAbstraction's shape class: N points, S FPS centres, Cin = Cout / 2"""
    pts, pad = frames(B, N)
    xyz, lengths = ops.prepare_points(pts.to(DEV).contiguous(), pad.to(DEV))
    _, centers, _ = ops.fps(xyz, lengths, S)
    idx = ops.knn_hybrid(xyz, lengths, centers, K, radius)
    g = torch.Generator().manual_seed(2)
    Cin = Cout // 2
    fea = torch.randn(B, N, Cin, generator=g).to(DEV)
    W = (torch.randn(Cout, Cin + 3, generator=g) / (Cin + 3) ** 0.5).to(DEV)
    bias, gamma, beta = torch.zeros(Cout, device=DEV), torch.ones(Cout, device=DEV), torch.zeros(Cout, device=DEV)
    dout = torch.randn(B, S, Cout, generator=g).to(DEV)

    def leaves():
        return [t.detach().clone().requires_grad_(True) for t in (fea, W, bias, gamma, beta)]

    def hip():
        f, w, b, ga, be = leaves()
        with torch.enable_grad():
            P = torch.nn.functional.linear(f, w[:, :Cin], b)
            out = ops.group_train(P, xyz, centers, idx, w[:, Cin:].contiguous(), ga, be, radius)
            return torch.autograd.grad(out, (f, w, b, ga, be), dout)

    def torch_dense():
        f, w, b, ga, be = leaves()
        with torch.enable_grad():
            out, _, _ = R.group_layer(xyz, f, centers, idx, w, b, ga, be, radius)
            return torch.autograd.grad(out, (f, w, b, ga, be), dout)

    row = dict(B=B, N=N, S=S, K=K, Cout=Cout, hip=timed(hip, reps, warmup))
    if dense:
        row["dense"] = guarded(lambda: timed(torch_dense, reps, warmup))
    return row


def step_row(B, N, reps, warmup, dense):
    cfg = default_args()
    pts, pad = frames(B, N)
    pts, pad = pts.to(DEV), pad.to(DEV)
    enc = init_procedural(Encoder(cfg)).to(DEV).train()
    params = list(enc.parameters())
    S = cfg.encoder.npoint[len(cfg.encoder.npoint) - cfg.encoder.upsample_layers - 1]
    G = torch.randn(B, cfg.encoder.out_channel, S, generator=torch.Generator().manual_seed(3)).to(DEV)

    def hip():
        _, fea, _ = enc(pts, pad)
        with torch.enable_grad():
            return torch.autograd.grad((fea * G).sum(), params)

    row = dict(B=B, N=N)
    for label, rows in (("hip", 1 << 62), ("hip_recompute", 0)):
        enc.train_checkpoint_rows = rows
        row[label] = timed(hip, reps, warmup)
    if dense:
        trace = {}
        enc.train_checkpoint_rows = 1 << 62
        enc(pts, pad, trace=trace)
        n = len(cfg.encoder.npoint)
        level_xyz = [trace[f"downsampler.{i}.fps.new"] for i in range(n)]
        level_len = [trace[f"downsampler.{i}.len"] for i in range(n)]
        idx = {name: trace[name + ".idx"] for name, *_ in R.layer_names(cfg)}
        xyz = pts.transpose(1, 2).contiguous()
        sd = {k: v.detach().clone().requires_grad_(True) for k, v in enc.state_dict().items()}
        del trace

        def torch_dense():
            with torch.enable_grad():
                fea, _ = R.encoder_train_restated(cfg, sd, xyz, level_xyz, level_len, idx)
                return torch.autograd.grad((fea.transpose(1, 2) * G).sum(), list(sd.values()))
        row["dense"] = guarded(lambda: timed(torch_dense, reps, warmup))
    return row


def cell(r):
    return "- | -" if r is None else f"{r['ms']:.2f} [{r['ms_min']:.2f}, {r['ms_max']:.2f}] | {r['peak_mib']:.0f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2x8192,8x16384")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-dense", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("encoder_train_bench.py measures on a GPU; none is visible")
    torch.set_grad_enabled(False)
    shapes = [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",")]
    layers, steps = [], []
    for B, N in shapes:
        layers.append(layer_row(B, N, 4096, 32, 32, 0.05, a.reps, a.warmup, not a.no_dense))
        print(json.dumps(layers[-1]), flush=True)
        steps.append(step_row(B, N, a.reps, a.warmup, not a.no_dense))
        print(json.dumps(steps[-1]), flush=True)
    os.makedirs(a.out_dir, exist_ok=True)
    meta = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=a.reps, warmup=a.warmup)
    json.dump(dict(meta=meta, layer=layers, step=steps), open(os.path.join(a.out_dir, "encoder_train_bench.json"), "w"), indent=1)
    write_md(meta, layers, steps, a.out_dir)


def write_md(meta, layers, steps, out_dir):
    with open(os.path.join(out_dir, "encoder_train_bench.md"), "w") as f:
        f.write("# Encoder training step: the HIP grouping layer against dense fp32 torch autograd\n\n")
        f.write(f"`python scripts/encoder_train_bench.py` on {meta['device']} (torch {meta['torch']}); median [min, max] ms of "
                f"{meta['reps']} steps after {meta['warmup']} warm-up steps, host clock around a step that ends in a device synchronise; "
                "peak = torch.cuda.max_memory_allocated above the state before the step.  The dense side is the plain-torch "
                "restatement (tests/encoder_train_restated.py) on the same device and the same neighbour indices.\n\n")
        f.write("## (a) one grouping layer, forward + backward (projection included), S = 4096 centres, K = 32, Cout = 32\n\n")
        f.write("| B | N | HIP ms | HIP peak MiB | dense torch ms | dense torch peak MiB |\n|---|---|---|---|---|---|\n")
        for r in layers:
            f.write(f"| {r['B']} | {r['N']} | {cell(r['hip'])} | {cell(r.get('dense'))} |\n")
        f.write("\n## (b) `Encoder.train().forward` -> backward, shipped config (sampling and neighbour queries included on the HIP "
                "side; the dense side is given the geometry)\n\n")
        f.write("| B | N | HIP ms | HIP peak MiB | HIP, stages recomputed ms | peak MiB | dense restatement ms | dense restatement peak MiB |\n"
                "|---|---|---|---|---|---|---|---|\n")
        for r in steps:
            f.write(f"| {r['B']} | {r['N']} | {cell(r['hip'])} | {cell(r['hip_recompute'])} | {cell(r.get('dense'))} |\n")
        f.write("\n## Recomputing the stages in the backward (`Encoder.train_checkpoint_rows`)\n\n")
        for r in steps:
            h, c = r["hip"], r["hip_recompute"]
            f.write(f"* B x N = {r['B']} x {r['N']} ({r['B'] * r['N']} input points): recomputation saves "
                    f"{h['peak_mib'] - c['peak_mib']:.0f} of {h['peak_mib']:.0f} MiB and costs {c['ms'] - h['ms']:+.2f} ms "
                    f"({100 * (c['ms'] / h['ms'] - 1):+.0f} %).\n")
        f.write("\nWhat a step keeps without recomputation is the dense layers' activations, about 1.5 KiB per input point at the "
                "shipped widths; the grouping layers add their projected rows and a byte per output element.  The default threshold "
                "(2^20 input points per call, where that comes to about 1.5 GiB) is set from these rows: below it the saving is a "
                "small fraction of a GiB on a 288 GB device and every step pays the extra forward.\n")


if __name__ == "__main__":
    main()
