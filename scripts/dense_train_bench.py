"""The dense training kernels (csrc/dense_train.hip) on the GPU, against the torch layers they replace -- the "torch" mode of the
same checkout, which is the code path before them, unchanged:
(a) ops.dense_linear_train / ops.dense_linear_ln_train forward + backward against F.linear (+ F.layer_norm, F.relu) under autograd,
    at (R, Cin, Cout) = (4096, 256, 768), (4096, 256, 256) normed, (131072, 16, 32), (4096, 512, 2048) normed;
(b) Decoder.forward -> RegistrationLoss -> backward() at B = 8, 256 x 256 and B = 2, 4096 x 4096, train_dense "torch" and "hip";
(c) Encoder.train().forward -> backward at 8 x 16 384 points, both modes.
Per line: ms per step (median, min and max of --reps after --warmup; a host clock around work that ends in a device synchronise,
the two sides alternating step by step) and peak device memory above what is allocated before the step.  Writes dense_train_bench.json and .md into --out-dir (default profiles/).

  python scripts/dense_train_bench.py [--reps 10] [--warmup 3] [--out-dir profiles] [--only a,b,c]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch
import torch.nn.functional as F

import decoder_train_cases as C
from deeppointmap_amd import ops, synthetic
from deeppointmap_amd.config import default_args
from deeppointmap_amd.decoder import Decoder
from deeppointmap_amd.encoder import Encoder
from deeppointmap_amd.loss import RegistrationLoss
from deeppointmap_amd.weights import init_procedural

DEV = "cuda"
OPS = [(4096, 256, 768, False), (4096, 256, 256, True), (131072, 16, 32, False), (4096, 512, 2048, True)]
STEPS = [(8, 256, 256), (2, 4096, 4096)]


def timed(steps, reps, warmup):
    """steps: {side: callable}.  The sides alternate step by step (what else runs on the machine then hits both alike); every
    shape is warmed up on every side first.  -> {side: dict(ms (median), ms_min, ms_max, peak_mib)}"""
    for _ in range(warmup):
        for step in steps.values():
            step()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    times, peak = {k: [] for k in steps}, {k: 0 for k in steps}
    for _ in range(reps):
        for k, step in steps.items():
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
            peak[k] = max(peak[k], torch.cuda.max_memory_allocated() - base)
    out = {}
    for k, t in times.items():
        t.sort()
        out[k] = dict(ms=t[len(t) // 2], ms_min=t[0], ms_max=t[-1], peak_mib=peak[k] / 2**20)
    return out


def op_row(R, Cin, Cout, normed, reps, warmup):
    g = torch.Generator().manual_seed(1)
    x, dy, res = (torch.randn(R, c, generator=g).to(DEV) for c in (Cin, Cout, Cout))
    W = (torch.randn(Cout, Cin, generator=g) / Cin ** 0.5).to(DEV)
    b, ga, be = torch.zeros(Cout, device=DEV), torch.ones(Cout, device=DEV), torch.zeros(Cout, device=DEV)

    def leaves():
        return [t.detach().clone().requires_grad_(True) for t in ((x, W, b, ga, be, res) if normed else (x, W, b))]

    def hip():
        L = leaves()
        with torch.enable_grad():
            out = ops.dense_linear_ln_train(L[0], L[1], L[2], L[3], L[4], residual=L[5], act=ops.ACT_RELU) if normed else \
                ops.dense_linear_train(L[0], L[1], L[2], act=ops.ACT_RELU)
            return torch.autograd.grad(out, L, dy)

    def torch_layers():
        L = leaves()
        with torch.enable_grad():
            out = F.relu(F.layer_norm(F.linear(L[0], L[1], L[2]) + L[5], (Cout,), L[3], L[4])) if normed else \
                F.relu(F.linear(L[0], L[1], L[2]))
            return torch.autograd.grad(out, L, dy)
    return dict(R=R, Cin=Cin, Cout=Cout, normed=normed, **timed(dict(torch=torch_layers, hip=hip), reps, warmup))


def decoder_row(B, M, N, reps, warmup, layers=3):
    cfg = C.cfg(layers=layers)
    side = (B * M * N * 33.5 / 4000.0) ** (1 / 3) if M * N > 1 << 16 else 30.0   # a few thousand offset pairs at every shape
    inputs = C._make(7, B, M, N, side=max(side, 20.0))
    t = lambda a: torch.from_numpy(a).to(DEV, torch.float32)   # noqa: E731
    src, dst, Rg, Tg = t(inputs["src"]), t(inputs["dst"]), t(inputs["R"]), t(inputs["T"])
    ps, pd = (torch.from_numpy(m).to(DEV) for m in C.masks(inputs))
    xs_global = Rg @ src[:, -3:] + Tg
    dec = Decoder(cfg)
    dec.load_state_dict(C.state_dict(cfg), strict=True)
    dec = dec.to(DEV).train()
    crit = RegistrationLoss(cfg)
    params = [p for p in dec.parameters() if p.requires_grad]

    def step(mode):
        dec.set_train_dense(mode)
        a, b = src.detach().requires_grad_(True), dst.detach().requires_grad_(True)
        with torch.enable_grad():
            outs = dec(a, b, ps, pd, (Rg, Tg))
            loss = crit(xs_global, dst[:, -3:], ps, pd, *outs)[0]
            torch.autograd.grad(loss, [a, b] + params, allow_unused=True)
    return dict(B=B, M=M, N=N, layers=layers, checkpointed=B * (M + N) >= dec.train_checkpoint_rows,
                **timed(dict(torch=lambda: step("torch"), hip=lambda: step("hip")), reps, warmup))


def encoder_row(B, N, reps, warmup):
    cfg = default_args()
    base = synthetic.base_cloud(N, seed=9)
    pts = torch.stack([synthetic.frame(2 * b, N, base) for b in range(B)]).float().to(DEV)
    pad = torch.zeros(B, N, dtype=torch.bool, device=DEV)
    enc = init_procedural(Encoder(cfg)).to(DEV).train()
    params = list(enc.parameters())
    S = cfg.encoder.npoint[len(cfg.encoder.npoint) - cfg.encoder.upsample_layers - 1]
    G = torch.randn(B, cfg.encoder.out_channel, S, generator=torch.Generator().manual_seed(3)).to(DEV)

    def step(mode):
        enc.set_train_dense(mode)
        _, fea, _ = enc(pts, pad)
        with torch.enable_grad():
            return torch.autograd.grad((fea * G).sum(), params)
    return dict(B=B, N=N, **timed(dict(torch=lambda: step("torch"), hip=lambda: step("hip")), reps, warmup))


def cell(r):
    return f"{r['ms']:.2f} [{r['ms_min']:.2f}, {r['ms_max']:.2f}] | {r['peak_mib']:.0f}"


def verdict(rows, label):
    slower = [label(r) for r in rows if r["hip"]["ms"] >= r["torch"]["ms"]]
    if not slower:
        return "`hip` is faster at every row of this section.\n"
    return "`hip` is NOT faster at: " + "; ".join(slower) + ".\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--only", default="a,b,c")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dense_train_bench.py measures on a GPU; none is visible")
    torch.set_grad_enabled(False)
    only = set(a.only.split(","))
    ops_rows = [op_row(*s, a.reps, a.warmup) for s in OPS] if "a" in only else []
    for r in ops_rows:
        print(json.dumps(r), flush=True)
    dec_rows = []
    for s in STEPS if "b" in only else []:
        dec_rows.append(decoder_row(*s, a.reps, a.warmup))
        print(json.dumps(dec_rows[-1]), flush=True)
    enc_rows = [encoder_row(8, 16384, a.reps, a.warmup)] if "c" in only else []
    for r in enc_rows:
        print(json.dumps(r), flush=True)
    os.makedirs(a.out_dir, exist_ok=True)
    meta = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=a.reps, warmup=a.warmup)
    json.dump(dict(meta=meta, ops=ops_rows, decoder=dec_rows, encoder=enc_rows), open(os.path.join(a.out_dir, "dense_train_bench.json"), "w"),
              indent=1)
    with open(os.path.join(a.out_dir, "dense_train_bench.md"), "w") as f:
        f.write("# Dense training layers: csrc/dense_train.hip against the torch layers under autograd\n\n")
        f.write(f"`python scripts/dense_train_bench.py` on {meta['device']} (torch {meta['torch']}); median [min, max] ms of {a.reps} "
                f"steps after {a.warmup} warm-up steps, host clock around a step that ends in a device synchronise, the two sides alternating step by step; peak = device "
                "memory allocated above the state before the step.  The baseline is the `\"torch\"` mode of the same checkout: the "
                "code path before these kernels, unchanged.  Nothing here is gated on.\n\n")
        f.write("## (a) one layer, forward + backward (ReLU; the normed rows with a residual)\n\n")
        f.write("| R | Cin | Cout | form | torch ms | torch peak MiB | hip ms | hip peak MiB |\n|---|---|---|---|---|---|---|---|\n")
        for r in ops_rows:
            f.write(f"| {r['R']} | {r['Cin']} | {r['Cout']} | {'normed' if r['normed'] else 'plain'} | {cell(r['torch'])} | {cell(r['hip'])} |\n")
        f.write("\n" + verdict(ops_rows, lambda r: f"({r['R']}, {r['Cin']}, {r['Cout']})"))
        f.write("\n## (b) `Decoder.forward` -> `RegistrationLoss` -> backward, attention_layers = 3\n\n")
        f.write("| B | M | N | layers recomputed | torch ms | torch peak MiB | hip ms | hip peak MiB |\n|---|---|---|---|---|---|---|---|\n")
        for r in dec_rows:
            f.write(f"| {r['B']} | {r['M']} | {r['N']} | {'yes' if r['checkpointed'] else 'no'} | {cell(r['torch'])} | {cell(r['hip'])} |\n")
        f.write("\n" + verdict(dec_rows, lambda r: f"B = {r['B']}, {r['M']} x {r['N']}"))
        f.write("\n## (c) `Encoder.train().forward` -> backward, shipped config\n\n")
        f.write("| B | N | torch ms | torch peak MiB | hip ms | hip peak MiB |\n|---|---|---|---|---|---|\n")
        for r in enc_rows:
            f.write(f"| {r['B']} | {r['N']} | {cell(r['torch'])} | {cell(r['hip'])} |\n")
        f.write("\n" + verdict(enc_rows, lambda r: f"{r['B']} x {r['N']}"))


if __name__ == "__main__":
    main()
