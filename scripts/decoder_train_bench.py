"""The decoder's training step on the GPU: (a) ops.attention_train forward + backward against autograd over the dense formula in
fp32 torch, (b) Decoder.forward -> RegistrationLoss -> backward() against the dense plain-torch restatement
(tests/decoder_train_restated.py), at (B, M, N) = (8, 256, 256), (2, 4096, 256), (2, 4096, 4096), attention_layers = 3.
Per shape and side: ms per step (median, min and max of --reps after --warmup; a host clock around work that ends in a device
synchronise), peak device memory above what is allocated before the step, and for the HIP step the time between device events
around its HIP operators (attention cores, offset pairing, loss), i.e. the share left to the torch dense layers.
Writes profiles/decoder_train_bench.json and .md.

  python scripts/decoder_train_bench.py [--shapes 8x256x256,2x4096x256,2x4096x4096] [--reps 10] [--warmup 3]
  rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/decoder_train_bench.py --shapes 2x4096x4096 --reps 3 --warmup 1 --no-dense --no-write
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

import decoder_train_cases as C
import decoder_train_restated as R
from deeppointmap_amd import ops
from deeppointmap_amd.decoder import Decoder
from deeppointmap_amd.loss import RegistrationLoss

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
        out = step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    peak = torch.cuda.max_memory_allocated() - base
    times.sort()
    return dict(ms=times[len(times) // 2], ms_min=times[0], ms_max=times[-1], peak_mib=peak / 2**20), out


def guarded(fn):
    try:
        return fn()
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        return None


def attention_rows(B, M, N, reps, warmup, dense):
    g = torch.Generator().manual_seed(1)
    q, k, v, do = (torch.randn(B * n, 256, generator=g).to(DEV) for n in (M, N, N, M))

    def hip():
        leaves = [t.detach().requires_grad_(True) for t in (q, k, v)]
        with torch.enable_grad():
            return torch.autograd.grad(ops.attention_train(*leaves, B, M, N, 8), leaves, do)

    def torch_dense():
        leaves = [t.detach().requires_grad_(True) for t in (q, k, v)]
        with torch.enable_grad():
            h = lambda t, n: t.view(B, n, 8, 32).transpose(1, 2)   # noqa: E731
            s = h(leaves[0], M) @ h(leaves[1], N).transpose(-1, -2) / 32 ** 0.5
            o = (torch.softmax(s, -1) @ h(leaves[2], N)).transpose(1, 2).reshape(B * M, 256)
            return torch.autograd.grad(o, leaves, do)

    row = dict(B=B, M=M, N=N, hip=timed(hip, reps, warmup)[0])
    if dense:
        r = guarded(lambda: timed(torch_dense, reps, warmup))
        row["dense"] = r[0] if r else None
    return row


class HipClock:
    """device events around the HIP operators of a step (one stream: the time between an operator's events is its kernels')"""

    NAMES = ("attention_train_forward", "attention_train_backward", "offset_pairs", "reg_loss_pairs", "reg_loss_forward",
             "reg_loss_backward", "_segment_sum")

    def __init__(self):
        self.events, self.orig = [], {}

    def __enter__(self):
        for n in self.NAMES:
            f = self.orig[n] = getattr(ops, n)

            def wrapped(*a, _f=f, **k):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                out = _f(*a, **k)
                e.record()
                self.events.append((s, e))
                return out
            setattr(ops, n, wrapped)
        return self

    def __exit__(self, *exc):
        for n, f in self.orig.items():
            setattr(ops, n, f)

    def ms(self):
        torch.cuda.synchronize()
        return sum(s.elapsed_time(e) for s, e in self.events)


def step_rows(B, M, N, layers, reps, warmup, dense):
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

    def hip():
        a, b = src.detach().requires_grad_(True), dst.detach().requires_grad_(True)
        with torch.enable_grad():
            outs = dec(a, b, ps, pd, (Rg, Tg))
            loss = crit(xs_global, dst[:, -3:], ps, pd, *outs)[0]
            torch.autograd.grad(loss, [a, b] + params, allow_unused=True)
        return float(loss), outs[4].shape[0]

    sd = {k: v.detach().clone().requires_grad_("loop" not in k) for k, v in dec.state_dict().items()}
    sd_params = [v for v in sd.values() if v.requires_grad]

    def torch_dense():
        a, b = src.detach().requires_grad_(True), dst.detach().requires_grad_(True)
        with torch.enable_grad():
            loss, outs, _ = R.training_step(sd, cfg, a, b, ps, pd, Rg, Tg)
            torch.autograd.grad(loss, [a, b] + sd_params, allow_unused=True)
        return float(loss), outs[4].shape[0]

    row = dict(B=B, M=M, N=N, layers=layers, checkpointed=B * (M + N) >= dec.train_checkpoint_rows)
    row["hip"], (loss, K) = timed(hip, reps, warmup)
    row["hip"].update(loss=loss, K=K)
    with HipClock() as clock:
        n = 3
        for _ in range(n):
            hip()
        row["hip"]["hip_operators_ms"] = clock.ms() / n
    row["hip"]["torch_layers_share"] = 1.0 - row["hip"]["hip_operators_ms"] / row["hip"]["ms"]
    if dense:
        r = guarded(lambda: timed(torch_dense, reps, warmup))
        row["dense"] = dict(r[0], loss=r[1][0], K=r[1][1]) if r else None
    return row


def fmt(r, key="ms"):
    return "-" if r is None else f"{r[key]:.2f}" if key == "ms" else f"{r[key]:.0f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x256x256,2x4096x256,2x4096x4096")
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-dense", action="store_true")
    ap.add_argument("--no-attention", action="store_true")
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decoder_train_bench.py measures on a GPU; none is visible")
    torch.set_grad_enabled(False)
    shapes = [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",")]
    att, steps = [], []
    for B, M, N in shapes:
        if not a.no_attention:
            att.append(attention_rows(B, M, N, a.reps, a.warmup, not a.no_dense))
            print(json.dumps(att[-1]), flush=True)
        steps.append(step_rows(B, M, N, a.layers, a.reps, a.warmup, not a.no_dense))
        print(json.dumps(steps[-1]), flush=True)
    if a.no_write:
        return
    prof = os.path.join(ROOT, "profiles")
    meta = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=a.reps, warmup=a.warmup, layers=a.layers)
    json.dump(dict(meta=meta, attention=att, step=steps), open(os.path.join(prof, "decoder_train_bench.json"), "w"), indent=1)
    with open(os.path.join(prof, "decoder_train_bench.md"), "w") as f:
        f.write("# Decoder training step: HIP attention / offset pairing against dense fp32 torch\n\n")
        f.write(f"`python scripts/decoder_train_bench.py` on {meta['device']} (torch {meta['torch']}); median [min, max] ms of "
                f"{a.reps} steps after {a.warmup} warm-up steps, host clock around a step that ends in a device synchronise; "
                "peak = device memory allocated above the state before the step.\n\n")
        f.write("## (a) `ops.attention_train` forward + backward, 8 heads x 32, no mask\n\n")
        f.write("| B | M | N | HIP ms | HIP peak MiB | dense torch ms | dense torch peak MiB |\n|---|---|---|---|---|---|---|\n")
        for r in att:
            h, d = r["hip"], r.get("dense")
            ds = f"{d['ms']:.2f} [{d['ms_min']:.2f}, {d['ms_max']:.2f}] | {d['peak_mib']:.0f}" if d else "- | -"
            f.write(f"| {r['B']} | {r['M']} | {r['N']} | {h['ms']:.2f} [{h['ms_min']:.2f}, {h['ms_max']:.2f}] | {h['peak_mib']:.0f} | {ds} |\n")
        f.write(f"\n## (b) `Decoder.forward` -> `RegistrationLoss` -> backward, attention_layers = {a.layers}\n\n")
        f.write("| B | M | N | K | layers recomputed | HIP ms | HIP peak MiB | of which HIP operators ms | torch dense layers' share | "
                "dense restatement ms | dense restatement peak MiB |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in steps:
            h, d = r["hip"], r.get("dense")
            ds = f"{d['ms']:.2f} [{d['ms_min']:.2f}, {d['ms_max']:.2f}] | {d['peak_mib']:.0f}" if d else "- | -"
            f.write(f"| {r['B']} | {r['M']} | {r['N']} | {h['K']} | {'yes' if r['checkpointed'] else 'no'} | {h['ms']:.2f} "
                    f"[{h['ms_min']:.2f}, {h['ms_max']:.2f}] | {h['peak_mib']:.0f} | {h['hip_operators_ms']:.2f} | "
                    f"{100 * h['torch_layers_share']:.0f} % | {ds} |\n")


if __name__ == "__main__":
    main()
