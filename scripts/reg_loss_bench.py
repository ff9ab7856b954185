"""RegistrationLoss forward + backward at B = 4, S = D in {1024, 4096, 8192}: the fused HIP loss (deeppointmap_amd/loss.py)
against the plain-torch restatement (tests/reg_loss_restated.py) on the same GPU.  Per shape: ms per forward + backward (median
of --reps after --warmup), peak device memory above what the inputs hold, and the loss of both.  Writes
profiles/reg_loss_bench.json and .md.

  python scripts/reg_loss_bench.py [--sizes 1024,4096,8192] [--reps 10] [--warmup 3]
  rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/reg_loss_bench.py --sizes 8192 --reps 3 --no-restated --no-write
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

import reg_loss_cases
import reg_loss_restated as R
from deeppointmap_amd.loss import RegistrationLoss


def inputs(B, S, D, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    side = (S / 6.0) ** (1 / 3)
    xs = torch.rand(B, 3, S, generator=g) * side
    idx = torch.randint(0, S, (B, D), generator=g)
    xd = torch.gather(xs, 2, idx.unsqueeze(1).expand(B, 3, D)) + (torch.rand(B, 3, D, generator=g) - 0.5) * 0.3
    t = dict(xs=xs, xd=xd, ps=torch.zeros(B, S, dtype=torch.bool), pd=torch.zeros(B, D, dtype=torch.bool),
             fs=torch.randn(B, 256, S, generator=g), fd=torch.randn(B, 256, D, generator=g),
             cs=torch.randn(B, 128, S, generator=g), cd=torch.randn(B, 128, D, generator=g),
             os=torch.randn(64, 3, 1, generator=g), od=torch.randn(64, 3, 1, generator=g))
    return {k: v.to(dev) for k, v in t.items()}


def measure(fn, t, reps, warmup):
    feats = [t[k].detach().requires_grad_(True) for k in ("fs", "fd", "cs", "cd")]

    def step():
        with torch.enable_grad():
            out = fn(t["xs"], t["xd"], t["ps"], t["pd"], *feats, t["os"], t["od"])
            torch.autograd.grad(out[0], feats)
        return out

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
    return dict(ms=times[len(times) // 2], ms_min=times[0], peak_mib=peak / 2**20, loss=float(out[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096,8192")
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-restated", action="store_true")
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    cfg = reg_loss_cases.cfg("manhattan")
    fused = RegistrationLoss(cfg)
    rows = []
    for S in [int(x) for x in a.sizes.split(",")]:
        t = inputs(a.B, S, S, "cuda")
        row = dict(B=a.B, S=S, D=S, inputs_mib=sum(t[k].numel() * 4 for k in ("fs", "fd", "cs", "cd")) / 2**20)
        row["fused"] = measure(fused, t, a.reps, a.warmup)
        if not a.no_restated:
            try:
                row["restated"] = measure(lambda *x: R.registration_loss(*x, cfg)[0], t, a.reps, a.warmup)
            except torch.cuda.OutOfMemoryError as e:   # noqa: F841
                row["restated"] = None
                torch.cuda.empty_cache()
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.no_write:
        return
    prof = os.path.join(ROOT, "profiles")
    meta = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=a.reps, warmup=a.warmup)
    json.dump(dict(meta=meta, rows=rows), open(os.path.join(prof, "reg_loss_bench.json"), "w"), indent=1)
    with open(os.path.join(prof, "reg_loss_bench.md"), "w") as f:
        f.write("# RegistrationLoss forward + backward: fused HIP vs the plain-torch restatement\n\n")
        f.write(f"`python scripts/reg_loss_bench.py` on {meta['device']} (torch {meta['torch']}), fp32 features C = 256 / C' = 128, "
                f"no padding, median of {a.reps} after {a.warmup} warm-up calls; peak = device memory allocated above the inputs "
                "during forward + backward.\n\n")
        f.write("| B | S = D | feature inputs MiB | fused ms | fused peak MiB | restated ms | restated peak MiB | loss fused | loss restated |\n")
        f.write("|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            fu, re_ = r["fused"], r.get("restated")
            rs = (f"{re_['ms']:.2f} | {re_['peak_mib']:.0f} | {fu['loss']:.6f} | {re_['loss']:.6f}" if re_ else
                  f"- | - | {fu['loss']:.6f} | -")
            f.write(f"| {r['B']} | {r['S']} | {r['inputs_mib']:.0f} | {fu['ms']:.2f} | {fu['peak_mib']:.0f} | {rs} |\n")


if __name__ == "__main__":
    main()
