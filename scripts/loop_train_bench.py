"""The loop-detection training stage on the GPU, at (B, M, N) = (32, 256, 256) and (8, 4096, 4096), attention_layers = 3:
(a) the loop head forward + loss + backward through ops.loop_pool (Decoder._loop_head_train) against the dense torch autograd
    OverlapHead (tests/loop_train_restated.py) on the same correlated features;
(b) a whole stage-two step -- frozen encoder on 2 B clouds of --points points, trunk, head, LoopDetectionLoss, backward -- with
    both modules at train stage "loop_detection" (encoder and trunk on the inference kernels) against the same step with the
    encoder and the trunk on their registration-stage training forwards under no_grad, which is what `.train()` ran before the
    stage switch existed.  The decoder's descriptors are the seeded ones of tests/golden/decoder_train_cases.py at the
    requested (B, M, N) in both arms (the encoder's token count is not a parameter of the step); the encoder's work is timed
    with the step, as a stage-two step pays it.
Per arm: ms per step (median, min and max of --reps after --warmup; a host clock around work that ends in a device synchronise)
and peak device memory above what is allocated before the step.  Writes profiles/loop_train_bench.json and .md.

  python scripts/loop_train_bench.py [--shapes 32x256x256,8x4096x4096] [--reps 10] [--warmup 3] [--points 16384]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch
import torch.nn.functional as F

import loop_train_cases as C
import loop_train_restated as R
from decoder_train_bench import guarded, timed
from deeppointmap_amd import ops, synthetic
from deeppointmap_amd.config import default_args
from deeppointmap_amd.decoder import Decoder
from deeppointmap_amd.encoder import Encoder
from deeppointmap_amd.loss import LoopDetectionLoss
from deeppointmap_amd.weights import init_procedural

DEV = "cuda"


def head_rows(dec, cfg, B, M, N, reps, warmup):
    g = torch.Generator().manual_seed(2)
    E = cfg.decoder.model_channel
    x, y = torch.randn(B * M, E, generator=g).to(DEV), torch.randn(B * N, E, generator=g).to(DEV)
    gt = torch.arange(B, device=DEV) % 2 == 0
    params = [p for p in dec.parameters() if p.requires_grad]

    def hip():
        with torch.enable_grad():
            loss, _ = ops.loop_bce(dec._loop_head_train(x, y, B, M, N), gt.float())
            torch.autograd.grad(loss, params)
        return loss

    sd = {k: v.detach().clone().requires_grad_(True) for k, v in dec.state_dict().items() if "loop" in k}

    def dense():
        with torch.enable_grad():
            loss, _ = R.loop_loss(R.loop_head(sd, x.view(B, M, E), y.view(B, N, E)), gt)
            torch.autograd.grad(loss, list(sd.values()))
        return loss

    row = dict(B=B, M=M, N=N, hip=timed(hip, reps, warmup)[0])
    r = guarded(lambda: timed(dense, reps, warmup))
    row["dense"] = r[0] if r else None
    return row


def trunk_training_forward(dec, src, dst, ps, pd):
    """the attention trunk as Decoder.forward runs it in the registration stage (torch dense layers, ops.attention_train)
    -> x (B*M,E), y (B*N,E)"""
    C_, E = dec.in_channel, dec.model_channel
    B, _, M = src.shape
    N = dst.shape[2]
    rows = torch.cat([src[:, :C_].transpose(1, 2).reshape(B * M, C_), dst[:, :C_].transpose(1, 2).reshape(B * N, C_)])
    xyz = torch.cat([src[:, C_:].transpose(1, 2).reshape(B * M, 3), dst[:, C_:].transpose(1, 2).reshape(B * N, 3)])
    pos = ops.posemb(xyz, dec._dimt(src.device), E)
    z = F.linear(rows, *dec._w("projection"))
    for l in range(dec.attention_layers):
        z = dec._train_layer(l, z, pos, B, M, N, ps.view(torch.uint8), pd.view(torch.uint8))
    return z[:B * M].contiguous(), z[B * M:].contiguous()


def step_rows(dec, enc, cfg, B, M, N, points, reps, warmup):
    inputs = C.D._make(7, B, M, N)
    t = lambda a: torch.from_numpy(a).to(DEV, torch.float32)   # noqa: E731
    src, dst = t(inputs["src"]), t(inputs["dst"])
    ps, pd = (torch.from_numpy(m).to(DEV) for m in C.masks(inputs))
    src_T = torch.zeros(B, 3, 1, device=DEV)
    dst_T = src_T.clone()
    dst_T[:, 0, 0] = torch.where(torch.arange(B, device=DEV) % 2 == 0, 3.0, 30.0)
    base = synthetic.base_cloud(points, seed=4)
    clouds = torch.stack([synthetic.frame(f, points, base) for f in range(2 * B)]).float().to(DEV)
    cpad = torch.zeros(2 * B, points, dtype=torch.bool, device=DEV)
    crit = LoopDetectionLoss(cfg)
    params = [p for k, p in dec.flat().items() if "loop" in k]

    def staged():
        enc.set_train_stage("loop_detection").train(), dec.set_train_stage("loop_detection").train()
        with torch.enable_grad():
            enc(clouds, cpad)
            loss, _ = crit(dec.loop_detection_forward(src, dst, ps, pd), src_T, dst_T)
            torch.autograd.grad(loss, params)
        return loss

    def unstaged():
        enc.set_train_stage("registration").train(), dec.set_train_stage("loop_detection").train()
        with torch.no_grad():
            enc(clouds, cpad)      # the training forward builds (and drops) its graph whatever the caller's grad mode
            x, y = trunk_training_forward(dec, src, dst, ps, pd)
        with torch.enable_grad():
            loss, _ = crit(dec._loop_head_train(x, y, B, M, N), src_T, dst_T)
            torch.autograd.grad(loss, params)
        return loss

    row = dict(B=B, M=M, N=N, points=points, clouds=2 * B, staged=timed(staged, reps, warmup)[0])
    r = guarded(lambda: timed(unstaged, reps, warmup))
    row["unstaged"] = r[0] if r else None
    enc.eval(), dec.eval()
    return row


def cell(d):
    return f"{d['ms']:.2f} [{d['ms_min']:.2f}, {d['ms_max']:.2f}] | {d['peak_mib']:.0f}" if d else "- | -"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32x256x256,8x4096x4096")
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loop_train_bench.py measures on a GPU; none is visible")
    torch.set_grad_enabled(False)
    cfg = C.cfg(layers=a.layers)
    dec = Decoder(cfg)
    dec.load_state_dict(C.state_dict(cfg), strict=True)
    dec = dec.to(DEV)
    enc = init_procedural(Encoder(default_args())).to(DEV)
    heads, steps = [], []
    for B, M, N in [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",")]:
        dec.set_train_stage("loop_detection").train()
        heads.append(head_rows(dec, cfg, B, M, N, a.reps, a.warmup))
        print(json.dumps(heads[-1]), flush=True)
        steps.append(step_rows(dec, enc, cfg, B, M, N, a.points, a.reps, a.warmup))
        print(json.dumps(steps[-1]), flush=True)
    if a.no_write:
        return
    prof = os.path.join(ROOT, "profiles")
    meta = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=a.reps, warmup=a.warmup, layers=a.layers)
    json.dump(dict(meta=meta, head=heads, step=steps), open(os.path.join(prof, "loop_train_bench.json"), "w"), indent=1)
    with open(os.path.join(prof, "loop_train_bench.md"), "w") as f:
        f.write("# Loop-detection training stage: fused loop head and the stage switch\n\n")
        f.write(f"`python scripts/loop_train_bench.py` on {meta['device']} (torch {meta['torch']}); median [min, max] ms of "
                f"{a.reps} steps after {a.warmup} warm-up steps, host clock around a step that ends in a device synchronise; "
                "peak = device memory allocated above the state before the step.  Reports, not thresholds.\n\n")
        f.write("## (a) loop head forward + loss + backward on given features\n\n")
        f.write("| B | M | N | `ops.loop_pool` head ms | peak MiB | dense torch head ms | peak MiB |\n|---|---|---|---|---|---|---|\n")
        for r in heads:
            f.write(f"| {r['B']} | {r['M']} | {r['N']} | {cell(r['hip'])} | {cell(r['dense'])} |\n")
        f.write(f"\n## (b) a whole stage-two step (encoder on 2 B clouds, trunk of {a.layers} layers, head, loss, backward)\n\n")
        f.write("| B | M | N | clouds x points | stage `loop_detection` ms | peak MiB | encoder and trunk on their training "
                "forwards ms | peak MiB |\n|---|---|---|---|---|---|---|---|\n")
        for r in steps:
            f.write(f"| {r['B']} | {r['M']} | {r['N']} | {r['clouds']} x {r['points']} | {cell(r['staged'])} | {cell(r['unstaged'])} |\n")


if __name__ == "__main__":
    main()
