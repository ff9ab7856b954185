"""One registration training step on the GPU, at B maps of S frames of --points points (default encoder: 256 tokens a frame, so
B = 8, S = 2 is the decoder's 8 x 256 x 256), `set_train_dense("hip")`, done two ways on the same modules and batch:
  torch glue   encoder -> tests/train_step_restated.py (the map assembly as batched torch operations, poses included) ->
               decoder -> RegistrationLoss -> backward -> torch.optim.AdamW, in its default form and with fused=True
  this project DeepPointModelPipeline (ops.map_poses + ops.map_assemble) -> backward -> deeppointmap_amd.optim.AdamW
plus the two new pieces alone: the assembly (poses + assemble forward + backward) against the same torch glue, and the
optimiser step over the model's 184 trained tensors against torch.optim.AdamW (default, foreach=False, fused=True).
Per arm: ms (median, min and max of --reps after --warmup; a host clock around work that ends in a device synchronise) and the
number of host synchronisations torch reports in one step (torch.cuda.set_sync_debug_mode("warn"): calls made through
torch that wait for the device; both arms share the encoder's, the decoder's and the criterion's).
Reports, not thresholds; every number stands next to the torch-glue number of the same run.  Also turns
test_logs/train_step_errors.log, which the GPU tests write, into profiles/train_step_accuracy.md (--accuracy-only: just that).

  python scripts/train_step_bench.py [--maps 8] [--frames 2] [--points 16384] [--reps 10] [--warmup 3]
"""
import argparse
import os
import pickle
import sys
import tempfile
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np
import torch

import train_step_restated as R

DEV = "cuda"
LOSS = dict(tau=0.1, offset_value="manhattan", eps_positive=1.0, eps_offset=2.0, lambda_p=1.0, lambda_c=1.0, lambda_o=1.0)


def timed(step, reps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    torch.cuda.set_sync_debug_mode("warn")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        step()
    torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    syncs = sum("synchroniz" in str(w.message).lower() for w in caught)
    return dict(ms=times[len(times) // 2], ms_min=times[0], ms_max=times[-1], syncs=syncs)


def accuracy_md():
    src = os.path.join(ROOT, "test_logs", "train_step_errors.log")
    if not os.path.exists(src):
        return False
    lines = sorted(set(open(src).read().splitlines()))
    with open(os.path.join(ROOT, "profiles", "train_step_accuracy.md"), "w") as f:
        f.write("# Training step: observed errors\n\nEvery comparison the GPU tests of the map assembly, the pipeline and the optimisers "
                "made (tests/test_gpu_train_step.py, tests/test_gpu_optim.py), as they logged it; the bounds are derived in those "
                "files.  `ref32` / `ref64`: the reference's (assembly) or torch.optim's (optimisers) fp32 and fp64 runs.\n\n```\n")
        f.write("\n".join(lines) + "\n```\n")
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--accuracy-only", action="store_true")
    a = ap.parse_args()
    wrote = accuracy_md()
    if a.accuracy_only:
        sys.exit(0 if wrote else "test_logs/train_step_errors.log not found: run the GPU tests first")
    if not torch.cuda.is_available():
        sys.exit("train_step_bench.py measures on a GPU; none is visible")
    from deeppointmap_amd import ops, optim, synthetic
    from deeppointmap_amd.config import default_args
    from deeppointmap_amd.decoder import Decoder
    from deeppointmap_amd.encoder import Encoder
    from deeppointmap_amd.loss import RegistrationLoss
    from deeppointmap_amd.train_pipeline import DeepPointModelPipeline, icp_table
    from deeppointmap_amd.weights import init_procedural
    torch.set_grad_enabled(False)
    cfg = default_args()
    cfg.loss = dict(LOSS)
    cfg.train = dict(registration=dict(map_size_max=8))
    B, S, N = a.maps, a.frames, a.points
    F, S1 = B * S, max(1, S // 2)
    enc = init_procedural(Encoder(cfg)).to(DEV).set_train_dense("hip")
    dec = init_procedural(Decoder(cfg)).to(DEV).set_train_dense("hip")
    crit = RegistrationLoss(cfg)
    model = DeepPointModelPipeline(cfg, enc, dec, crit)
    model.train()
    trained = [p for p in model.parameters() if p.requires_grad]
    base = synthetic.base_cloud(N, seed=4)
    ids = [3 * b + s for b in range(B) for s in range(S)]
    pcd = torch.stack([synthetic.frame(f, N, base) for f in ids]).float().to(DEV)
    P = torch.stack([synthetic.sensor_pose(f) for f in ids]).float()
    Rm, T = P[:, :3, :3].contiguous().to(DEV), P[:, :3, 3:].contiguous().to(DEV)
    calib, pad = torch.eye(4).repeat(F, 1, 1).to(DEV), torch.zeros(F, N, dtype=torch.bool, device=DEV)
    table = {(ids[b * S], ids[b * S + s]): synthetic.relative_pose(ids[b * S + s], ids[b * S]).numpy() for b in range(B) for s in range(1, S)}
    path = os.path.join(tempfile.mkdtemp(), "refined.pkl")
    pickle.dump(table, open(path, "wb"))
    info = {"num_map": B, "dsf_index": [(0, 0, f) for f in ids], "refined_SE3_file": [path] * B}
    scale = cfg.slam_system.coor_scale
    index = np.asarray(ids).reshape(B, S)

    def glue(coor, fea, mask):
        icp, has = icp_table(index, [table] * B, S1)
        rel, gt = R.poses(Rm, T, calib, torch.from_numpy(icp).to(DEV), torch.from_numpy(has).to(DEV), S, S1)
        return R.assemble(coor, fea, mask, rel, gt, S, S1, scale), gt

    def hip_glue(coor, fea, mask):
        icp, has = icp_table(index, [table] * B, S1)
        rel, gt = ops.map_poses(Rm, T, calib, torch.from_numpy(icp).to(DEV), torch.from_numpy(has).to(DEV), S, S1)
        return ops.map_assemble(coor, fea, mask, rel, gt, S, S1, scale), gt

    def torch_step(opt):
        def step():
            with torch.enable_grad():
                coor, fea, mask = enc(pcd, pad)
                (sd, dd, sm, dm, sg, dg), gt = glue(coor, fea, mask)
                gt = gt.reshape(B, 3, 4)
                outs = dec(sd, dd, src_padding_mask=sm, dst_padding_mask=dm, gt_Rt=(gt[:, :, :3].contiguous(), gt[:, :, 3:].contiguous()))
                loss = crit(sg, dg, sm, dm, *outs)[0]
                opt.zero_grad()
                loss.backward()
            opt.step()
        return step

    def hip_step(opt):
        def step():
            with torch.enable_grad():
                loss, _ = model(pcd, Rm, T, pad, calib, info, s1=S1)
                opt.zero_grad()
                loss.backward()
            opt.step()
        return step

    rows = []
    kw = dict(lr=1e-5, weight_decay=1e-2)
    for name, make in (("torch glue + torch.optim.AdamW", lambda: torch_step(torch.optim.AdamW(trained, **kw))),
                       ("torch glue + torch.optim.AdamW(fused=True)", lambda: torch_step(torch.optim.AdamW(trained, fused=True, **kw))),
                       ("DeepPointModelPipeline + optim.AdamW", lambda: hip_step(optim.AdamW(trained, **kw)))):
        rows.append(("step", name, timed(make(), a.reps, a.warmup)))
        print(rows[-1], flush=True)
    # the assembly alone: forward + backward on the encoder's outputs
    with torch.enable_grad():
        coor, fea, mask = enc(pcd, pad)
    coor, fea = coor.detach(), fea.detach()

    def assembly(fn):
        def step():
            leaf = fea.clone().requires_grad_(True)
            with torch.enable_grad():
                (sd, dd, *_), _ = fn(coor, leaf, mask)
                (sd.sum() + dd.sum()).backward()
        return step
    rows.append(("assembly", "torch glue (batched torch operations)", timed(assembly(glue), a.reps, a.warmup)))
    rows.append(("assembly", "ops.map_poses + ops.map_assemble", timed(assembly(hip_glue), a.reps, a.warmup)))
    # the optimiser step alone, on the gradients of the last step
    for p in trained:
        if p.grad is None:
            p.grad = torch.zeros_like(p)
    for name, opt in (("torch.optim.AdamW (default)", torch.optim.AdamW(trained, **kw)),
                      ("torch.optim.AdamW(foreach=False)", torch.optim.AdamW(trained, foreach=False, **kw)),
                      ("torch.optim.AdamW(fused=True)", torch.optim.AdamW(trained, fused=True, **kw)),
                      ("optim.AdamW (one launch)", optim.AdamW(trained, **kw))):
        rows.append(("optimiser", name, timed(opt.step, a.reps, a.warmup)))
    for r in rows[3:]:
        print(r, flush=True)
    with open(os.path.join(ROOT, "profiles", "train_step_bench.md"), "w") as f:
        f.write("# The registration training step: torch glue and torch.optim against the pipeline and the one-launch optimiser\n\n")
        f.write(f"`python scripts/train_step_bench.py --maps {B} --frames {S} --points {N}` on {torch.cuda.get_device_name(0)} (torch "
                f"{torch.__version__}): {B} maps of {S} frames (S1 = {S1}), {len(trained)} trained tensors, `set_train_dense(\"hip\")`; "
                f"median [min, max] ms of {a.reps} runs after {a.warmup} warm-up runs, host clock around work that ends in a device "
                "synchronise; syncs = host synchronisations torch reports in one run.  Reports, not thresholds: compare each row "
                "with the torch row of its block.\n\n| what | arm | ms | syncs |\n|---|---|---|---|\n")
        for what, name, d in rows:
            f.write(f"| {what} | {name} | {d['ms']:.3f} [{d['ms_min']:.3f}, {d['ms_max']:.3f}] | {d['syncs']} |\n")
        by = {(w, n): d["ms"] for w, n, d in rows}
        slower = [f"{w}: {n} ({by[(w, n)]:.3f} ms against {ref:.3f} ms)" for (w, n), ref in
                  ((("step", rows[2][1]), rows[0][2]["ms"]), (("assembly", rows[4][1]), rows[3][2]["ms"]),
                   (("optimiser", rows[8][1]), min(r[2]["ms"] for r in rows[5:8]))) if by[(w, n)] > ref]
        f.write("\nWhere HIP is slower than the torch arm of its block: " + ("; ".join(slower) if slower else "nowhere in this run") + ".\n")


if __name__ == "__main__":
    main()
