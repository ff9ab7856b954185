#!/usr/bin/env python3
"""profiles/scan_context_bench.md: what the Scan Context build and search (csrc/scan_context.hip) cost, next to a dense torch
formulation of the same distances.

* build: one HDL64E-sized frame (64 x 2048 = 131072 rows) of a simulated street into one database row, 20 x 60;
* search: Q = 1 against D = 1 000 and D = 10 000 (the online case) and Q = D = 2 000 with query i limited to the rows below
  i - 50 (the offline case), K = 4, on random descriptors with 60 % occupancy;
* dense torch: all shifted cosine sums as one circular cross-correlation of the columns (an FFT over the sector axis) plus
  the mask overlaps by a second one, a (Q, D, sectors) tensor, min over shifts, top-k over rows -- the tensors the HIP search
  never stores.  Its results are compared with the HIP search's before anything is timed.

Device time between two events around --inner calls, per call, median [min, max] of --reps such windows after --warmup.
Operations of the search as the algorithm needs them: 2 * rings * sectors^2 per visible pair (the Gram matrix).  A report, not a target: nothing about its speed is claimed in advance.

  python scripts/scan_context_bench.py [--reps 20] [--inner 10] [--warmup 3]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

DEV = "cuda"
RINGS, SECTORS, K = 20, 60, 4


def timed(fn, reps, inner, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def fmt(t):
    return f"{t[0] * 1e3:.1f} [{t[1] * 1e3:.1f}, {t[2] * 1e3:.1f}]"


def random_db(n, gen):
    """n normalised descriptors and masks on the device from random raw heights, five columns empty (normalised by torch:
    valid inputs of the search, not the bytes the build would give)"""
    raw = torch.rand(n, RINGS, SECTORS, device=DEV, generator=gen) * 20
    raw = raw * (torch.rand(n, RINGS, SECTORS, device=DEV, generator=gen) < 0.6)
    raw[:, :, :5] = 0
    n2 = (raw * raw).sum(1, keepdim=True)
    norm = torch.where(n2 > 0, raw / n2.sqrt().clamp_min(1e-30), torch.zeros_like(raw)).contiguous()
    bits = (n2[:, 0] > 0).to(torch.int64)
    mask = (bits << torch.arange(SECTORS, device=DEV, dtype=torch.int64)).sum(1)
    return norm, mask


def dense_torch(qn, qm, dn, dm, limit, k, chunk=256):
    """the same distances, densely: S(q, c, s) = sum_j <Aq[:, j], Ac[:, (j + s) % sectors]> by FFT over the sector axis"""
    bit = lambda m: ((m[:, None] >> torch.arange(SECTORS, device=DEV, dtype=torch.int64)) & 1).float()
    fd, fdm = torch.fft.rfft(dn, dim=2), torch.fft.rfft(bit(dm), dim=1)
    rows = torch.arange(dn.shape[0], device=DEV)
    out_d, out_r, out_s = [], [], []
    for a in range(0, qn.shape[0], chunk):
        fq, fqm = torch.fft.rfft(qn[a:a + chunk], dim=2), torch.fft.rfft(bit(qm[a:a + chunk]), dim=1)
        S = torch.fft.irfft((fq.conj()[:, None] * fd[None]).sum(2), n=SECTORS, dim=2)                 # (q, D, sectors)
        used = torch.fft.irfft(fqm.conj()[:, None] * fdm[None], n=SECTORS, dim=2).round()
        d = torch.where(used > 0, (1 - S / used.clamp_min(1)).clamp_min(0), torch.ones_like(S))
        best, shift = d.min(dim=2)
        best = torch.where(rows[None] < limit[a:a + chunk, None], best, torch.full_like(best, float("inf")))
        top = torch.topk(best, k, dim=1, largest=False)
        out_d.append(top.values), out_r.append(top.indices), out_s.append(torch.gather(shift, 1, top.indices))
    return torch.cat(out_d), torch.cat(out_r), torch.cat(out_s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scan_context_bench.py runs on a GPU; none is visible")
    from deeppointmap_amd import lidar_sim as LS, ops
    from deeppointmap_amd.loop_closure import ScanContext, ScanContextDB
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    lines = []

    # build
    scene = LS.street_scene(0, blocks=(3, 3))
    frame = LS.LidarSimulator(scene, LS.HDL64E, device=DEV).frames(LS.circuit(scene, spacing=2.0)[:1])[0]
    sc = ScanContext(RINGS, SECTORS, max_range=80.0, z_offset=LS.SENSOR_HEIGHT)
    db = ScanContextDB(sc, 4)
    out = (db.raw[:1], db.norm[:1], db.mask[:1])
    n = int(frame.count.item())
    t = timed(lambda: sc.describe(frame, out=out), a.reps, a.inner, a.warmup)
    bytes_build = 12 * n + 3 * 4 * RINGS * SECTORS
    lines.append(f"| build, one frame, capacity {frame.cap} rows ({n} valid), {RINGS} x {SECTORS} | {fmt(t)} | - | 3 launches; "
                 f"{bytes_build / 1e6:.2f} MB read and written: {bytes_build / t[0] / 1e6:.1f} GB/s of the call, launch gaps included |")

    # search
    for Q, D, offline in ((1, 1000, False), (1, 10000, False), (2000, 2000, True)):
        dn, dm = random_db(D, gen)
        if offline:
            qn, qm = dn, dm
            limit = torch.clamp(torch.arange(D, device=DEV, dtype=torch.int32) - 50, min=0)
        else:
            qn, qm = random_db(Q, gen)
            limit = torch.full((Q,), D, device=DEV, dtype=torch.int32)
        pairs = int(limit.sum().item())
        got = ops.scan_context_search(qn, qm, dn, dm, limit, K)
        want = dense_torch(qn, qm, dn, dm, limit, K)
        real = torch.isfinite(want[0])
        agree = float((got[1][real] == want[1][real]).float().mean()), float((got[2][real] == want[2][real]).float().mean())
        worst = float((got[0][real] - want[0][real]).abs().max())
        t_hip = timed(lambda: ops.scan_context_search(qn, qm, dn, dm, limit, K), a.reps, a.inner, a.warmup)
        t_torch = timed(lambda: dense_torch(qn, qm, dn, dm, limit, K), max(a.reps // 4, 3), max(a.inner // 5, 1), 1)
        flops = 2.0 * RINGS * SECTORS * SECTORS * pairs
        lines.append(f"| search Q = {Q}, D = {D}{', query i sees rows below i - 50' if offline else ''}, K = {K}: {pairs} pairs | {fmt(t_hip)} | "
                     f"{fmt(t_torch)} | {flops / t_hip[0] / 1e9:.2f} TFLOP/s of the Gram products over the call; rows equal to dense torch's "
                     f"{agree[0]:.4f}, shifts {agree[1]:.4f}, largest distance difference {worst:.1e} |")

    with open(os.path.join(ROOT, "profiles", "scan_context_bench.md"), "w") as f:
        f.write("# Scan Context: build and search\n\n")
        f.write(f"`python scripts/scan_context_bench.py --reps {a.reps} --inner {a.inner} --warmup {a.warmup}` on {torch.cuda.get_device_name(0)}.  "
                f"Device time in microseconds between two events around {a.inner} calls, per call: median [min, max] of {a.reps} windows "
                "(dense torch: a quarter of the windows, a fifth of the calls).  The times are whole calls (two or three launches "
                "and the gaps between them), not kernel times.  Dense torch: the same distances by an FFT over the sector axis, "
                "through (Q, D, sectors) tensors, in chunks of 256 queries.  Where rows or shifts differ from dense torch's, two "
                "distances lie within the rounding of one of the two formulations.  A report, not a target.\n\n")
        f.write("| case | HIP us | dense torch us | notes |\n|---|---|---|---|\n" + "\n".join(lines) + "\n")
    print(open(os.path.join(ROOT, "profiles", "scan_context_bench.md")).read())


if __name__ == "__main__":
    main()
