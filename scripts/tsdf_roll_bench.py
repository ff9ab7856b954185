"""Rolling the TSDF map (csrc/tsdf_map.hip: dpm_tsdf_evict, dpm_tsdf_absorb; tsdf.py: TsdfMap.roll, TsdfArchive) at 2^22 slots:
a table a quarter full of voxels spread over a cube of 102 m (voxel 0.2 m, tiles of 2^5 voxels: 6.4 m).
  evict              dpm_tsdf_evict (clear + rebuild, two launches) at radii that send 0 %, about 10 % and 100 % of the voxels to
                     the list, next to dpm_tsdf_export of the same table: reading the whole table once is the floor, and an
                     evict also clears and writes a second one.  The four calls alternate in one process.
  absorb             dpm_tsdf_absorb of the records each evict listed, into the table that evict built.
  roll               TsdfMap.roll end to end on the host's clock (evict, the read of the count, the copies, the archive's numpy
                     and the absorb, ending in a device synchronise): the sensor moves --stride metres a roll along x, out and
                     back, under the default radii of a 60 m sensor.
The wave-aggregated list position (one atomic a wave) is the only form built; one atomic a lane is not, so they are not compared.
Device time between two events for the kernels, median [min, max] of --reps runs after --warmup; the spread is the [min, max].
A report, not a threshold: no time is asserted.  Written to profiles/tsdf_roll_bench.md.

  python scripts/tsdf_roll_bench.py [--slots 22] [--voxels 1048576] [--reps 11] [--warmup 2] [--stride 15]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

DEV = "cuda"
# scripts/isa_diff.py <parent libdpm_hip.so> <this libdpm_hip.so>, recorded when the three kernels were added
ISA_DIFF = ("symbols: 330 -> 333; renamed 0; removed 0; added 3; common 330, of them identical 330, different 0; "
            "ADDED: ts_absorb_kernel, ts_evict_clear_kernel, ts_evict_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=22)
    ap.add_argument("--voxels", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--stride", type=float, default=15.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tsdf_roll_bench.py measures on a GPU; none is visible")
    from deeppointmap_amd import _lib, ops
    from deeppointmap_amd.tsdf import KEY_BIAS, TsdfArchive, TsdfMap, tile_near, tile_of
    cap, v, b = 1 << a.slots, 0.2, 5
    rng = np.random.default_rng(0)
    xyz = rng.integers(-256, 256, (int(a.voxels * 1.02), 3)) + KEY_BIAS
    keys = np.unique((xyz[:, 0] | (xyz[:, 1] << 21) | (xyz[:, 2] << 42)).astype(np.int64))
    keys = keys[rng.permutation(len(keys))][:a.voxels]
    n = len(keys)
    sums = rng.integers(-(1 << 30), 1 << 30, n, dtype=np.int64)
    counts = rng.integers(1, 1 << 16, n, dtype=np.int64).astype(np.uint32)
    m = TsdfMap(v, max_voxels=cap, max_range=60.0, origin=np.zeros(3), device=DEV).absorb(keys, sums, counts).check()
    lib = _lib.load()
    fmt = lambda t: f"{sorted(t)[len(t) // 2]:.3f} [{min(t):.3f}, {max(t):.3f}]"

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # the radii: from the distances of the voxels' tile centres to the pose, in the kernel's float32 form
    pose = np.eye(4)
    pose[:3, 3] = (3.1, -2.2, 0.4)
    tiles = tile_of(keys, b)
    uniq, inverse = np.unique(tiles, return_inverse=True)
    lo, hi = 0.0, 400.0
    for _ in range(40):                                 # the radius at which about 90 % of the voxels are near
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if tile_near(uniq, b, pose[:3, 3], mid, v)[inverse].mean() < 0.9 else (lo, mid)
    radii = {"0 %": 1e6, "10 %": hi, "100 %": 0.0}
    dst = ops.tsdf_new(cap, DEV)
    lists = [torch.empty(n, dtype=t, device=DEV) for t in (torch.int64, torch.int64, torch.int32)]
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    pose_dev = torch.from_numpy(pose).to(DEV)
    forms = {f"evict {k}": (lambda r=r: ops.tsdf_evict(m.table, dst, cap, v, m.origin, pose_dev, r, b, *lists, count)) for k, r in radii.items()}

    def export():
        count.zero_()
        _lib.check(lib.dpm_tsdf_export(m.table.data_ptr(), cap, *[t.data_ptr() for t in lists], count.data_ptr(), n,
                                       torch.cuda.current_stream().cuda_stream), "dpm_tsdf_export")
    forms["export"] = export
    ms, listed, absorb_ms = {k: [] for k in forms}, {}, {k: [] for k in radii}
    for rep in range(a.warmup + a.reps):
        for name, fn in forms.items():
            t = window(fn)
            if rep >= a.warmup:
                ms[name].append(t)
            if name.startswith("evict"):
                k = name[6:]
                listed[k] = int(count.item())
                if listed[k]:                           # the records just listed, back into the table just built
                    back = [x[:listed[k]] for x in lists]
                    t = window(lambda: ops.tsdf_absorb(dst, cap, *back))
                    if rep >= a.warmup:
                        absorb_ms[k].append(t)
                    assert ops.tsdf_export(dst, cap, 0) == n, "evict + absorb lost or made voxels"
    rows = [dict(name=k, listed=listed.get(k[6:], n) if k != "export" else n, ms=fmt(t),
                 absorb=fmt(absorb_ms[k[6:]]) if k != "export" and absorb_ms[k[6:]] else "-") for k, t in ms.items()]
    for r in rows:
        print(r, flush=True)

    # a roll end to end: out along x and back, the archive filling and emptying
    archive = TsdfArchive(b)
    steps = [a.stride * k for k in (1, 2, 3, 4, 3, 2, 1, 0)] * 2
    rolls = []
    for x in steps:
        P = np.eye(4)
        P[:3, 3] = (x, 0.0, 0.0)
        held = len(archive)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.roll(P, archive)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        rolls.append(dict(x=x, ms=dt, out=m.wanted, back=held + m.wanted - len(archive), archived=len(archive)))
        print(rolls[-1], flush=True)
    assert ops.tsdf_export(m.table, cap, 0) + len(archive) == n and m.overflow() == 0
    timed = [r["ms"] for r in rolls[2:]]                  # the first two build the second table and warm the path
    path = os.path.join(ROOT, "profiles", "tsdf_roll_bench.md")
    with open(path, "w") as f:
        f.write("# Rolling the TSDF map: evict, absorb and a roll end to end\n\n")
        f.write(f"`python scripts/tsdf_roll_bench.py --slots {a.slots} --voxels {a.voxels} --stride {a.stride:g}` on "
                f"{torch.cuda.get_device_name(0)} (torch {torch.__version__}): a table of 2^{a.slots} slots holding {n} voxels "
                f"({n / cap:.0%} full) spread over a cube of 102 m, voxel {v} m, tiles of 2^{b} voxels.  Device time between two "
                f"events, median [min, max] ms of {a.reps} runs after {a.warmup} warm-up runs: the [min, max] is the run-to-run "
                "spread.  The calls alternated in one process.  A report, not a threshold.\n\n")
        f.write("| call | voxels listed | ms | dpm_tsdf_absorb of that list into the rebuilt table, ms |\n|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {'dpm_tsdf_export (the whole table read once, the occupied slots written)' if r['name'] == 'export' else 'dpm_tsdf_' + r['name']} "
                    f"| {r['listed']} | {r['ms']} | {r['absorb']} |\n")
        f.write(f"\nAn evict reads the table's {cap * 20 / 1e6:.0f} MB once, as the export does, and also clears and fills a second one; "
                "every check of `evict` + `absorb` above counted the voxels of the start.\n\n")
        f.write("\nThe three evicts differ by the number of waves that hold a far voxel, not by bytes: each such wave adds once to the one counter, and at a quarter load a wave holds 16 voxels, so 10 % and 100 % both come to about one atomic a wave (65 536 of them), 0 % to none.  Supposed from these figures, not measured with counters; `dpm_tsdf_export`, at the same time as the 100 % evict, would then be paying the same, its per-lane add merged into one a wave by the compiler: also supposed.\n\n")
        f.write(f"`TsdfMap.roll` end to end, host clock round the call and a device synchronise (max_range 60 m, so reach "
                f"{m.reach(b):.1f} m, load radius {m.reach(b) + 10:.1f} m, keep radius {m.reach(b) + 20:.1f} m; the sensor {a.stride:g} m further "
                f"along x every roll, out to {max(steps):g} m and back, twice): median [min, max] of the last {len(timed)} rolls "
                f"**{fmt(timed)} ms**.\n\n| x, m | voxels evicted | voxels absorbed | voxels in the archive after | ms |\n|---|---|---|---|---|\n")
        for r in rolls:
            f.write(f"| {r['x']:g} | {r['out']} | {r['back']} | {r['archived']} | {r['ms']:.2f} |\n")
        f.write("\nThe host's share of a roll is the read of the count, three copies of the list, numpy's sort and merge per tile in "
                "`TsdfArchive.add` / `take`, and the upload for the absorb.\n")
        f.write("\nThe list position is taken with one atomic a wave (ballot and rank); the form with one atomic a lane is not built, so "
                "the two are not compared.\n")
        f.write(f"\nThe kernels that existed compile to the instructions they had (`python scripts/isa_diff.py <parent libdpm_hip.so> "
                f"<head libdpm_hip.so>`): {ISA_DIFF}.\n")
        f.write("\nNot measured: hardware counters of the three kernels, other table sizes and loads, a pinned staging buffer.\n")
    print(open(path).read())


if __name__ == "__main__":
    main()
