"""Meshing the TSDF map (csrc/tsdf_map.hip: dpm_tsdf_mesh, dpm_tsdf_mesh_indexed; deeppointmap_amd/tsdf.py) on the workload of
scripts/tsdf_bench.py: the stored frames of lidar_sim.street_scene(2) under HDL64E, one metre apart along the circuit, thinned as
LoopCloser stores them (voxel_sample 0.5, the first 8192 valid rows), fused in one launch; voxel 0.2 m, TsdfMap's defaults.
  mesh()            as it is, in its three parts: the kernel (dpm_tsdf_mesh into outputs sized by a counting pass, the count's
                    read included: device events), the copy of the soup to the host and the numpy weld (host clock).
  mesh_indexed()    dpm_tsdf_mesh_indexed with outputs sized by its counting pass (six launches, the read of V and F included:
                    device events), the sorts into weld's order (TsdfMap.mesh_indexed whole, host clock to a synchronise, minus
                    nothing: reported whole) and the copy of the five tensors to the host.
  merged_mesh       the same map through one scratch table in k batches of tiles (32 voxels a side) holding about equal numbers of
                    voxels, k = 2 and 8: whole (host clock), and its parts -- the export and the cut into tiles alone, those
                    two with the batches (needed_records, absorb, mesh_indexed(tiles=), copy), the merge by vertex name in
                    numpy: whole is about the last two together.
mesh(), mesh_indexed() + copy and merged_mesh alternate in one process; median [min, max] of --reps runs after --warmup; two
windows [min, max] that do not overlap are called disjoint.  Every result is compared with mesh()'s bytes before it is timed.
A report, not a threshold: no time is asserted.  Written to profiles/tsdf_mesh_bench.md.

  python scripts/tsdf_mesh_bench.py [--frames 200] [--reps 5] [--warmup 1] [--batches 2 8]
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


def window(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def clocked(fn):
    """host clock round fn, which ends on the host or in a synchronise -> (ms, result)"""
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def evented(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def equal_split(by_tile, k):
    """the sorted tiles in k consecutive groups holding about equal numbers of voxels"""
    tiles = sorted(by_tile)
    total, out, run = sum(len(by_tile[t][0]) for t in tiles), [[]], 0
    for t in tiles:
        if run >= total * len(out) / k and len(out) < k:
            out.append([])
        out[-1].append(t)
        run += len(by_tile[t][0])
    return [np.array(b, np.int64) for b in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--max-voxels", type=int, default=1 << 22)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tsdf_mesh_bench.py measures on a GPU; none is visible")
    from deeppointmap_amd import augment, lidar_sim as LS, ops, tsdf
    from deeppointmap_amd.odometry import _copy
    scene, model = LS.street_scene(2), LS.HDL64E
    truth = LS.circuit(scene, spacing=1.0)[:a.frames]
    F, P = len(truth), a.points
    sim = LS.LidarSimulator(scene, model, device=DEV)
    store = torch.zeros(F, 3, P, device=DEV)
    lengths = torch.zeros(F, device=DEV, dtype=torch.int32)
    for k, f in enumerate(sim.frames(truth)):
        work = augment.voxel_sample(_copy(f), 0.5)
        n = min(work.cap, P)
        store[k, :, :n] = work.xyz[:n].t()
        lengths[k:k + 1] = torch.clamp(work.count, min=0, max=n)
    g = tsdf.TsdfMap(max_voxels=a.max_voxels, max_range=model.max_range, origin=truth[F // 2][:3, 3], device=DEV)
    g.integrate_frames(store, lengths, torch.arange(F, device=DEV, dtype=torch.int32), torch.from_numpy(np.ascontiguousarray(truth)).to(DEV))
    g.check()
    n_vox, n_tri = ops.tsdf_export(g.table, g.max_voxels, 0), ops.tsdf_mesh(g.table, g.max_voxels, g.voxel_size, 1, 0)
    V, Fc = ops.tsdf_mesh_indexed(g.table, g.max_voxels, g.voxel_size, 1, max_out=(0, 0))
    assert Fc == n_tri
    b = 5
    by_tile = tsdf.records_by_tile(*g.export(), b)
    plans = {k: equal_split(by_tile, k) for k in a.batches}
    scratch = {}
    for k, plan in plans.items():
        need = max(len(tsdf.needed_records(by_tile, owners, b)[0]) for owners in plan)
        scratch[k] = 1 << int(np.ceil(np.log2(2 * need)))                          # the smallest table the largest batch half fills

    want = g.mesh()
    same = lambda x, y: all(p.dtype == q.dtype and p.shape == q.shape and p.tobytes() == q.tobytes() for p, q in zip(x, y))
    whole = [t.cpu().numpy() for t in g.mesh_indexed()]
    assert same(whole[:2], want), "mesh_indexed: other bytes than mesh()"
    for k in a.batches:
        got = tsdf.merged_mesh(g, None, scratch_voxels=scratch[k], batches=plans[k])
        assert same(got, whole[:3]), f"merged_mesh in {k} batches: other bytes"

    ms = {name: [] for name in ("mesh(): kernel", "mesh(): copy", "mesh(): numpy weld", "mesh(): whole", "mesh_indexed(): kernels",
                                "mesh_indexed(): whole", "mesh_indexed(): copy", "mesh_indexed() + copy")}
    for k in a.batches:
        ms.update({f"merged_mesh, {k} batches: {part}": [] for part in ("whole", "export and tiles alone", "export, tiles and batches", "merge")})
    for rep in range(a.warmup + a.reps):
        row = {}
        row["mesh(): kernel"], soup = evented(lambda: ops.tsdf_mesh(g.table, g.max_voxels, g.voxel_size, 1, n_tri)[1:])
        row["mesh(): copy"], on_host = clocked(lambda: [t.cpu().numpy() for t in soup])
        row["mesh(): numpy weld"], _ = clocked(lambda: tsdf.weld(*on_host))
        row["mesh(): whole"], _ = clocked(g.mesh)
        del soup, on_host
        row["mesh_indexed(): kernels"], _ = evented(lambda: ops.tsdf_mesh_indexed(g.table, g.max_voxels, g.voxel_size, 1, max_out=(V, Fc)))
        row["mesh_indexed(): whole"], mesh = clocked(g.mesh_indexed)
        row["mesh_indexed(): copy"], _ = clocked(lambda: [t.cpu().numpy() for t in mesh])
        row["mesh_indexed() + copy"], _ = clocked(lambda: [t.cpu().numpy() for t in g.mesh_indexed()])
        del mesh
        for k in a.batches:
            head = f"merged_mesh, {k} batches: "
            row[head + "whole"], _ = clocked(lambda: tsdf.merged_mesh(g, None, scratch_voxels=scratch[k], batches=plans[k]))
            row[head + "export and tiles alone"], _ = clocked(lambda: tsdf.records_by_tile(*g.export(), b))
            row[head + "export, tiles and batches"], parts = clocked(lambda: tsdf._batched(g, None, scratch[k], plans[k], lambda s, owners, bits: [
                t.cpu().numpy() for t in s.mesh_indexed(1, owners, bits)]))
            row[head + "merge"], _ = clocked(lambda: tsdf.weld_indexed(parts))
            del parts
        print(f"run {rep + 1} of {a.warmup + a.reps}: " + ", ".join(f"{name} {v:.0f}" for name, v in row.items()), flush=True)
        if rep >= a.warmup:
            for name, v in row.items():
                ms[name].append(v)
    t = {name: window(v) for name, v in ms.items()}
    fmt = lambda w: f"{w[0]:.1f} [{w[1]:.1f}, {w[2]:.1f}]"
    disjoint = lambda x, y: "disjoint" if t[x][2] < t[y][1] or t[y][2] < t[x][1] else "overlapping"
    path = os.path.join(ROOT, "profiles", "tsdf_mesh_bench.md")
    with open(path, "w") as f:
        f.write("# Meshing the TSDF map: the soup welded in numpy, the indexed mesh, and the mesh in batches\n\n")
        f.write(f"`python scripts/tsdf_mesh_bench.py --frames {a.frames} --reps {a.reps} --warmup {a.warmup}` on {torch.cuda.get_device_name(0)}: "
                f"{F} stored frames ({int(lengths.sum())} points) fused into {n_vox} voxels of 0.2 m in a table of {g.max_voxels} slots; "
                f"{n_tri} triangles, {V} vertices.  Milliseconds, median [min, max] of {a.reps} runs after {a.warmup}, the forms "
                f"alternating in one process.  `kernel(s)` rows are device time between two events with the read of the counts "
                f"inside; every other row is the host's clock round work that ends on the host or in a synchronise.  mesh_indexed() and "
                f"every merged_mesh were compared with mesh()'s bytes first: identical.\n\n")
        f.write("| what | ms |\n|---|---|\n")
        for name in ms:
            f.write(f"| {name} | {fmt(t[name])} |\n")
        f.write("\n| batches | tiles per batch | scratch table, slots | largest batch's records (owners + halo) |\n|---|---|---|---|\n")
        for k in a.batches:
            need = max(len(tsdf.needed_records(by_tile, owners, b)[0]) for owners in plans[k])
            f.write(f"| {k} | {[len(p) for p in plans[k]]} | {scratch[k]} | {need} |\n")
        f.write(f"\nWindows: mesh(): whole against mesh_indexed() + copy: {disjoint('mesh(): whole', 'mesh_indexed() + copy')}; the numpy weld "
                f"against mesh_indexed(): whole (kernels and the device sorts): {disjoint('mesh(): numpy weld', 'mesh_indexed(): whole')}; "
                f"mesh(): kernel against mesh_indexed(): kernels: {disjoint('mesh(): kernel', 'mesh_indexed(): kernels')}.\n\n")
        f.write("What this does not measure: kernel times apart from each other (no profiler run was made: the six launches of the "
                "indexed mesh and torch's sorts are inside one window each), a map that really rolled (the archive here is empty: "
                "the records all come from the table's export), other voxel sizes or tile sizes, and the per-batch host work in "
                "needed_records apart from absorb and the extraction.  No ratio is promised; the rows above are one session's.\n")
    print(open(path).read())


if __name__ == "__main__":
    main()
