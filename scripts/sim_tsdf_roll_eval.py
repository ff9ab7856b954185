"""The rolling TSDF tracker (deeppointmap_amd/tsdf.py: TsdfTracker(archive=...), TsdfMap.roll, TsdfArchive) over a simulated
circuit, in a table too small for the run: the frames of scripts/sim_tsdf_tracker_eval.py (street_scene(2), sweep motion
deskewed with the true motion, plane distance with normals estimated from each frame alone), tracked three times --
  whole     in 2^22 slots without an archive: the run as it was, and the number of voxels it ends with;
  small     without an archive in --slots slots (default: the largest power of two below that number), stopped at the first
            frame after which overflow() is non-zero: from there the map is undefined;
  rolling   with an archive in the same --slots slots: rolls, peak resident voxels, archive size, merged_export size, overflow().
For each: ATE against the exact poses and the frames lost.  The sensor reaches further (--sensor-range) than the map fuses
(--max-range), and a registration reads the field at every row: rows beyond the window read where the rolling map has sent its
tiles to the host, so its poses need not be the whole run's -- the difference is recorded.  Nothing is asserted.

  python scripts/sim_tsdf_roll_eval.py [--frames 240] [--spacing 1.0] [--voxel 0.5] [--max-range 40] [--slack 10] [--tile-bits 4] [--slots N]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--spacing", type=float, default=1.0)
    ap.add_argument("--beams", type=int, default=16)
    ap.add_argument("--columns", type=int, default=512)
    ap.add_argument("--sigma", type=float, default=0.02)
    ap.add_argument("--voxel", type=float, default=0.5)
    ap.add_argument("--normals-radius", type=float, default=1.0)
    ap.add_argument("--sensor-range", type=float, default=80.0)
    ap.add_argument("--max-range", type=float, default=40.0)
    ap.add_argument("--slack", type=float, default=10.0)
    ap.add_argument("--tile-bits", type=int, default=4)
    ap.add_argument("--slots", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sim_tsdf_roll_eval.py runs on a GPU; none is visible")
    from deeppointmap_amd import augment, evaluate, lidar_sim as LS, ops
    from deeppointmap_amd.tsdf import TsdfTracker, merged_export
    scene = LS.street_scene(2)
    model = LS.LidarModel(np.linspace(10.0, -20.0, a.beams), a.columns, 0.9, a.sensor_range, range_sigma=a.sigma)
    poses = LS.circuit(scene, spacing=a.spacing)[:a.frames]
    F = len(poses)
    rng = torch.Generator(device=DEV)
    rng.manual_seed(1)
    sim = LS.LidarSimulator(scene, model, rng=rng if a.sigma > 0 else None, device=DEV)
    P0, P1 = LS.sweep_poses(poses)
    frames = [augment.deskew(f, f.sweep_motion, time="column", azimuth_steps=model.azimuth_steps) for f in sim.frames(P0, poses_end=P1)]
    first_motion = LS.sweep_delta(poses[0], poses[1])
    kw = dict(voxel_size=a.voxel, max_range=a.max_range, device=DEV, distance="plane", kernel_scale=a.voxel)
    resident = lambda tr: ops.tsdf_export(tr.map.table, tr.map.max_voxels, 0)

    def run(tr, stop_when_full=False):
        """-> (frames tracked, resident voxels per frame, seconds)"""
        held, t0 = [], time.perf_counter()
        for k, f in enumerate(frames):
            tr.step(f, a.normals_radius, pose=poses[0] if k == 0 else poses[0] @ first_motion if k == 1 else None)
            held.append(resident(tr))
            if stop_when_full and tr.map.overflow():
                break
        torch.cuda.synchronize()
        return len(held), held, time.perf_counter() - t0

    whole = TsdfTracker(max_voxels=1 << 22, **kw)
    n_whole, held_whole, s_whole = run(whole)
    total = held_whole[-1]
    slots = a.slots or 1 << (int(total).bit_length() - 1)
    small = TsdfTracker(max_voxels=slots, **kw)
    n_small, held_small, s_small = run(small, stop_when_full=True)
    rolling = TsdfTracker(max_voxels=slots, archive=True, slack=a.slack, tile_bits=a.tile_bits, **kw)
    n_roll, held_roll, s_roll = run(rolling)
    merged = merged_export(rolling.map, rolling.archive)
    same = all(x.tobytes() == y.tobytes() for x, y in zip(merged, whole.map.export()))
    gap = np.linalg.norm(np.stack(rolling.poses)[:, :3, 3] - np.stack(whole.poses)[:, :3, 3], axis=1)
    reach = rolling.map.reach(a.tile_bits)

    def row(name, tr, n, held, secs, extra):
        est = np.stack(tr.poses)
        ate = evaluate.ate(est, poses[:n]) if np.isfinite(est).all() and n > 2 else None
        return (f"| {name} | {tr.map.max_voxels} | {n} of {F} | {max(held)} | {held[-1]} | {tr.map.overflow()} | {tr.lost} | "
                f"{ate['rmse'] if ate else float('nan'):.4f} | {secs:.1f} | {extra} |\n")
    path = os.path.join(ROOT, "profiles", "sim_tsdf_roll_eval.md")
    with open(path, "w") as f:
        f.write("# The rolling TSDF tracker in a table too small for the run\n\n")
        f.write(f"`python scripts/sim_tsdf_roll_eval.py --frames {a.frames} --spacing {a.spacing} --voxel {a.voxel} --max-range {a.max_range:g} "
                f"--slack {a.slack:g} --tile-bits {a.tile_bits}` on {torch.cuda.get_device_name(0)}: lidar_sim.street_scene(2), {F} poses of its "
                f"circuit {a.spacing} m apart, {a.beams} beams x {a.columns} columns reaching {a.sensor_range:g} m, range noise {a.sigma} m, sweep "
                f"motion deskewed with the true motion; TsdfTracker: voxel {a.voxel} m, plane distance with normals estimated within "
                f"{a.normals_radius} m, kernel_scale {a.voxel}, returns fused up to {a.max_range:g} m.  Rolling: tiles of 2^{a.tile_bits} voxels "
                f"({(1 << a.tile_bits) * a.voxel:g} m), reach {reach:.1f} m, load radius {reach + a.slack:.1f} m, keep radius {reach + 2 * a.slack:.1f} m, "
                f"a roll whenever the start pose is {a.slack / 2:g} m from the last roll's centre.  Recorded, nothing asserted.\n\n"
                "| run | slots | frames tracked | peak resident voxels | resident at the end | overflow() | frames lost | ATE rmse m | seconds | |\n"
                "|---|---|---|---|---|---|---|---|---|---|\n")
        f.write(row("whole (no archive)", whole, n_whole, held_whole, s_whole, f"{total} voxels at the end"))
        f.write(row("small (no archive)", small, n_small, held_small, s_small,
                    f"stopped after frame {n_small - 1}: the map is undefined" if small.map.overflow() else "did not overflow"))
        f.write(row("rolling", rolling, n_roll, held_roll, s_roll,
                    f"{rolling.rolls} rolls; {len(rolling.archive)} voxels in {len(rolling.archive.tiles)} tiles archived; merged_export "
                    f"{len(merged[0])} voxels"))
        f.write(f"\nThe rolling run's poses against the whole run's: largest distance {gap.max():.4f} m, at the end {gap[-1]:.4f} m; its "
                f"merged_export {'equals' if same else 'differs from'} the whole run's export byte for byte"
                f"{'' if same else ' (the poses differ, so different samples were fused)'}.  The sensor reaches {a.sensor_range:g} m and every "
                f"row is registered: rows more than the load radius from the last roll's centre read where the rolling map's tiles are "
                "on the host, which the guarantee of `TsdfMap.roll` leaves out.\n")
        f.write(f"\nResident voxels per twentieth frame:\n\n```\nwhole:   {held_whole[::20]}\nsmall:   {held_small[::20]}\nrolling: {held_roll[::20]}\n```\n")
    print(open(path).read())


if __name__ == "__main__":
    main()
