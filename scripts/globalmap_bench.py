"""The end-of-run global map at KITTI-00 size: 4 541 scans x 14 500 points (65.8 M points), voxel 0.5 m, all clouds on the
device (globalmap.voxel_map -> csrc/voxel_map.hip).  Prints one JSON line: ms per map (median of --reps after a warm-up),
points/s, the bytes the two streaming passes read against the HBM rate, atomics per point, peak device memory, and the
fp64 numpy restatement's time on the host for a tenth of the scans, for context.

  python scripts/globalmap_bench.py [--scans 4541] [--points 14500] [--reps 5] [--out result.json]

Synthetic scans are LiDAR-like: 64 rings x azimuth order over a street (ground plane, walls 6-10 m away, 80 m cap), the sensor driving a loop (poses advance ~1.3 m
per scan, so consecutive scans overlap as on a drive)."""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from deeppointmap_amd import globalmap

HBM_BYTES_PER_S = 8.0e12   # MI355X peak HBM3E rate


def scans(n_scans, n_pts, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    rings = 64
    az = n_pts // rings
    n = rings * az
    elev = torch.linspace(-0.43, 0.05, rings, device=dev).repeat_interleave(az)          # ring-major, then azimuth
    phi = torch.linspace(-math.pi, math.pi, az, device=dev).repeat(rings)
    clouds = torch.empty(n_scans, 3, n, device=dev)
    for a in range(0, n_scans, 256):
        b = min(n_scans, a + 256)
        # a street: ground 1.73 m below the sensor, walls 6-10 m to either side (varying per scan), 80 m range cap
        wall = 6.0 + 4.0 * torch.rand(b - a, 1, 1, device=dev, generator=g)
        r_ground = torch.where(elev < 0, 1.73 / torch.sin(-elev).clamp_min(1e-3), torch.full_like(elev, 1e9))
        r_wall = wall / (torch.cos(elev) * torch.sin(phi).abs()).clamp_min(1e-3)
        r = torch.minimum(torch.minimum(r_ground.expand_as(r_wall), r_wall), torch.full_like(r_wall, 80.0))
        r = r + 0.02 * torch.randn(b - a, 1, n, device=dev, generator=g)
        clouds[a:b, 0] = (r * torch.cos(elev) * torch.cos(phi))[:, 0]
        clouds[a:b, 1] = (r * torch.cos(elev) * torch.sin(phi))[:, 0]
        clouds[a:b, 2] = (r * torch.sin(elev))[:, 0]
    t = torch.arange(n_scans, dtype=torch.float64) * 1.3
    yaw = t / 600.0
    poses = torch.eye(4, dtype=torch.float64).repeat(n_scans, 1, 1)
    poses[:, 0, 0], poses[:, 0, 1], poses[:, 1, 0], poses[:, 1, 1] = yaw.cos(), -yaw.sin(), yaw.sin(), yaw.cos()
    poses[:, 0, 3], poses[:, 1, 3] = 600.0 * yaw.sin(), 600.0 * (1 - yaw.cos())
    return clouds, poses.float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=4541)
    ap.add_argument("--points", type=int, default=14500)
    ap.add_argument("--voxel", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-fraction", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    clouds, poses = scans(a.scans, a.points, dev)
    cl = list(clouds.unbind(0))
    N = clouds.shape[0] * clouds.shape[2]
    torch.cuda.synchronize()
    st = {}
    globalmap.voxel_map(cl, poses, a.voxel, stats=st)          # warm-up (and the counters)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        c, n = globalmap.voxel_map(cl, poses, a.voxel)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        del c, n
    peak = torch.cuda.max_memory_allocated(dev) - base
    ms = float(np.median(times))
    read = 2 * 12 * N                                          # the two streaming passes over the clouds
    res = dict(what="globalmap.voxel_map", scans=a.scans, points=N, voxel=a.voxel, voxels=int(st["voxels"]),
               ms_per_map=round(ms, 3), ms_all=[round(x, 3) for x in times], points_per_s=N / (ms * 1e-3),
               stream_bytes=read, stream_ms_at_hbm_peak=round(read / HBM_BYTES_PER_S * 1e3, 3),
               runs=int(st["runs"]), cas=int(st["cas"]), atomics_per_point=round(st["atomics_per_point"], 5),
               workspace_bytes=int(st["workspace_bytes"]), workspace_bytes_per_point=round(st["workspace_bytes"] / N, 2),
               peak_device_bytes=int(peak), peak_device_bytes_per_point=round(peak / N, 2))
    # the fp64 numpy restatement (tests/test_globalmap_host.py) on a fraction of the scans
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from test_globalmap_host import transform_fp32, voxel_down_sample_ref
    k = max(1, int(a.scans * a.host_fraction))
    hc, hp = clouds[:k].cpu().numpy(), poses[:k].numpy()
    t0 = time.perf_counter()
    world = np.concatenate([transform_fp32(hc[i], hp[i]) for i in range(k)], axis=1)
    voxel_down_sample_ref(world, a.voxel)
    host_s = time.perf_counter() - t0
    res.update(host_restatement_scans=k, host_restatement_s=round(host_s, 3),
               host_restatement_s_scaled_to_all=round(host_s * a.scans / k, 1))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
