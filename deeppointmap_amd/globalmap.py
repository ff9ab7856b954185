"""The end-of-run point-cloud map: what the reference's ResultLogger.draw_trajectory builds on the CPU with torch matmuls
and open3d's voxel_down_sample (system/modules/recoder.py:167-190), as one pass of HIP kernels over the device-resident
scan clouds (csrc/voxel_map.hip), and the binary PCD files that the reference's save_map body names.

  voxel_map(clouds, poses, voxel_size)  -> (centroids (3,M) fp32, counts (M,) int32) on the device
  write_pcd(path, xyz)                  binary PCD v0.7, x y z float32

Semantics (open3d PointCloud::VoxelDownSample, restated): min_b = min over all points - vs/2; voxel index =
floor((p - min_b) / vs) in fp64 from the fp32 transformed point; centroid = mean of the voxel's points (within 1.2e-10 m of
the fp64 mean before the final fp32 rounding).  Output order: first appearance in the concatenation (scan order, then point
order); open3d's is unspecified.  The result is bit-reproducible and independent of the order in which scans are given,
up to the output order.

Memory: dpm_voxel_map_workspace_bytes(N) <= 51 B per input point (+ 8 KB); it, the staging buffers and the per-scan arrays
are checked against the free device memory before they are allocated, the output (16 B per voxel) once the voxel count is
known; host-resident clouds pass through STAGING_POINTS-point pinned buffers (two, double-buffered on a copy
stream), twice: once for the bounds and once for the accumulation.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops

STAGING_POINTS = 1 << 20            # points per pinned staging buffer (12 MB; two of them)
MAX_WORKSPACE_BYTES_PER_POINT = 64  # the documented bound (the layout needs <= 51)
KEY_BITS = 21                       # per axis: 3 x 21 bits in a 63-bit voxel key


def _decode_ordered(u: np.ndarray) -> np.ndarray:
    """inverse of the kernel's order-preserving image of an fp32 value"""
    u = u.astype(np.uint32)
    bits = np.where(u & np.uint32(0x80000000), u ^ np.uint32(0x80000000), ~u).astype(np.uint32)
    return bits.view(np.float32)


def _pose_rows(poses) -> torch.Tensor:
    P = torch.stack([torch.as_tensor(p) for p in poses]) if isinstance(poses, (list, tuple)) else torch.as_tensor(poses)
    P = P.detach().to("cpu", torch.float32).reshape(-1, 4, 4)
    return torch.cat([P[:, :3, :3].reshape(-1, 9), P[:, :3, 3]], dim=1).contiguous()


def voxel_map(clouds: Sequence[Optional[torch.Tensor]], poses, voxel_size: float = 0.5, device=None,
              stats: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """clouds: (3,N_i) fp32 clouds (metres, channel-first; on the device or on the host, None / empty = no points),
    poses: (n,4,4) or a list of (4,4) SE3 (the scan -> world transform, SE3_pred) -> voxel-centroid map of the union of
    the transformed points: centroids (3,M) fp32 and counts (M,) int32 on the device, in order of first appearance.
    Raises ValueError for voxel_size <= 0, non-finite points, extents the 21-bit key cannot hold, or inputs beyond the
    fixed-point bound; MemoryError when the workspace does not fit.  stats (optional dict) receives the counters."""
    vs = float(voxel_size)
    if not (math.isfinite(vs) and vs > 0.0):
        raise ValueError(f"voxel_map: voxel_size must be finite and > 0, got {voxel_size}")
    P = _pose_rows(poses)
    if P.shape[0] != len(clouds):
        raise ValueError(f"voxel_map: {len(clouds)} clouds but {P.shape[0]} poses")
    if device is None:
        device = next((c.device for c in clouds if c is not None and c.is_cuda), None)
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    parts = []   # (cloud tensor (3,n), n, pose row index, on_device)
    for i, c in enumerate(clouds):
        if c is None or c.numel() == 0:
            continue
        if c.dim() != 2 or c.shape[0] != 3:
            raise ValueError(f"voxel_map: cloud {i} has shape {tuple(c.shape)}, expected (3, N)")
        if c.is_cuda:
            if c.device != device:
                raise ValueError(f"voxel_map: cloud {i} is on {c.device}, the map on {device}")
            parts.append((c.to(torch.float32).contiguous(), c.shape[1], i, True))
        else:
            c = c.to(torch.float32)
            for a in range(0, c.shape[1], STAGING_POINTS):      # a host cloud larger than a staging buffer is split
                parts.append((c[:, a:a + STAGING_POINTS], min(STAGING_POINTS, c.shape[1] - a), i, False))
    N = sum(p[1] for p in parts)
    empty = (torch.empty(3, 0, device=device, dtype=torch.float32), torch.empty(0, device=device, dtype=torch.int32))
    if stats is not None:
        stats.update(n_points=N, voxels=0, runs=0, cas=0, workspace_bytes=0, atomics_per_point=0.0)
    if N == 0:
        return empty
    if N > 0x7FFFFFFF:
        raise ValueError(f"voxel_map: {N} points; at most 2^31 - 1 per map")
    if N * (vs * 2.0 ** 32 + 2.0) >= 2.0 ** 62:
        raise ValueError(f"voxel_map: {N} points at voxel_size {vs} exceed the fixed-point bound N * (vs * 2^32 + 2) < 2^62")

    ws_bytes = ops.voxel_map_workspace_bytes(N)
    assert 0 < ws_bytes <= MAX_WORKSPACE_BYTES_PER_POINT * N + 8192, ws_bytes
    # device memory the call adds before the output exists: the workspace, the two device staging buffers (host clouds
    # only) and the per-scan pointer / offset / pose arrays.  fp32 / contiguous copies of device clouds are already in `parts`
    # (and in the allocator's numbers); the output, 16 B per voxel, is checked once the voxel count is known (_run).
    need = ws_bytes + (2 * 12 * STAGING_POINTS if any(not p[3] for p in parts) else 0) + len(parts) * (8 + 8 + 48) + 8
    with torch.cuda.device(device):
        _check_free(device, need, f"the workspace for {N} points")
        return _run(parts, P, N, vs, device, ws_bytes, stats)


def _check_free(device, need: int, what: str) -> None:
    free, _ = torch.cuda.mem_get_info(device)
    cached = torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
    if need > free + cached:
        raise MemoryError(f"voxel_map: {what} needs {need / 2**20:.1f} MiB, {(free + cached) / 2**20:.1f} MiB are free on {device}")


def _run(parts, P, N, vs, device, ws_bytes, stats):
    stream = torch.cuda.current_stream(device)
    ws = torch.empty(ws_bytes, device=device, dtype=torch.uint8)
    n_host = sum(not p[3] for p in parts)
    if n_host:
        pinned = [torch.empty(3 * STAGING_POINTS, dtype=torch.float32, pin_memory=True) for _ in range(2)]
        staged = [torch.empty(3 * STAGING_POINTS, device=device, dtype=torch.float32) for _ in range(2)]
        copy_stream = torch.cuda.Stream(device=device)
    # batches: runs of consecutive device clouds form one call; every host part is a call of its own, reading a staging
    # buffer.  All pointer / offset / pose arrays are built once and uploaded once.
    batches, ptrs, offs, rows = [], [], [], []
    k = 0
    for c, n, i, on_dev in parts:
        if on_dev and batches and batches[-1]["dev"]:
            b = batches[-1]
        else:
            b = dict(dev=on_dev, first=len(ptrs), off=len(offs), n_scans=0, n=0, parts=[],
                     slot=None if on_dev else k % 2)
            k += not on_dev
            batches.append(b)
            offs.append(0)
        ptrs.append(c.data_ptr() if on_dev else staged[b["slot"]].data_ptr())
        rows.append(i)
        b["n_scans"] += 1
        b["n"] += n
        b["parts"].append((c, n))
        offs.append(b["n"])
    ptr_t = torch.tensor(ptrs, dtype=torch.int64).to(device)
    off_t = torch.tensor(offs, dtype=torch.int64).to(device)
    pose_t = P[rows].contiguous().to(device)
    addr = lambda b: (ptr_t.data_ptr() + 8 * b["first"], off_t.data_ptr() + 8 * b["off"], pose_t.data_ptr() + 48 * b["first"])

    def sweep(launch):
        """every batch in order; host parts copied through the two staging buffers, overlapped with the kernels"""
        if n_host:
            copied = [torch.cuda.Event(), torch.cuda.Event()]   # H2D of the slot done (pinned buffer reusable)
            used = [torch.cuda.Event(), torch.cuda.Event()]     # kernel that read the slot done (device buffer reusable)
            for e in copied + used:
                e.record(stream)
        base = 0
        for b in batches:
            if not b["dev"]:
                s, (c, n) = b["slot"], b["parts"][0]
                copied[s].synchronize()
                pinned[s][:3 * n].view(3, n).copy_(c)
                with torch.cuda.stream(copy_stream):
                    copy_stream.wait_event(used[s])
                    staged[s][:3 * n].copy_(pinned[s][:3 * n], non_blocking=True)
                    copied[s].record(copy_stream)
                stream.wait_event(copied[s])
            launch(b, base)
            if not b["dev"]:
                used[b["slot"]].record(stream)
            base += b["n"]
        assert base == N

    ops.voxel_map_init(ws, N)
    sweep(lambda b, base: ops.voxel_map_bounds(ws, *addr(b), b["n_scans"], b["n"]))
    hdr = ws[:ops.VOXEL_MAP_HDR_BYTES].cpu().numpy()
    h32 = hdr.view(np.uint32)
    if h32[6]:
        raise ValueError(f"voxel_map: {int(h32[6])} non-finite coordinates among the transformed points")
    lo, hi = _decode_ordered(h32[0:3]).astype(np.float64), _decode_ordered(h32[3:6]).astype(np.float64)
    min_b = lo - vs / 2.0                                   # open3d: GetMinBound() - voxel_size / 2, in double
    top = np.floor((hi - min_b) / vs)
    if (top >= 2 ** KEY_BITS).any():
        raise ValueError(f"voxel_map: extent {(hi - lo).tolist()} m at voxel_size {vs} exceeds the 2^{KEY_BITS} voxels per "
                         "axis of the key packing")
    sweep(lambda b, base: ops.voxel_map_insert(ws, *addr(b), b["n_scans"], b["n"], base, N, min_b, vs))
    ops.voxel_map_finish(ws, N)
    hdr = ws[:ops.VOXEL_MAP_HDR_BYTES].cpu().numpy()
    h32, h64 = hdr.view(np.uint32), hdr.view(np.uint64)
    if h32[7]:
        raise _lib.DpmError(f"voxel_map: {int(h32[7])} points fell outside the checked key range")
    M = int(h32[8])
    _check_free(device, 16 * M, f"the map of {M} voxels")
    out = ops.voxel_map_emit(ws, N, min_b, vs, M)
    if stats is not None:
        runs, cas = int(h64[8]), int(h64[9])
        stats.update(voxels=M, runs=runs, cas=cas, workspace_bytes=ws_bytes, min_b=min_b.tolist(),
                     atomics_per_point=(5 * runs + cas) / N)
    return out


def write_pcd(path: str, xyz) -> None:
    """xyz (3,M) (tensor on any device, or array) -> binary PCD v0.7 with fields x y z, float32 (what open3d's
    write_point_cloud writes for a cloud without colours or normals, as binary)"""
    a = xyz.detach().cpu().numpy() if isinstance(xyz, torch.Tensor) else np.asarray(xyz)
    if a.ndim != 2 or a.shape[0] != 3:
        raise ValueError(f"write_pcd: expected (3, M), got {a.shape}")
    pts = np.ascontiguousarray(a.T.astype("<f4"))
    M = pts.shape[0]
    head = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\n"
            f"WIDTH {M}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {M}\nDATA binary\n")
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(pts.tobytes())
