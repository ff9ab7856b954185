"""dpm_local_map_insert_frames restated in numpy on top of lidar_odometry_restated.Map, written from the contract
(include/dpm_hip.h; DESIGN §7k "Rebuilding the map"): a list of stored frames, each under a pose and a stamp, offered by
Map.insert's rule with the COLUMN of a point as its row number, and -- with a centre -- only where Map.prune's test would keep
the voxel.  float32 mirrors the kernel's operation order; the yardstick of tests/test_gpu_local_map_rebuild.py.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restated as I  # noqa: E402
import lidar_odometry_restated as L  # noqa: E402


def within(m, key, centre, radius):
    """Map.prune's test on keys (n,): the voxel's centre within `radius` of the centre's map-frame translation, in m.dtype"""
    dt = m.dtype
    t = L.map_pose(centre, m.origin)[:3, 3].astype(dt)
    r2 = dt(radius * radius)
    c = ((L.unpack_key(key).astype(dt) + dt(0.5)) * dt(m.voxel)).astype(dt)
    d = (c - t).astype(dt)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= r2


def insert_frames(m, store, lengths, frames, poses, stamps=None, centre=None, radius=None):
    """m: L.Map; store (capacity,3,P) float32, lengths (capacity,), frames (F,) rows, poses (F,4,4) float64, stamps (F,)
    (None: the rows).  -> the number of rows that passed the filter (each needs its voxel to have a slot)."""
    store = np.asarray(store, np.float32)
    P = store.shape[2]
    stamps = frames if stamps is None else stamps
    offered = 0
    for row, pose, stamp in zip(frames, np.asarray(poses, np.float64).reshape(-1, 4, 4), stamps):
        n = min(max(int(lengths[row]), 0), P)
        xyz = np.ascontiguousarray(store[row, :, :n].T)
        keep = m.gate(xyz)
        q = I.transform(L.map_pose(pose, m.origin), xyz, m.dtype)
        vox, sub, inside = L.cells(q, m.voxel, m.s, m.dtype)
        m.outside += int((keep & ~inside).sum())
        key = L.pack_key(vox)
        ok = keep & inside
        if centre is not None:
            ok &= within(m, key, centre, m.max_range if radius is None else radius)
        offered += int(ok.sum())
        for i in np.nonzero(ok)[0]:
            word = (int(stamp) << 32) | int(i)
            cell = m.vox.setdefault(int(key[i]), {})
            if int(sub[i]) not in cell or word < cell[int(sub[i])][0]:
                cell[int(sub[i])] = (word, q[i].copy())
    return offered


def sequential(m, store, lengths, frames, poses, stamps=None, centre=None, radius=None):
    """the defining identity's other side: Map.insert of each list entry with its stamp, then Map.prune(centre, radius)"""
    store = np.asarray(store, np.float32)
    P = store.shape[2]
    stamps = frames if stamps is None else stamps
    for row, pose, stamp in zip(frames, np.asarray(poses, np.float64).reshape(-1, 4, 4), stamps):
        n = min(max(int(lengths[row]), 0), P)
        m.insert(np.ascontiguousarray(store[row, :, :n].T), np.arange(n), pose, stamp)
    if centre is not None:
        m.prune(centre, m.max_range if radius is None else radius)
    return m
