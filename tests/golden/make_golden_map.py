#!/usr/bin/env python3
"""The REFERENCE's ResultLogger.draw_trajectory (system/modules/recoder.py:99-203) on a small hand-built PoseGraph ->
tests/golden/result_map.npz.  Runs only in the build container (imports /root/reference, read-only; colorlog, easydict and
readerwriterlock are stubbed as in make_trace.py; matplotlib runs on the Agg backend).

The graph: 12 scans of two agents (agent 0: 7, agent 1: 5, timesteps interleaved), key frames and non-key frames, clouds of
700-1 500 points, key points (8, 96) with xyz in the last three rows, one key frame whose full_pcd is None, SE3_gt on every
scan, and edges of all four types (odom, locz, loop, prxy).  draw_trajectory runs twice, draft=False and draft=True.
Recorded:
  * the scans and edges of the graph (what the test rebuilds a back end from);
  * every array handed to open3d's Vector3dVector (which points, transformed how, in what order) and every voxel size;
  * every ax.plot / ax.scatter call of both runs (tests/golden/map_calls.py: coordinates, colour, marker, ...).
open3d is absent here, so PointCloud.voxel_down_sample is a stub that returns the fp64 numpy restatement of open3d's
VoxelDownSample (tests/test_globalmap_host.voxel_down_sample_ref): the map layers pin which points the reference
down-samples and how it draws them, NOT open3d's voxel semantics (those are the restatement's)."""
import json
import logging
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from map_calls import recording  # noqa: E402
from test_globalmap_host import voxel_down_sample_ref  # noqa: E402

VOXEL_LOG = []      # (which, voxel_size, points handed to Vector3dVector)


class _PointCloud:
    def __init__(self):
        self.points = None

    def voxel_down_sample(self, voxel_size):
        pts = np.asarray(self.points)
        VOXEL_LOG[-1]["voxel_size"] = float(voxel_size)
        c, _, _, _ = voxel_down_sample_ref(pts.T.astype(np.float32), float(voxel_size))
        out = _PointCloud()
        out.points = c.T
        return out


def _vector3d(a):
    a = np.array(a, copy=True)
    VOXEL_LOG.append(dict(points=a))
    return a


o3d = types.ModuleType("open3d")
o3d.geometry = types.SimpleNamespace(PointCloud=_PointCloud)
o3d.utility = types.SimpleNamespace(Vector3dVector=_vector3d)
o3d.open3d = o3d
sys.modules["open3d"] = o3d
sys.modules["colorlog"] = logging
ed = types.ModuleType("easydict")
ed.EasyDict = dict
sys.modules["easydict"] = ed
rw, rwl = types.ModuleType("readerwriterlock"), types.ModuleType("readerwriterlock.rwlock")


class _L:
    def acquire(self, blocking=True):
        return True

    def release(self):
        pass


class RWLockFair:
    def gen_rlock(self):
        return _L()

    def gen_wlock(self):
        return _L()


rwl.RWLockFair = RWLockFair
rw.rwlock = rwl
sys.modules["readerwriterlock"], sys.modules["readerwriterlock.rwlock"] = rw, rwl
sys.path.insert(0, "/root/reference")
from system.modules.pose_graph import PoseGraph, PoseGraph_Edge, ScanPack  # noqa: E402
from system.modules.recoder import ResultLogger  # noqa: E402


def _se3(rng, pos, yaw):
    S = torch.eye(4)
    S[0, 0], S[0, 1], S[1, 0], S[1, 1] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw)
    S[:3, 3] = torch.tensor(pos, dtype=torch.float32)
    return S


def build(rng):
    pg = PoseGraph(args=None, agent_id=0, device="cpu")
    scans, edges = [], []
    plan = [(0, 0), (1, 0), (0, 1), (0, 2), (1, 1), (0, 3), (1, 2), (0, 4), (1, 3), (0, 5), (1, 4), (0, 6)]   # (agent, step)
    nonkey = {(0, 2), (0, 4), (1, 2)}
    pos = {0: np.array([0.0, 0.0, 0.0]), 1: np.array([30.0, -10.0, 0.5])}
    last_kf = {}
    for a, s in plan:
        pos[a] = pos[a] + np.array([rng.uniform(1.0, 4.0), rng.uniform(-1.5, 1.5), rng.uniform(-0.1, 0.1)])
        pred = _se3(rng, pos[a], rng.uniform(-np.pi, np.pi))
        gt = _se3(rng, pos[a] + rng.normal(scale=0.3, size=3), 0.0)
        n = int(rng.integers(700, 1500))
        ang = np.sort(rng.uniform(-np.pi, np.pi, n))
        r = rng.uniform(3.0, 25.0, n)
        pcd = torch.from_numpy(np.stack([r * np.cos(ang), r * np.sin(ang), rng.uniform(-1.7, 2.0, n)]).astype(np.float32))
        kp = torch.from_numpy(np.concatenate([rng.normal(size=(5, 96)), rng.uniform(-20, 20, size=(3, 96))]).astype(np.float32))
        if (a, s) == (1, 3):
            pcd = None                   # a key frame whose full cloud is gone
        sp = ScanPack(timestamp=s * 0.1, agent_id=a, timestep=s, key_points=kp, full_pcd=pcd, SE3_pred=pred, SE3_gt=gt,
                      coor_sys=a)
        if (a, s) in nonkey:
            sp = sp.nonkeyframe()
        pg.add_vertex(sp)
        scans.append(sp)
        if a in last_kf:
            ty = "locz" if (a, s) in nonkey else "odom"
            edges.append(PoseGraph_Edge(last_kf[a], sp.token, torch.eye(4), torch.eye(6), type=ty))
            pg.add_edge(edges[-1])
        if (a, s) not in nonkey:
            last_kf[a] = sp.token
    for src, dst, ty in (((0 << 16) + 0, (0 << 16) + 5, "loop"), ((1 << 16) + 0, (0 << 16) + 3, "prxy"),
                         ((0 << 16) + 6, (1 << 16) + 4, "loop"), ((1 << 16) + 1, (0 << 16) + 1, "prxy")):
        edges.append(PoseGraph_Edge(src, dst, torch.eye(4), torch.eye(6), type=ty))
        pg.add_edge(edges[-1])
    return pg, scans, edges


def main():
    rng = np.random.default_rng(2024)
    pg, scans, edges = build(rng)
    out = {}
    for i, sp in enumerate(scans):
        out[f"scan{i}.SE3_pred"] = sp.SE3_pred.numpy()
        out[f"scan{i}.SE3_gt"] = sp.SE3_gt.numpy()
        if sp.full_pcd is not None:
            out[f"scan{i}.full_pcd"] = sp.full_pcd.numpy()
        if sp.key_points is not None:
            out[f"scan{i}.key_points"] = sp.key_points.numpy()
    out["scan_token"] = np.array([sp.token for sp in scans], np.int64)
    out["scan_type"] = np.array([sp.type for sp in scans])
    out["edges"] = np.array([[e.src_scan_token, e.dst_scan_token] for e in edges], np.int64)
    out["edge_type"] = np.array([e.type for e in edges])
    for draft in (False, True):
        VOXEL_LOG.clear()
        with tempfile.TemporaryDirectory() as d, recording() as calls:
            ResultLogger(args=None, system_info=None, posegraph_map=pg, log_dir=d).draw_trajectory("t", draft=draft)
            assert os.path.exists(os.path.join(d, "t.map.jpg"))
        tag = "draft" if draft else "full"
        out[f"{tag}.calls"] = np.array(json.dumps(calls))
        if not draft:
            assert [v["voxel_size"] for v in VOXEL_LOG] == [0.5, 0.5]
            out["vector3d.full"], out["vector3d.key"] = (v["points"].astype(np.float32) for v in VOXEL_LOG)
            out["voxel_size"] = np.array([v["voxel_size"] for v in VOXEL_LOG])
        else:
            assert not VOXEL_LOG
    path = os.path.join(HERE, "result_map.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(json.loads(str(out["full.calls"]))), "calls (full),",
          len(json.loads(str(out["draft.calls"]))), "(draft)")


if __name__ == "__main__":
    main()
