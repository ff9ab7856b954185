"""Refined-pose tables for training: batched ICP on the GPU (csrc/icp.hip) and the per-scene table built from it.

The reference's training step takes every frame-to-map pose from a pickled `refined_SE3.pkl` per scene
(pipeline/modules/model_pipeline.py:199-282; dataloader/body.py:142-146 names the file) that nothing in the reference
writes: it was made offline with a third-party ICP.  `build_refined_table` makes such a table from a scene's scans and
global poses in the key convention `train_pipeline.refined_pose` reads: key (i, j) with i < j, value the refined pose of
frame j in frame i as a 4x4 float64 array.  What it is pinned to is this project's own float64 restatement of the same
algorithm and scenes with a known answer (tests/test_gpu_icp.py) -- not the third-party ICP, which cannot be run here.
"""
from __future__ import annotations

import pickle
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

POINT, PLANE = "point", "plane"
_METRIC = {POINT: ops.ICP_POINT, PLANE: ops.ICP_PLANE}
CONVERGED, MAX_ITER, NO_MATCH, SINGULAR = ops.ICP_CONVERGED, ops.ICP_MAX_ITER, ops.ICP_NO_MATCH, ops.ICP_SINGULAR
STATUS_NAMES = {CONVERGED: "CONVERGED", MAX_ITER: "MAX_ITER", NO_MATCH: "NO_MATCH", SINGULAR: "SINGULAR"}


class IcpResult(NamedTuple):
    """per pair: pose (P,4,4) float64 of the source in the target, fitness = matches / source points and rmse of the matches
    at the last evaluated pose (float32), iterations (steps taken) and status (int32)"""
    pose: torch.Tensor
    fitness: torch.Tensor
    rmse: torch.Tensor
    iterations: torch.Tensor
    status: torch.Tensor


def icp(pcd: torch.Tensor, lengths: torch.Tensor, src_frame: torch.Tensor, dst_frame: torch.Tensor, init: torch.Tensor,
        max_dist: float = 1.0, max_iter: int = 30, metric: str = PLANE, tol_rot: float = 1e-7, tol_trans: float = 1e-6,
        schedule: Optional[Sequence[Tuple[float, int]]] = None, normals: Optional[torch.Tensor] = None,
        normals_radius: float = 1.0) -> IcpResult:
    """Registers frame src_frame[p] of pcd (F,3,N) fp32 metres onto frame dst_frame[p], for all P pairs together, starting
    from init (P,4,4).  lengths (F,): valid leading points per frame.  schedule: [(max_dist, max_iter), ...] stages run back
    to back on the same grids (coarse to fine) instead of the single (max_dist, max_iter).  metric "plane" needs the
    targets' normals: pass `normals` (F,N,3), or leave it and they are computed here within normals_radius
    (ops.icp_target_normals; that reads the frame list on the host).  Everything else stays on the device."""
    if metric not in _METRIC:
        raise ValueError(f"metric must be 'point' or 'plane', got {metric!r}")
    stages = [(max_dist, max_iter)] if schedule is None else list(schedule)
    if not stages:
        raise ValueError("schedule: at least one (max_dist, max_iter) stage")
    init = init.to(device=pcd.device, dtype=torch.float64).contiguous()
    if metric == PLANE and normals is None:
        normals = ops.icp_target_normals(pcd, lengths, dst_frame, normals_radius)
    return IcpResult(*ops.icp_refine(pcd, lengths, src_frame, dst_frame, init, stages, _METRIC[metric], tol_rot, tol_trans,
                                     normals=normals))


def candidate_pairs(T, distance: float) -> np.ndarray:
    """T (n,3) or (n,3,1) ground-truth positions -> (m,2) int64 pairs i < j whose positions are within `distance`, in
    lexicographic order: the pairs a map of that radius can draw (dataloader/body.py:125 uses distance - 0.25)."""
    T = np.asarray(T, np.float64).reshape(-1, 3)
    out: List[np.ndarray] = []
    for i in range(len(T) - 1):
        d = np.linalg.norm(T[i + 1:] - T[i], axis=1)
        j = np.nonzero(d <= distance)[0] + i + 1
        out.append(np.stack([np.full(len(j), i, np.int64), j.astype(np.int64)], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)


def relative_poses(R, T, pairs) -> np.ndarray:
    """global poses R (n,3,3), T (n,3[,1]) -> (m,4,4) float64: frame j in frame i for every pair (i, j)"""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    T = np.asarray(T, np.float64).reshape(-1, 3)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    out = np.tile(np.eye(4), (len(pairs), 1, 1))
    Ri, Rj = R[pairs[:, 0]], R[pairs[:, 1]]
    out[:, :3, :3] = np.einsum("pki,pkj->pij", Ri, Rj)
    out[:, :3, 3] = np.einsum("pki,pk->pi", Ri, T[pairs[:, 1]] - T[pairs[:, 0]])
    return out


def accept(result: IcpResult, init, min_fitness: float, max_shift: float) -> np.ndarray:
    """(P,) bool: status CONVERGED or MAX_ITER, fitness >= min_fitness, and the refined translation within max_shift metres
    of the initial one -- everything else is left to the global poses, the reference's own fallback"""
    status = result.status.cpu().numpy()
    fitness = result.fitness.cpu().numpy()
    pose = result.pose.cpu().numpy()
    init = np.asarray(init.cpu() if isinstance(init, torch.Tensor) else init, np.float64)
    shift = np.linalg.norm(pose[:, :3, 3] - init[:, :3, 3], axis=1)
    return ((status == CONVERGED) | (status == MAX_ITER)) & (fitness >= min_fitness) & (shift <= max_shift) & \
        np.isfinite(pose).all(axis=(1, 2))


def build_refined_table(scans: torch.Tensor, R, T, pairs=None, *, distance: float = 20.0, batch_pairs: int = 64,
                        min_fitness: float = 0.3, max_shift: float = 2.0, lengths: Optional[torch.Tensor] = None,
                        **icp_kwargs) -> Dict[Tuple[int, int], np.ndarray]:
    """scans (F,3,N) fp32 metres on the GPU (lengths (F,) int32: valid points, default all N), global poses R (F,3,3),
    T (F,3[,1]) -> {(i, j): 4x4 float64 refined pose of frame j in frame i, i < j}.  pairs: (m,2), default
    candidate_pairs(T, distance).  Pair (i, j) starts from the global poses' frame j in frame i; entries that fail `accept`
    are left out.  Pairs run in batches of batch_pairs, so memory does not grow with the scene."""
    scans = scans.contiguous()
    F, _, N = scans.shape
    dev = scans.device
    if lengths is None:
        lengths = torch.full((F,), N, device=dev, dtype=torch.int32)
    R = R.detach().cpu().numpy() if isinstance(R, torch.Tensor) else R
    T = T.detach().cpu().numpy() if isinstance(T, torch.Tensor) else T
    pairs = candidate_pairs(T, distance) if pairs is None else np.asarray(pairs, np.int64).reshape(-1, 2)
    if len(pairs) and not ((pairs[:, 0] < pairs[:, 1]).all() and pairs.min() >= 0 and pairs.max() < F):
        raise ValueError("pairs: every pair must be (i, j) with 0 <= i < j < F")
    normals = None
    if icp_kwargs.get("metric", PLANE) == PLANE and len(pairs):   # once per scene: the targets are the pairs' first frames
        dst_all = torch.from_numpy(np.unique(pairs[:, 0]).astype(np.int32)).to(dev)
        normals = ops.icp_target_normals(scans, lengths, dst_all, icp_kwargs.pop("normals_radius", 1.0))
    table: Dict[Tuple[int, int], np.ndarray] = {}
    for a in range(0, len(pairs), batch_pairs):
        batch = pairs[a:a + batch_pairs]
        init = relative_poses(R, T, batch)
        src = torch.from_numpy(batch[:, 1].astype(np.int32)).to(dev)
        dst = torch.from_numpy(batch[:, 0].astype(np.int32)).to(dev)
        result = icp(scans, lengths, src, dst, torch.from_numpy(init), normals=normals, **icp_kwargs)
        keep = accept(result, init, min_fitness, max_shift)
        pose = result.pose.cpu().numpy()
        for k in np.nonzero(keep)[0]:
            table[(int(batch[k, 0]), int(batch[k, 1]))] = pose[k].copy()
    return table


def write_refined_table(path, table) -> None:
    """the plain pickle DeepPointModelPipeline loads: {(i, j): 4x4 float64 ndarray}"""
    with open(path, "wb") as f:
        pickle.dump({(int(i), int(j)): np.asarray(M, np.float64) for (i, j), M in table.items()}, f)


def read_refined_table(path) -> Dict[Tuple[int, int], np.ndarray]:
    with open(path, "rb") as f:
        return pickle.load(f)
