"""Run evaluation: how good is a trajectory, how good is a map.

The reference has no counterpart for any of this (its ResultLogger writes a trajectory, a picture and nothing about
them); what this module computes is pinned to this project's own numpy restatement (tests/map_eval_restated.py: float32 bit
for bit, float64 within a bound) and to constructed cases with known answers, and to nothing else.

TRAJECTORY side -- numpy float64 on the host, no GPU (a trajectory is a few thousand poses).  Trajectories are (n,4,4)
sensor-to-world poses, `est[i]` and `gt[i]` the same scan.  Definitions:

* `align_trajectory(est, gt, mode)` -> S (4,4), applied as S @ est[i].  "se3": the rigid S that minimises
  sum |S p_est_i - p_gt_i|^2 over the POSITIONS (Kabsch / Umeyama without scale: SVD of the cross-covariance of the centred
  positions, the sign of the last singular vector flipped when det < 0 -- the reflection guard).  "first": S = gt[0] est[0]^-1.
  "none": the identity.
* `ate(est, gt, mode)`: the absolute trajectory error e_i = |S p_est_i - p_gt_i| after alignment -- rmse, mean, median, max
  (metres) -- and the angle of R_gt_i^T R_S R_est_i -- rot_mean, rot_max (radians).
* `rpe(est, gt, delta)`: E_i = (G_i^-1 G_{i+delta})^-1 (P_i^-1 P_{i+delta}) with G = gt, P = est, over i = 0 .. n-delta-1;
  trans_* = rmse / mean / max of |translation of E_i| (metres), rot_* of the angle of its rotation (radians).
* `kitti_odometry_error(est, gt, lengths, step)`: the KITTI odometry devkit's segment errors.  Path length from the gt
  positions (cumulative chord length); a start every `step` frames; for every length L the segment ends at the first frame
  whose path length is AT OR PAST the start's plus L (the devkit compares with >; on real data the two never differ, on a
  constructed path that lands exactly on L this one keeps the exact segment); with D_gt = gt[a]^-1 gt[b], D_est =
  est[a]^-1 est[b] and E = D_est^-1 D_gt: t_err = |translation of E| / L (a ratio; the devkit prints it times 100 as %),
  r_err = angle of E / L (rad/m).  Means over all segments, per-length rows, the segment count.  Lengths the path never
  reaches are skipped; with every length skipped the result is None, not NaN.

The angle of a rotation R is atan2(|R - R^T|_F / (2 sqrt 2), (tr R - 1) / 2), which keeps its accuracy near zero.

MAP side -- HIP kernels (csrc/map_eval.hip) on (3,M) fp32 channel-first clouds on the device, the layout
globalmap.voxel_map returns (a map is millions of points):

* `scene_distance(points, scene, origin)` -> (dist (M,), surf (M,)): distance to the nearest surface of a simulator `Scene`
  (lidar_sim.py) and its id, 0..P-1 a primitive, P the ground, -1 none: the EXACT yardstick a simulated run has and no real
  dataset offers.
* `cloud_nn(query, target, max_dist, origin)` -> (dist (Nq,), idx (Nq,)): exact nearest neighbour within max_dist.
* `distance_stats(dist, thresholds, max_dist, surf, class_id, n_classes)` -> (C+1, 5+T) float64 table on the device.
* `map_accuracy(map_xyz, scene, thresholds, max_dist)`: per class of the nearest surface and in total -- mean, rmse, max of
  the matched distances (a point is matched when its distance is finite and <= max_dist), the share of ALL the row's points
  within each threshold, the unmatched share.
* `map_to_map(est, ref, thresholds, max_dist)`: accuracy (est -> ref) and completeness (ref -> est) rows like the above,
  chamfer = accuracy mean + completeness mean, and per threshold precision (share of est points with a ref point within it),
  recall (share of ref points with an est point within it) and fscore = 2 P R / (P + R) (0 when both are 0).  The general
  yardstick: ref is the map of the SAME clouds under the ground-truth poses.

`origin`: three float64 numbers every point is shifted by ONCE, in float64, before anything is computed in fp32 -- so a map
a kilometre from the world's origin is evaluated as accurately as one around it.  None = the float64 centre of the points'
bounding box, which costs one read-back; pass an origin to stay free of host synchronisations (the functions above that
return tensors then make none; `map_accuracy` and `map_to_map` return numbers and read their small tables back).

`python -m deeppointmap_amd.evaluate est.txt gt.txt` prints the trajectory metrics of two KITTI-style files (twelve numbers
per line: what ResultLogger.save_trajectory writes) as JSON.
"""
from __future__ import annotations

import json
import math
import sys
from typing import Optional, Sequence

import numpy as np

DEFAULT_THRESHOLDS = (0.05, 0.1, 0.2, 0.5)
DEFAULT_MAX_DIST = 1.0
KITTI_LENGTHS = (100.0, 200.0, 300.0, 400.0, 500.0, 600.0, 700.0, 800.0)


# ------------------------------------------------------------------------------------------------------------
# trajectories (host, float64)
# ------------------------------------------------------------------------------------------------------------
def _traj(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    a = np.asarray(x, dtype=np.float64)
    if a.ndim == 2 and a.shape[1] == 12:
        a = np.concatenate([a.reshape(-1, 3, 4), np.tile([[[0.0, 0.0, 0.0, 1.0]]], (a.shape[0], 1, 1))], axis=1)
    if a.ndim != 3 or a.shape[1:] != (4, 4):
        raise ValueError(f"a trajectory is (n,4,4), got {a.shape}")
    return a


def _pair(est, gt):
    est, gt = _traj(est), _traj(gt)
    if est.shape != gt.shape or est.shape[0] < 1:
        raise ValueError(f"est {est.shape} and gt {gt.shape}: the same scans, at least one")
    return est, gt


def rotation_angle(R) -> np.ndarray:
    """angle (rad) of (...,3,3) rotations: atan2(|R - R^T|_F / (2 sqrt 2), (tr R - 1) / 2)"""
    R = np.asarray(R, np.float64)
    skew = R - np.swapaxes(R, -1, -2)
    return np.arctan2(np.sqrt((skew ** 2).sum(axis=(-1, -2))) / (2.0 * math.sqrt(2.0)), (np.trace(R, axis1=-2, axis2=-1) - 1.0) / 2.0)


def _inv(T: np.ndarray) -> np.ndarray:
    """inverse of (...,4,4) rigid transforms"""
    out = np.zeros_like(T)
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -(Rt @ T[..., :3, 3:])[..., 0]
    out[..., 3, 3] = 1.0
    return out


def align_trajectory(est, gt, mode: str = "se3") -> np.ndarray:
    """-> S (4,4) float64; the aligned trajectory is S @ est[i] (module docstring)"""
    est, gt = _pair(est, gt)
    S = np.eye(4)
    if mode == "none":
        return S
    if mode == "first":
        return gt[0] @ _inv(est[0])
    if mode != "se3":
        raise ValueError("mode is 'se3', 'first' or 'none'")
    p, q = est[:, :3, 3], gt[:, :3, 3]
    mp, mq = p.mean(axis=0), q.mean(axis=0)
    H = (q - mq).T @ (p - mp)                       # sum q' p'^T
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U @ Vt) >= 0 else -1.0])
    R = U @ D @ Vt
    S[:3, :3], S[:3, 3] = R, mq - R @ mp
    return S


def _summary(prefix: str, v: np.ndarray, median: bool = False) -> dict:
    out = {prefix + "rmse": float(np.sqrt((v ** 2).mean())), prefix + "mean": float(v.mean()), prefix + "max": float(v.max())}
    if median:
        out[prefix + "median"] = float(np.median(v))
    return out


def ate(est, gt, mode: str = "se3") -> dict:
    """absolute trajectory error after `align_trajectory(est, gt, mode)`: rmse, mean, median, max (m), rot_mean, rot_max (rad), n"""
    est, gt = _pair(est, gt)
    A = align_trajectory(est, gt, mode) @ est
    e = np.linalg.norm(A[:, :3, 3] - gt[:, :3, 3], axis=1)
    ang = rotation_angle(np.swapaxes(gt[:, :3, :3], -1, -2) @ A[:, :3, :3])
    out = _summary("", e, median=True)
    out.update(rot_mean=float(ang.mean()), rot_max=float(ang.max()), n=int(len(e)), align=mode)
    return out


def rpe(est, gt, delta: int = 1) -> Optional[dict]:
    """relative pose error over `delta` frames: trans_rmse / _mean / _max (m), rot_rmse / _mean / _max (rad), n; None when
    the trajectory has no pair `delta` apart"""
    est, gt = _pair(est, gt)
    delta = int(delta)
    if delta < 1:
        raise ValueError("delta >= 1")
    if est.shape[0] <= delta:
        return None
    E = _inv(_inv(gt[:-delta]) @ gt[delta:]) @ (_inv(est[:-delta]) @ est[delta:])
    out = _summary("trans_", np.linalg.norm(E[:, :3, 3], axis=1))
    out.update(_summary("rot_", rotation_angle(E[:, :3, :3])))
    out.update(n=int(E.shape[0]), delta=delta)
    return out


def kitti_odometry_error(est, gt, lengths: Sequence[float] = KITTI_LENGTHS, step: int = 10) -> Optional[dict]:
    """KITTI segment errors (module docstring): t_err (ratio), r_err (rad/m), per_length [{length, t_err, r_err, n}],
    segments; None when the path reaches none of the lengths"""
    est, gt = _pair(est, gt)
    step = int(step)
    if step < 1 or not len(lengths) or min(lengths) <= 0:
        raise ValueError("step >= 1 and positive lengths")
    pos = gt[:, :3, 3]
    dist = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(pos, axis=0), axis=1))])
    rows, t_all, r_all = [], [], []
    for L in lengths:
        t_err, r_err = [], []
        for a in range(0, len(dist), step):
            b = int(np.searchsorted(dist, dist[a] + float(L), side="left"))     # first frame at or past
            if b >= len(dist):
                break
            E = _inv(_inv(est[a]) @ est[b]) @ (_inv(gt[a]) @ gt[b])
            t_err.append(float(np.linalg.norm(E[:3, 3])) / float(L))
            r_err.append(float(rotation_angle(E[:3, :3])) / float(L))
        if t_err:
            rows.append(dict(length=float(L), t_err=float(np.mean(t_err)), r_err=float(np.mean(r_err)), n=len(t_err)))
            t_all += t_err
            r_all += r_err
    if not rows:
        return None
    return dict(t_err=float(np.mean(t_all)), r_err=float(np.mean(r_all)), per_length=rows, segments=len(t_all), step=step)


def trajectory_metrics(est, gt, mode: str = "se3", delta: int = 1, lengths: Sequence[float] = KITTI_LENGTHS, step: int = 10) -> dict:
    """ate, rpe and the KITTI segment errors of one trajectory in one dict"""
    est, gt = _pair(est, gt)
    return dict(n=int(est.shape[0]), ate=ate(est, gt, mode), rpe=rpe(est, gt, delta), kitti=kitti_odometry_error(est, gt, lengths, step))


def load_kitti_trajectory(path) -> np.ndarray:
    """twelve numbers per line (the first three rows of the pose: what ResultLogger.save_trajectory writes) -> (n,4,4)"""
    a = np.loadtxt(str(path), dtype=np.float64, ndmin=2)
    if a.shape[1] != 12:
        raise ValueError(f"{path}: expected 12 numbers per line, got {a.shape[1]}")
    return _traj(a)


# ------------------------------------------------------------------------------------------------------------
# maps (GPU)
# ------------------------------------------------------------------------------------------------------------
def scene_records(scene, origin) -> np.ndarray:
    """(P,12) float32 records of dpm_scene_distance (include/dpm_hip.h), prepared in float64 and rounded once: centre -
    origin, cos and sin of the yaw (a cylinder: 1, 0), the extents (a box: half extents; a cylinder: radius, HALF height, 0,
    its centre moved to the middle of the axis), the kind as bits, padding"""
    from . import ops
    q, kind = scene.params, scene.kind
    o = np.asarray(origin, np.float64).reshape(3)
    box = kind == 0
    rec64 = np.zeros((scene.P, ops.MAP_EVAL_REC), np.float64)
    rec64[:, 0:2] = q[:, 0:2] - o[:2]
    rec64[:, 2] = np.where(box, q[:, 2], q[:, 2] + 0.5 * q[:, 4]) - o[2]
    rec64[:, 3] = np.where(box, np.cos(q[:, 6]), 1.0)
    rec64[:, 4] = np.where(box, np.sin(q[:, 6]), 0.0)
    rec64[:, 5] = q[:, 3]
    rec64[:, 6] = np.where(box, q[:, 4], 0.5 * q[:, 4])
    rec64[:, 7] = np.where(box, q[:, 5], 0.0)
    rec = np.ascontiguousarray(rec64.astype(np.float32))
    rec.view(np.int32)[:, 8] = kind
    return rec


def bounding_box_centre(*clouds):
    """the float64 centre of the bounding box of the finite points of (3,N) device clouds: ONE read-back"""
    import torch
    lo, hi = [], []
    for c in clouds:
        if c.numel() == 0:
            continue
        ok = torch.isfinite(c).all(dim=0, keepdim=True)
        lo.append(torch.where(ok, c, torch.full_like(c, math.inf)).amin(dim=1))
        hi.append(torch.where(ok, c, torch.full_like(c, -math.inf)).amax(dim=1))
    if not lo:
        return [0.0, 0.0, 0.0]
    b = torch.stack([torch.stack(lo).amin(dim=0), torch.stack(hi).amax(dim=0)]).double().cpu().numpy()
    mid = 0.5 * (b[0] + b[1])
    return [float(v) if math.isfinite(v) else 0.0 for v in mid]


def _cloud(x, name: str):
    import torch
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[0] != 3:
        raise ValueError(f"{name}: a (3,N) tensor")
    return x.to(torch.float32).contiguous()


def scene_distance(points, scene, origin=None):
    """-> (dist (M,) fp32, surf (M,) int32) on the points' device (module docstring)"""
    import torch
    from . import ops
    points = _cloud(points, "points")
    origin = bounding_box_centre(points) if origin is None else [float(v) for v in origin]
    rec = torch.from_numpy(scene_records(scene, origin)).to(points.device)
    ground = None if scene.z0 is None else scene.z0 - origin[2]
    return ops.scene_distance(points, rec, ground, origin)


def cloud_nn(query, target, max_dist: float, origin=None):
    """-> (dist (Nq,) fp32, idx (Nq,) int32) on the query's device (module docstring)"""
    from . import ops
    query, target = _cloud(query, "query"), _cloud(target, "target")
    origin = bounding_box_centre(query, target) if origin is None else origin
    return ops.cloud_nn(query, target, max_dist, origin)


def distance_stats(dist, thresholds=DEFAULT_THRESHOLDS, max_dist: float = DEFAULT_MAX_DIST, surf=None, class_id=None,
                   n_classes: int = 0):
    """-> (n_classes + 1, 5 + T) float64 on the device: rows = classes then the total; columns = matched, unmatched, sum d,
    sum d^2, max d, count with d <= thresholds[t] (ops.distance_stats)"""
    from . import ops
    return ops.distance_stats(dist, list(thresholds), max_dist, surf=surf, class_id=class_id, n_classes=n_classes)


def stats_row(row, thresholds) -> dict:
    """one row of the statistics table as numbers: n, matched, unmatched_share, mean, rmse, max (None without a matched
    point), within {threshold: share of the row's n points}"""
    row = [float(v) for v in row]
    matched, unmatched = row[0], row[1]
    n = matched + unmatched
    out = dict(n=int(n), matched=int(matched), unmatched_share=(unmatched / n) if n else None,
               mean=(row[2] / matched) if matched else None, rmse=math.sqrt(row[3] / matched) if matched else None,
               max=row[4] if matched else None)
    out["within"] = {f"{float(t):g}": ((row[5 + k] / n) if n else None) for k, t in enumerate(thresholds)}
    return out


def map_accuracy(map_xyz, scene, thresholds=DEFAULT_THRESHOLDS, max_dist: float = DEFAULT_MAX_DIST, origin=None) -> dict:
    """a map against the scene it was scanned from: {"classes": {name: row}, "total": row}, the class being that of the
    nearest surface (lidar_sim.CLASS_NAMES), rows as `stats_row`"""
    import torch
    from . import lidar_sim
    dist, surf = scene_distance(map_xyz, scene, origin)
    class_id = np.concatenate([scene.class_id, [lidar_sim.GROUND]]).astype(np.int32)
    C = int(class_id.max()) + 1
    tab = distance_stats(dist, thresholds, max_dist, surf=surf, class_id=torch.from_numpy(class_id).to(dist.device),
                         n_classes=C).cpu().numpy()
    names = [lidar_sim.CLASS_NAMES.get(c, str(c)) for c in range(C)]
    return dict(classes={names[c]: stats_row(tab[c], thresholds) for c in range(C)}, total=stats_row(tab[C], thresholds),
                thresholds=[float(t) for t in thresholds], max_dist=float(max_dist))


def map_to_map(est, ref, thresholds=DEFAULT_THRESHOLDS, max_dist: float = DEFAULT_MAX_DIST, origin=None) -> dict:
    """an estimated map against a reference map: accuracy (est -> ref), completeness (ref -> est), chamfer, and per
    threshold precision / recall / fscore (module docstring)"""
    est, ref = _cloud(est, "est"), _cloud(ref, "ref")
    origin = bounding_box_centre(est, ref) if origin is None else origin
    d_acc, _ = cloud_nn(est, ref, max_dist, origin)
    d_cmp, _ = cloud_nn(ref, est, max_dist, origin)
    acc = stats_row(distance_stats(d_acc, thresholds, max_dist).cpu().numpy()[0], thresholds)
    cmp_ = stats_row(distance_stats(d_cmp, thresholds, max_dist).cpu().numpy()[0], thresholds)
    out = dict(accuracy=acc, completeness=cmp_, thresholds=[float(t) for t in thresholds], max_dist=float(max_dist),
               chamfer=(acc["mean"] + cmp_["mean"]) if acc["mean"] is not None and cmp_["mean"] is not None else None,
               precision={}, recall={}, fscore={})
    for key in acc["within"]:
        p, r = acc["within"][key], cmp_["within"][key]
        out["precision"][key], out["recall"][key] = p, r
        out["fscore"][key] = None if p is None or r is None else (2.0 * p * r / (p + r) if p + r > 0 else 0.0)
    return out


# ------------------------------------------------------------------------------------------------------------
def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m deeppointmap_amd.evaluate", description="trajectory metrics of two KITTI-style files")
    ap.add_argument("est"), ap.add_argument("gt")
    ap.add_argument("--align", default="se3", choices=["se3", "first", "none"])
    ap.add_argument("--delta", type=int, default=1)
    ap.add_argument("--step", type=int, default=10)
    a = ap.parse_args(argv)
    print(json.dumps(trajectory_metrics(load_kitti_trajectory(a.est), load_kitti_trajectory(a.gt), a.align, a.delta, step=a.step)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
