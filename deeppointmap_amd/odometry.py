"""A geometric LiDAR odometry on the GPU: a rolling hashed voxel map and robust ICP of every scan against it
(csrc/local_map.hip), in the KISS-ICP family: point-to-point rows, or point-to-plane rows on one plane per voxel, and
optionally KISS-ICP's adaptive gate.  The reference has no counterpart: its poses come from the learned pipeline
only.  Here it gives the evaluation tools (evaluate.py) a system to judge, the learned pipeline a baseline, the deskew
(augment.deskew) its motion source without ground truth, and refine.build_refined_table global poses to start from.

`LocalMap` is the map: insert, prune, planes, register, read-back.  Its content is a function of the inserted points alone
(DESIGN §7j): a sub-cell of a voxel keeps the point of the oldest frame, and within a frame of the smallest original row.
`insert_frames` / `rebuild` make it from a list of stored frames with a pose each (after a loop correction).
`LidarOdometry.step` is one frame: constant-velocity prediction on the host, optional deskew with that prediction, thinning
with augment.voxel_sample, then register -> insert -> prune queued on the device pose, and ONE read-back.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import augment, ops
from .refine import CONVERGED, MAX_ITER, NO_MATCH, SINGULAR, STATUS_NAMES, IcpResult  # noqa: F401

OVERFLOW = "the local map is full (max_voxels={}): points found no free slot and the map is undefined; raise max_voxels or prune"


def _pose_tensor(pose, dev) -> torch.Tensor:
    """(4,4) float64 on the device from numpy / a tensor anywhere"""
    p = torch.from_numpy(np.ascontiguousarray(pose, dtype=np.float64)) if not isinstance(pose, torch.Tensor) else pose
    if tuple(p.shape) != (4, 4):
        raise ValueError("pose: (4,4)")
    return p.to(device=dev, dtype=torch.float64).contiguous()


class _HashedMap:
    """What LocalMap and tsdf.TsdfMap are alike in: a table made at first use, an origin that defaults to the translation of
    the first pose, lists of stored frames and the header's counters.  A subclass has max_voxels, origin, device, table and
    _new() -> an empty table on self.device."""

    def _ready(self, dev, pose=None):
        if self.table is None:
            self.device = dev if self.device is None else torch.device(self.device)
            self.table = self._new()
        if self.origin is None:
            if pose is None:
                self.origin = np.zeros(3)
            else:
                if isinstance(pose, torch.Tensor) and pose.is_cuda:   # only here: give `origin` to keep the pose on the device
                    augment._SYNCS[0] += 1
                    pose = pose.detach().cpu().numpy()
                self.origin = np.asarray(pose, np.float64).reshape(4, 4)[:3, 3].copy()

    @staticmethod
    def _list(what, store, frames, poses):
        """-> (rows (F,) int32 on the device, poses (F,4,4)) of a list of stored frames, checked: host rows are uploaded
        (nothing is read back), rows on the device are taken as they are"""
        dev = store.device
        if isinstance(frames, torch.Tensor):
            rows = frames.to(device=dev, dtype=torch.int32).contiguous()
        else:
            host = np.asarray(frames, np.int64).reshape(-1)
            if host.size and not (0 <= host.min() and host.max() < store.shape[0]):
                raise ValueError(f"{what}: frames are rows of the store")
            rows = torch.from_numpy(host.astype(np.int32)).to(dev)
        if not isinstance(poses, torch.Tensor):
            poses = torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 4, 4))
        if poses.numel() != 16 * rows.numel() or rows.numel() > 65535:
            raise ValueError(f"{what}: poses (F,4,4), F <= 65535")
        return rows, poses

    def _header(self, word: int) -> int:
        """32-bit word `word` of the table's header, unsigned; 0 before the table exists.  One host synchronisation."""
        if self.table is None:
            return 0
        augment._SYNCS[0] += 1
        return int(self.table[4 * word:4 * word + 4].view(torch.int32).item()) & 0xFFFFFFFF


class LocalMap(_HashedMap):
    """A rolling voxel map of `max_voxels` slots (a power of two) with voxels of `voxel_size` metres cut into
    subdivisions^3 sub-cells of one point each.  Coordinates are kept in fp32 relative to `origin` (three float64; default:
    the translation of the first inserted pose), so work far from the world's zero keeps fp32 accuracy.  Points are
    offered when min_range <= |p| <= max_range in the sensor frame.  A map that ran out of slots is undefined: `overflow`
    is then non-zero and every read-back (`points`, `n_points`, `check`, `export_planes`) raises ValueError.
    plane_radius: a voxel's plane is fitted to the map points within this distance of its centre (default and at most
    1.5 * voxel_size: the ball must lie inside the 27 voxels around it)."""

    def __init__(self, voxel_size: float = 1.0, subdivisions: int = 3, max_voxels: int = 1 << 17, max_range: float = 100.0,
                 min_range: float = 0.0, origin=None, device=None, plane_radius: Optional[float] = None):
        if not voxel_size > 0 or subdivisions not in (1, 2, 3):
            raise ValueError("voxel_size > 0 and subdivisions in 1, 2, 3")
        if max_voxels < 2 or max_voxels > 1 << 24 or max_voxels & (max_voxels - 1):
            raise ValueError("max_voxels: a power of two in [2, 2^24]")
        if not 0.0 <= min_range <= max_range:
            raise ValueError("0 <= min_range <= max_range")
        self.voxel_size, self.subdivisions, self.max_voxels = float(voxel_size), int(subdivisions), int(max_voxels)
        self.max_range, self.min_range = float(max_range), float(min_range)
        self.origin = None if origin is None else np.asarray(origin, np.float64).reshape(3).copy()
        self.device = device
        self.table: Optional[torch.Tensor] = None
        self.half, self.stamp = 0, 0
        self.plane_radius = 1.5 * float(np.float32(self.voxel_size)) if plane_radius is None else float(plane_radius)
        if not 0.0 < self.plane_radius <= 1.5 * float(np.float32(self.voxel_size)):
            raise ValueError("0 < plane_radius <= 1.5 * voxel_size (a voxel's plane looks into the 27 voxels around it)")
        self._planes = None          # (planes, counts) of the current half, per slot: a cache derived from the map
        self._planes_stale = True    # set by insert and prune, so the host knows without a read

    # -- plumbing (_ready, _list and _header are _HashedMap's)
    def _new(self):
        return ops.local_map_new(self.max_voxels, self.subdivisions, self.device)

    def _args(self):
        return self.table, self.max_voxels, self.subdivisions, self.half, self.voxel_size, self.origin

    # -- the device operations: no host synchronisation
    def insert(self, pcd, pose):
        """the frame's valid rows under `pose` (4,4; numpy, or a tensor -- on the GPU it is read there, behind whatever wrote
        it); the rule sees the rows' `idx`.  Two launches."""
        self._ready(pcd.device, pose)
        if pcd.cap == 0:
            return self
        ops.local_map_insert(*self._args(), pcd.xyz, pcd.idx, pcd.count, _pose_tensor(pose, self.device), self.stamp,
                             self.min_range, self.max_range)
        self.stamp += 1
        self._planes_stale = True
        return self

    def prune(self, pose, radius: Optional[float] = None):
        """keep the voxels whose centre lies within `radius` (default max_range) of the pose's translation"""
        self._ready(self.device if self.device is not None else augment._device(), pose)
        ops.local_map_prune(*self._args(), _pose_tensor(pose, self.device), self.max_range if radius is None else float(radius))
        self.half = 1 - self.half
        self._planes_stale = True
        return self

    def insert_frames(self, store, lengths, frames, poses, stamps=None, centre=None, radius=None):
        """stored frames under a pose each, in two launches for any number of them: row frames[f] of `store` (capacity,3,P)
        fp32 channel-major / `lengths` (capacity,) int32 on the device (LoopCloser.store, .lengths) under poses[f] (F,4,4;
        sensor -> world), stamped stamps[f] (host integers, pairwise distinct; None: the rows themselves); the rule sees the
        COLUMN of a point as its row number.  frames / poses: host arrays (uploaded, nothing is read back) or device tensors;
        frames on the device need `stamps`.  centre (4,4): only voxels that `prune(centre, radius)` would keep are offered
        (radius None: max_range), so the result is that of `insert` of each frame with its stamp, in any order, and that
        prune -- without the slots the dropped voxels would have taken first.  Adds to the current half."""
        if stamps is None:
            if isinstance(frames, torch.Tensor):
                raise ValueError("insert_frames: frames on the device need stamps (host integers)")
            stamps = frames
        stamps = [int(s) for s in np.asarray(stamps).reshape(-1)]
        if len(set(stamps)) != len(stamps) or any(not 0 <= s < 0xFFFFFFFF for s in stamps):
            raise ValueError("insert_frames: stamps pairwise distinct, in [0, 2^32 - 1)")
        rows, poses = self._list("insert_frames", store, frames, poses)
        if len(stamps) != rows.numel():
            raise ValueError("insert_frames: one stamp per frame")
        first = centre if centre is not None else (poses.reshape(-1, 4, 4)[0] if rows.numel() else None)
        self._ready(store.device, first)
        if rows.numel() == 0:
            return self
        ops.local_map_insert_frames(*self._args(), store, lengths, rows, poses.to(device=self.device, dtype=torch.float64).contiguous(),
                                    torch.from_numpy(np.array(stamps, np.uint32).view(np.int32)).to(self.device),
                                    None if centre is None else _pose_tensor(centre, self.device),
                                    self.max_range if radius is None else float(radius), self.min_range, self.max_range)
        self.stamp = max(self.stamp, max(stamps) + 1)
        self._planes_stale = True
        return self

    def rebuild(self, store, lengths, frames, poses, centre, radius=None):
        """the map emptied (both halves, the header; `origin` is kept) and made anew from stored frames around `centre`:
        `insert_frames` into half 0.  No host synchronisation."""
        self._ready(store.device, centre)
        ops.local_map_clear(self.table, self.max_voxels, self.subdivisions)
        self.half = 0
        self._planes_stale = True
        return self.insert_frames(store, lengths, frames, poses, centre=centre, radius=radius)

    def planes(self):
        """(planes (max_voxels,4) float32 (normal, w), counts (max_voxels,) int32) on the device, per SLOT of the current
        half: one plane per held voxel (csrc/local_map.hip), w = smallest / middle eigenvalue, -1 where no plane is defined.
        Recomputed in one launch when the map has changed since the last call; the tensors are reused."""
        self._ready(self.device if self.device is not None else augment._device())
        if self._planes_stale or self._planes is None:
            self._planes = ops.local_map_planes(*self._args(), self.plane_radius, *(self._planes or (None, None)))
            self._planes_stale = False
        return self._planes

    def register(self, pcd, init, schedule: Sequence[Tuple[float, int]] = ((1.0, 30),), kernel_scale: float = 0.0,
                 tol_rot: float = 1e-7, tol_trans: float = 1e-6, debug: bool = False, metric: str = "point",
                 min_points: int = 5, max_ratio: float = 0.1):
        """ICP of the frame against the map from `init` (4,4) over schedule = [(max_dist <= voxel_size, max_iter), ...] ->
        refine.IcpResult with one problem (pose (1,4,4) float64, ...), all on the device[, (key, sub, system) with debug].
        metric "point": point-to-point rows.  "plane": the row of a match is its distance along the plane of the matched
        point's voxel (`planes()`), given only when that plane rests on >= min_points points and is flat, 0 <= w <= max_ratio;
        other matches give nothing, and debug's key and sub are -1 for them."""
        if metric not in ("point", "plane"):
            raise ValueError("metric is 'point' or 'plane'")
        if any(float(d) > float(np.float32(self.voxel_size)) for d, _ in schedule):
            raise ValueError("register: every max_dist of the schedule must be <= voxel_size (the search looks into 27 voxels)")
        self._ready(pcd.device, init)
        if metric == "plane":
            planes, counts = self.planes()
            out = ops.local_map_register_planes(*self._args(), planes, counts, min_points, max_ratio, pcd.xyz, pcd.count,
                                                _pose_tensor(init, self.device), schedule, kernel_scale, tol_rot, tol_trans,
                                                debug=debug)
        else:
            out = ops.local_map_register(*self._args(), pcd.xyz, pcd.count, _pose_tensor(init, self.device), schedule,
                                         kernel_scale, tol_rot, tol_trans, debug=debug)
        res = IcpResult(out[0].reshape(1, 4, 4), *out[1:5])
        return (res, out[5:]) if debug else res

    # -- read-back: host synchronisations
    @property
    def overflow(self) -> int:
        """points that found no free slot so far (0: the map is defined)"""
        return self._header(0)

    def check(self):
        n = self.overflow
        if n:
            raise ValueError(OVERFLOW.format(self.max_voxels) + f" ({n} points)")

    @property
    def n_points(self) -> int:
        if self.table is None:
            return 0
        self.check()
        augment._SYNCS[0] += 1
        return ops.local_map_export(self.table, self.max_voxels, self.subdivisions, self.half, max_out=0)

    def export(self, check: bool = True):
        """(key (n,) int64, sub (n,) int32, owner (n,) int64, xyz (n,3) float32 map-frame) numpy, sorted by (key, sub-cell):
        the same bytes whatever the order the points arrived in"""
        if self.table is None:
            return np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros((0, 3), np.float32)
        if check:
            self.check()
        augment._SYNCS[0] += 2
        keys, sub, owner, xyz = [t.cpu().numpy() for t in ops.local_map_export(self.table, self.max_voxels, self.subdivisions, self.half)]
        order = np.lexsort((sub, keys))
        return keys[order], sub[order], owner[order], xyz[order]

    def points(self) -> np.ndarray:
        """(n,3) float64 world coordinates in the export's order"""
        xyz = self.export()[3]
        return xyz.astype(np.float64) + (self.origin if self.origin is not None else 0.0)

    def export_planes(self):
        """(key (m,) int64, count (m,) int32, normal (m,3) float32, w (m,) float32) numpy of the held voxels, sorted by key:
        the same bytes whatever the order the points arrived in and whichever slots the voxels sit in"""
        if self.table is None:
            return np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros((0, 3), np.float32), np.zeros(0, np.float32)
        self.check()
        planes, counts = self.planes()
        S = self.subdivisions ** 3
        at = 256 + self.half * (self.max_voxels * 8 + self.max_voxels * S * 24)
        augment._SYNCS[0] += 3
        keys = self.table[at:at + 8 * self.max_voxels].view(torch.int64).cpu().numpy()
        planes, counts = planes.cpu().numpy(), counts.cpu().numpy()
        held = np.nonzero(keys != -1)[0]
        held = held[np.argsort(keys[held], kind="stable")]
        return keys[held], counts[held], planes[held, :3].copy(), planes[held, 3].copy()


def adaptive_sigma(deviations, sigma0: float, min_motion: float = 0.0) -> float:
    """KISS-ICP's adaptive threshold: sqrt(mean d^2) over the deviations d > min_motion (metres; how far the registered pose
    lay from the predicted one), `sigma0` while there is none"""
    d = [float(x) for x in deviations if float(x) > min_motion]
    if not d:
        return float(sigma0)
    return math.sqrt(sum(x * x for x in d) / len(d))


def prediction_deviation(pred, pose, max_range: float) -> float:
    """delta = |t| + 2 max_range sin(theta / 2) of pred^-1 pose (4,4 float64): how far a point at max_range is moved by the
    error of the prediction"""
    D = np.linalg.inv(np.asarray(pred, np.float64)) @ np.asarray(pose, np.float64)
    R = D[:3, :3]     # sin and cos of the angle, so that a small one is not lost in an arc cosine near 1
    theta = math.atan2(0.5 * math.sqrt((R[2, 1] - R[1, 2]) ** 2 + (R[0, 2] - R[2, 0]) ** 2 + (R[1, 0] - R[0, 1]) ** 2),
                       (float(np.trace(R)) - 1.0) / 2.0)
    return float(np.linalg.norm(D[:3, 3])) + 2.0 * float(max_range) * math.sin(theta / 2.0)


def adaptive_stage(sigma: float, voxel_size: float, max_iter: int):
    """((max_dist, max_iter), kernel_scale) of a step whose threshold is sigma: the gate 3 sigma, clipped at voxel_size (as
    fp32, the search's own bound: it looks into 27 voxels), and the Geman-McClure scale sigma / 3"""
    return (min(3.0 * float(sigma), float(np.float32(voxel_size))), int(max_iter)), float(sigma) / 3.0


class OdometryStep(NamedTuple):
    pose: np.ndarray          # (4,4) float64, sensor -> world
    fitness: float            # matches / registered points at the last evaluated pose
    rmse: float
    iterations: int
    status: int               # refine.CONVERGED / MAX_ITER / NO_MATCH / SINGULAR


def _copy(pcd):
    c = augment.PointCloud.from_buffers(pcd.xyz.clone(), pcd.idx.clone(), pcd.count.clone(), R=pcd.R, T=pcd.T, host_n=pcd._host_n)
    c.sweep_motion = pcd.sweep_motion
    return c


class LidarOdometry:
    """Scan-to-local-map odometry.  `step(pcd)` takes a frame (augment.PointCloud in the sensor frame) and returns its pose.

    min_range: points nearer than this are not put into the map.  schedule: ICP stages (max_dist <= voxel_size, max_iter).
    kernel_scale: Geman-McClure scale in metres (0: unweighted).  deskew: undo sweep motion with the constant-velocity
    prediction (augment.deskew, reference 0: the pose is the sensor's at the START of the sweep); time / azimuth_steps as
    there.  sample_map / sample_register: augment.voxel_sample edges for the points that are inserted and, thinned once
    more, for the points that are registered; None or 0 leaves the frame as it is.  first_pose: the first frame's pose
    (default identity).  initial_motion (4,4): the motion assumed between the first two frames, where constant velocity has
    nothing to extrapolate (default: none) -- from the vehicle's speed, say.  A sparse sensor over flat ground needs it with
    metric "point": the rings a scan draws on the ground travel with the sensor, so a second frame started one metre off
    settles on "no motion" (profiles/sim_odometry_eval.md).  metric "plane": point-to-plane rows on one plane per voxel
    (LocalMap.planes; plane_radius, min_points, max_ratio as in LocalMap.register) -- a ground point then has no say about
    motion inside the ground plane; one more launch a step.  adaptive = (sigma0, min_motion): instead of `schedule` and
    `kernel_scale` every step registers with ONE stage (min(3 sigma, voxel_size), max_iter of the schedule's last stage) and
    kernel_scale sigma / 3, sigma = adaptive_sigma of the deviations between predicted and registered pose so far (those above
    min_motion; sigma0 before there is one).  The gate is clipped at voxel_size because the search looks into 27 voxels.
    `gates` lists (schedule, kernel_scale) of every registered step.  `rebase(C)` moves the odometry into another frame (after a
    loop correction; loop_closure.GeometricSlam).

    One host synchronisation per step, counted in augment.host_syncs(): the read-back of the pose, the registration's
    results and the device-side error flags together.  The caller's frame keeps its bytes: the work is done on a copy."""

    def __init__(self, voxel_size: float = 1.0, subdivisions: int = 3, max_range: float = 100.0, min_range: float = 0.0,
                 schedule: Sequence[Tuple[float, int]] = ((1.0, 30),), kernel_scale: float = 0.1, deskew: bool = False,
                 time: str = "column", azimuth_steps: Optional[int] = None, sample_map: Optional[float] = None,
                 sample_register: Optional[float] = None, max_voxels: int = 1 << 17, first_pose=None, initial_motion=None,
                 tol_rot: float = 1e-7, tol_trans: float = 1e-6, metric: str = "point", plane_radius: Optional[float] = None,
                 min_points: int = 5, max_ratio: float = 0.1, adaptive: Optional[Tuple[float, float]] = None):
        if time not in ("column", "azimuth"):
            raise ValueError("time is 'column' or 'azimuth'")
        if metric not in ("point", "plane"):
            raise ValueError("metric is 'point' or 'plane'")
        if adaptive is not None and not (len(adaptive) == 2 and adaptive[0] > 0 and adaptive[1] >= 0):
            raise ValueError("adaptive: (sigma0 > 0, min_motion >= 0)")
        if deskew and time == "column" and not azimuth_steps:
            raise ValueError("deskew with time='column' needs azimuth_steps")
        self.local_map = LocalMap(voxel_size, subdivisions, max_voxels, max_range, min_range, plane_radius=plane_radius)
        self.metric, self.min_points, self.max_ratio = metric, int(min_points), float(max_ratio)
        self.adaptive = None if adaptive is None else (float(adaptive[0]), float(adaptive[1]))
        self.deviations: list = []   # the prediction's error at every registered step (adaptive gate)
        self.gates: list = []        # (schedule, kernel_scale) of every registered step
        self.schedule = [(float(d), int(n)) for d, n in schedule]
        if not self.schedule or any(d > float(np.float32(voxel_size)) or d <= 0 for d, _ in self.schedule):
            raise ValueError("schedule: stages (max_dist, max_iter) with 0 < max_dist <= voxel_size")
        self.kernel_scale, self.deskew, self.time, self.azimuth_steps = float(kernel_scale), bool(deskew), time, azimuth_steps
        self.sample_map, self.sample_register = sample_map, sample_register
        self.tol_rot, self.tol_trans = float(tol_rot), float(tol_trans)
        self.first_pose = np.eye(4) if first_pose is None else np.array(first_pose, np.float64).reshape(4, 4)
        self.initial_motion = np.eye(4) if initial_motion is None else np.array(initial_motion, np.float64).reshape(4, 4)
        self.poses: list = []
        self.steps: list = []
        self.rebases: list = []      # (index of the first pose in the new frame, C) of every rebase
        self._moved: dict = {}       # pose index -> that pose in the CURRENT frame, for the two poses a rebase moved

    def rebase(self, C):
        """from the next step on the odometry works in the frame C . old (C (4,4): a loop correction, say): the two poses the
        prediction reads become C @ P, so the predicted motion stays what it was up to the product's rounding.  `poses`
        recorded so far keep their bytes; `rebases` lists (len(poses), C).  The map is the caller's business
        (LocalMap.rebuild)."""
        C = np.array(C, np.float64).reshape(4, 4)
        n = len(self.poses)
        self._moved = {i: C @ self._pose(i) for i in range(max(n - 2, 0), n)}
        self.rebases.append((n, C))

    def _pose(self, i: int) -> np.ndarray:
        """pose i (negative: from the end) in the odometry's current frame: `poses[i]` unless a rebase has moved it since"""
        return self._moved.get(i % len(self.poses), self.poses[i])

    def predicted_motion(self, pcd=None) -> np.ndarray:
        """(4,4) float64: the motion predicted for the NEXT sweep, P_{k-2}^-1 P_{k-1} (`initial_motion` before two poses
        exist).  Takes and ignores a frame, so the bound method is a `motion` callable of augment.Deskew."""
        if len(self.poses) < 2:
            return self.initial_motion.copy()
        return np.linalg.inv(self._pose(-2)) @ self._pose(-1)

    def predicted_pose(self) -> np.ndarray:
        if not self.poses:
            return self.first_pose.copy()
        return self._pose(-1) @ self.predicted_motion()

    def gate(self):
        """((max_dist, max_iter), ...) and kernel_scale of the next registration: the schedule and scale given, or with
        `adaptive` the one stage that follows from the deviations so far"""
        if self.adaptive is None:
            return self.schedule, self.kernel_scale
        sigma = adaptive_sigma(self.deviations, *self.adaptive)
        stage, scale = adaptive_stage(sigma, self.local_map.voxel_size, self.schedule[-1][1])
        return [stage], scale

    def step(self, pcd) -> OdometryStep:
        dev = pcd.device
        first = not self.poses
        pred = self.predicted_pose()
        with torch.cuda.device(dev):
            work = _copy(pcd)
            if self.deskew and not first:
                augment.deskew(work, self.predicted_motion(), time=self.time, azimuth_steps=self.azimuth_steps, reference=0.0)
            if self.sample_map:
                augment.voxel_sample(work, self.sample_map)
            flags = [st[1:2] for st, _ in work._flags]
            messages = [msg for _, msg in work._flags]
            lm = self.local_map
            if first:
                lm.origin = pred[:3, 3].copy() if lm.origin is None else lm.origin
                pose_dev = _pose_tensor(pred, dev)
                lm.insert(work, pose_dev)
                lm.prune(pose_dev)
                results = torch.zeros(4, device=dev, dtype=torch.float64)
                results[3] = CONVERGED
            else:
                reg = work
                if self.sample_register:
                    reg = augment.voxel_sample(_copy(work), self.sample_register)
                    flags += [st[1:2] for st, _ in reg._flags]      # the copy starts without flags
                    messages += [msg for _, msg in reg._flags]
                schedule, kernel_scale = self.gate()
                self.gates.append((tuple(schedule), kernel_scale))
                if self.metric == "point":
                    res = lm.register(reg, pred, schedule, kernel_scale, self.tol_rot, self.tol_trans)
                else:
                    res = lm.register(reg, pred, schedule, kernel_scale, self.tol_rot, self.tol_trans, metric=self.metric,
                                      min_points=self.min_points, max_ratio=self.max_ratio)
                # a failed registration (NO_MATCH, SINGULAR: possibly after steps that led nowhere) keeps the prediction, and
                # its frame must not enter the map: pose and count are chosen on the device, so insert and prune still
                # queue without a host read
                ok = (res.status == CONVERGED) | (res.status == MAX_ITER)
                pose_dev = torch.where(ok, res.pose.reshape(4, 4), _pose_tensor(pred, dev))
                work.count = work.count * ok.to(torch.int32)
                lm.insert(work, pose_dev)
                lm.prune(pose_dev)
                results = torch.cat([res.fitness.double(), res.rmse.double(), res.iterations.double(), res.status.double()])
            hdr = lm.table[:4].view(torch.int32).double()
            back = torch.cat([pose_dev.reshape(16), results, hdr] + [f.double() for f in flags])
            augment._SYNCS[0] += 1
            host = back.cpu().numpy()          # the step's one host synchronisation
        for flag, msg in zip(host[21:], messages):
            if flag:
                raise ValueError(msg)
        if host[20]:
            raise ValueError(OVERFLOW.format(lm.max_voxels))
        pose = host[:16].reshape(4, 4).copy()
        # an ICP step turns the pose by an exact rotation, so whatever its rotation block has drifted from orthonormal stays,
        # and the extrapolation P (P'^-1 P) feeds it back every frame: the nearest rotation (SVD) is what is kept
        if first:
            pose = pred.copy()                 # the given pose, as given
        else:
            U, _, Vt = np.linalg.svd(pose[:3, :3])
            pose[:3, :3] = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt
        out = OdometryStep(pose, float(host[16]), float(host[17]), int(host[18]), int(host[19]))
        if not first and out.status in (CONVERGED, MAX_ITER):
            self.deviations.append(prediction_deviation(pred, pose, lm.max_range))
        self.poses.append(out.pose)
        self.steps.append(out)
        return out


def run_odometry(frames, **kw) -> np.ndarray:
    """frames: an iterable of augment.PointCloud in sensor coordinates -> (n,4,4) float64 poses.  kw: LidarOdometry's."""
    odo = LidarOdometry(**kw)
    for f in frames:
        odo.step(f)
    return np.stack(odo.poses) if odo.poses else np.zeros((0, 4, 4))
