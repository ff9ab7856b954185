"""A geometric LiDAR odometry on the GPU: a rolling hashed voxel map and robust point-to-point ICP of every scan against it
(csrc/local_map.hip), in the KISS-ICP family.  The reference has no counterpart: its poses come from the learned pipeline
only.  Here it gives the evaluation tools (evaluate.py) a system to judge, the learned pipeline a baseline, the deskew
(augment.deskew) its motion source without ground truth, and refine.build_refined_table global poses to start from.

`LocalMap` is the map: insert, prune, register, read-back.  Its content is a function of the inserted points alone
(DESIGN §7j): a sub-cell of a voxel keeps the point of the oldest frame, and within a frame of the smallest original row.
`LidarOdometry.step` is one frame: constant-velocity prediction on the host, optional deskew with that prediction, thinning
with augment.voxel_sample, then register -> insert -> prune queued on the device pose, and ONE read-back.
"""
from __future__ import annotations

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


class LocalMap:
    """A rolling voxel map of `max_voxels` slots (a power of two) with voxels of `voxel_size` metres cut into
    subdivisions^3 sub-cells of one point each.  Coordinates are kept in fp32 relative to `origin` (three float64; default:
    the translation of the first inserted pose), so work far from the world's zero keeps fp32 accuracy.  Points are
    offered when min_range <= |p| <= max_range in the sensor frame.  A map that ran out of slots is undefined: `overflow`
    is then non-zero and every read-back (`points`, `n_points`, `check`) raises ValueError."""

    def __init__(self, voxel_size: float = 1.0, subdivisions: int = 3, max_voxels: int = 1 << 17, max_range: float = 100.0,
                 min_range: float = 0.0, origin=None, device=None):
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

    # -- plumbing
    def _ready(self, dev, pose=None):
        if self.table is None:
            self.device = dev if self.device is None else torch.device(self.device)
            self.table = ops.local_map_new(self.max_voxels, self.subdivisions, self.device)
        if self.origin is None:
            if pose is None:
                self.origin = np.zeros(3)
            else:
                if isinstance(pose, torch.Tensor) and pose.is_cuda:
                    augment._SYNCS[0] += 1
                    pose = pose.detach().cpu().numpy()
                self.origin = np.asarray(pose, np.float64)[:3, 3].copy()

    def _args(self):
        return self.table, self.max_voxels, self.subdivisions, self.half, self.voxel_size, self.origin

    # -- the three device operations: no host synchronisation
    def insert(self, pcd, pose):
        """the frame's valid rows under `pose` (4,4; numpy, or a tensor -- on the GPU it is read there, behind whatever wrote
        it); the rule sees the rows' `idx`.  Two launches."""
        self._ready(pcd.device, pose)
        if pcd.cap == 0:
            return self
        ops.local_map_insert(*self._args(), pcd.xyz, pcd.idx, pcd.count, _pose_tensor(pose, self.device), self.stamp,
                             self.min_range, self.max_range)
        self.stamp += 1
        return self

    def prune(self, pose, radius: Optional[float] = None):
        """keep the voxels whose centre lies within `radius` (default max_range) of the pose's translation"""
        self._ready(self.device if self.device is not None else augment._device(), pose)
        ops.local_map_prune(*self._args(), _pose_tensor(pose, self.device), self.max_range if radius is None else float(radius))
        self.half = 1 - self.half
        return self

    def register(self, pcd, init, schedule: Sequence[Tuple[float, int]] = ((1.0, 30),), kernel_scale: float = 0.0,
                 tol_rot: float = 1e-7, tol_trans: float = 1e-6, debug: bool = False):
        """ICP of the frame against the map from `init` (4,4) over schedule = [(max_dist <= voxel_size, max_iter), ...] ->
        refine.IcpResult with one problem (pose (1,4,4) float64, ...), all on the device[, (key, sub, system) with debug]"""
        if any(float(d) > float(np.float32(self.voxel_size)) for d, _ in schedule):
            raise ValueError("register: every max_dist of the schedule must be <= voxel_size (the search looks into 27 voxels)")
        self._ready(pcd.device, init)
        out = ops.local_map_register(*self._args(), pcd.xyz, pcd.count, _pose_tensor(init, self.device), schedule, kernel_scale,
                                     tol_rot, tol_trans, debug=debug)
        res = IcpResult(out[0].reshape(1, 4, 4), *out[1:5])
        return (res, out[5:]) if debug else res

    # -- read-back: host synchronisations
    @property
    def overflow(self) -> int:
        """points that found no free slot so far (0: the map is defined)"""
        if self.table is None:
            return 0
        augment._SYNCS[0] += 1
        return int(self.table[:4].view(torch.int32).item())

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
    nothing to extrapolate (default: none) -- from the vehicle's speed, say.  A sparse sensor over flat ground needs it: the
    rings a scan draws on the ground travel with the sensor, so a second frame started one metre off settles on "no motion"
    (profiles/sim_odometry_eval.md).

    One host synchronisation per step, counted in augment.host_syncs(): the read-back of the pose, the registration's
    results and the device-side error flags together.  The caller's frame keeps its bytes: the work is done on a copy."""

    def __init__(self, voxel_size: float = 1.0, subdivisions: int = 3, max_range: float = 100.0, min_range: float = 0.0,
                 schedule: Sequence[Tuple[float, int]] = ((1.0, 30),), kernel_scale: float = 0.1, deskew: bool = False,
                 time: str = "column", azimuth_steps: Optional[int] = None, sample_map: Optional[float] = None,
                 sample_register: Optional[float] = None, max_voxels: int = 1 << 17, first_pose=None, initial_motion=None,
                 tol_rot: float = 1e-7, tol_trans: float = 1e-6):
        if time not in ("column", "azimuth"):
            raise ValueError("time is 'column' or 'azimuth'")
        if deskew and time == "column" and not azimuth_steps:
            raise ValueError("deskew with time='column' needs azimuth_steps")
        self.local_map = LocalMap(voxel_size, subdivisions, max_voxels, max_range, min_range)
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

    def predicted_motion(self, pcd=None) -> np.ndarray:
        """(4,4) float64: the motion predicted for the NEXT sweep, P_{k-2}^-1 P_{k-1} (`initial_motion` before two poses
        exist).  Takes and ignores a frame, so the bound method is a `motion` callable of augment.Deskew."""
        if len(self.poses) < 2:
            return self.initial_motion.copy()
        return np.linalg.inv(self.poses[-2]) @ self.poses[-1]

    def predicted_pose(self) -> np.ndarray:
        if not self.poses:
            return self.first_pose.copy()
        return self.poses[-1] @ self.predicted_motion()

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
                res = lm.register(reg, pred, self.schedule, self.kernel_scale, self.tol_rot, self.tol_trans)
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
        self.poses.append(out.pose)
        self.steps.append(out)
        return out


def run_odometry(frames, **kw) -> np.ndarray:
    """frames: an iterable of augment.PointCloud in sensor coordinates -> (n,4,4) float64 poses.  kw: LidarOdometry's."""
    odo = LidarOdometry(**kw)
    for f in frames:
        odo.step(f)
    return np.stack(odo.poses) if odo.poses else np.zeros((0, 4, 4))
