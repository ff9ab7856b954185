"""A GPU LiDAR simulator: procedural street scenes ray-cast with a spinning-LiDAR model (kernels in csrc/lidar_sim.hip).

The reference has no counterpart; what this module computes is pinned to this project's own restatement
(tests/lidar_sim_restated.py) and to nothing else.  It gives the training stack scans that look like scans -- surfaces,
occlusion, a scan pattern -- with EXACT ground-truth poses, and writes the dataset tree `dataset.SlamDatasets`,
`loader.EpochLoader` and `loader.SceneLoader` read.

Host side (numpy, float64, deterministic):

* `Scene`: a ground plane z = z0 (optional) plus P primitives: oriented boxes (centre, half extents, yaw about world z)
  and capped vertical cylinders (base centre, radius, height), each with a class id and an albedo.
* `street_scene(seed, blocks)`: a block grid with buildings along the roads, parked cars, poles and trunks; every random
  number is one `numpy.random.Generator(PCG64(seed)).random()` call, so every numpy build makes the same scene.
* `circuit(scene, spacing, laps)`: (F,4,4) float64 sensor poses round the scene's outer loop of roads, heading along the
  tangent, roll and pitch small and NON-zero.
* `LidarModel`: beam elevations x azimuth steps; ray r = beam * azimuth_steps + column.  The unit directions are computed
  once in float64 and rounded to float32: the kernels evaluate no trigonometry.
* Sweep motion (optional).  ONE definition, used by the simulator, by `augment.deskew` and by the restatement
  (tests/lidar_sweep_restated.py): a frame has a start pose P0 and an end pose P1, sensor-to-world, float64.
  D = P0^-1 P1 = (R_D, t_D), w = Log(R_D), a rotation vector with angle below pi.  At sweep fraction s in [0, 1] the sensor is
  at P(s) = P0 D(s), D(s) = (Exp(s w), s t_D): a constant turn rate about a fixed axis, the origin on a straight line at
  constant speed.  All beams of column c fire at s_c = c / azimuth_steps.  A raw point is t * dir in the sensor's frame AT
  ITS OWN TIME; deskewing to the reference time s_ref maps a raw point p fired at s to D(s_ref)^-1 D(s) p.
  `sweep_delta`, `motion_at`, `sweep_poses` are the host side of it.  Without end poses: one pose per frame, as before.

GPU side, following augment.py's two layers:

* FUNCTIONAL: `cast_rays(scene_dev, poses, model, poses_end=None)` -> (range, prim, cos_inc), `emit_frames(...)` -> frames
  (`augment.PointCloud.from_buffers`, idx = the ray index, so ring = idx // azimuth_steps and column = idx % azimuth_steps
  stay recoverable), intensity and label.  Every random quantity (`noise`, `u`) is an argument.  Three launches for F frames,
  no host synchronisation.  More than `max_kept` primitives in range of a frame raise ValueError at the frames' next
  read-back (PointCloud.check / nbr_point / collate_frames), the way augment.voxel_sample's grid flag does.
* CLASS: `LidarSimulator(scene, model, rng)`; `rng=None` gives clean scans, a `torch.Generator(device="cuda")` draws the
  range noise and the drop mask on the device.

`prim` ids: 0..P-1 the primitive, P (`Scene.ground_id`) the ground, -1 no return.
"""
from __future__ import annotations

import math
import os
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import ops

GROUND, BUILDING, VEHICLE, POLE, TRUNK = 0, 1, 2, 3, 4
CLASS_NAMES = {GROUND: "ground", BUILDING: "building", VEHICLE: "vehicle", POLE: "pole", TRUNK: "trunk"}
BOX, CYLINDER = ops.LIDAR_BOX, ops.LIDAR_CYLINDER
SENSOR_HEIGHT = 1.8


# ------------------------------------------------------------------------------------------------------------
# scene
# ------------------------------------------------------------------------------------------------------------
class Scene:
    """z0: height of the ground plane, None for a scene without ground.  Primitives are appended with add_box /
    add_cylinder; `kind` (P,) int32, `params` (P,7) float64 = (x, y, z, e0, e1, e2, yaw) with (e0, e1, e2) the half extents of a
    box about its centre (x, y, z), or (radius, height, 0) of a cylinder standing on its base centre (x, y, z);
    `class_id` (P,) int32, `albedo` (P,) float64.  `layout`: what street_scene laid out (circuit reads it)."""

    def __init__(self, z0: Optional[float] = 0.0, ground_albedo: float = 0.25):
        self.z0 = None if z0 is None else float(z0)
        self.ground_albedo = float(ground_albedo)
        self._kind, self._params, self._class, self._albedo = [], [], [], []
        self.layout = None

    def add_box(self, centre, half, yaw=0.0, class_id=BUILDING, albedo=0.5):
        if min(half) <= 0:
            raise ValueError("half extents must be positive")
        self._kind.append(BOX)
        self._params.append([*map(float, centre), *map(float, half), float(yaw)])
        self._class.append(int(class_id)), self._albedo.append(float(albedo))
        return len(self._kind) - 1

    def add_cylinder(self, base, radius, height, class_id=POLE, albedo=0.5):
        if radius <= 0 or height <= 0:
            raise ValueError("radius and height must be positive")
        self._kind.append(CYLINDER)
        self._params.append([*map(float, base), float(radius), float(height), 0.0, 0.0])
        self._class.append(int(class_id)), self._albedo.append(float(albedo))
        return len(self._kind) - 1

    @property
    def P(self) -> int:
        return len(self._kind)

    @property
    def ground_id(self) -> int:
        return self.P

    @property
    def kind(self):
        return np.asarray(self._kind, np.int32).reshape(-1)

    @property
    def params(self):
        return np.asarray(self._params, np.float64).reshape(-1, 7)

    @property
    def class_id(self):
        return np.asarray(self._class, np.int32).reshape(-1)

    @property
    def albedo(self):
        return np.asarray(self._albedo, np.float64).reshape(-1)

    def arrays(self):
        """what the kernels read: prims (P,10) float64 (include/dpm_hip.h: dpm_lidar_cull), kind (P,) int32, ground (2,)
        float64, albedo (P+1,) float32 and class_id (P+1,) int32 with the ground last"""
        q, kind = self.params, self.kind
        prims = np.zeros((self.P, ops.LIDAR_PRIM), np.float64)
        prims[:, :6] = q[:, :6]
        box = kind == BOX
        prims[:, 6] = np.where(box, np.cos(q[:, 6]), 1.0)
        prims[:, 7] = np.where(box, np.sin(q[:, 6]), 0.0)
        # bounding sphere: about the centre of a box, about the middle of a cylinder's axis
        prims[:, 8] = np.where(box, 0.0, 0.5 * q[:, 4])
        prims[:, 9] = np.where(box, np.sqrt(q[:, 3] ** 2 + q[:, 4] ** 2 + q[:, 5] ** 2), np.sqrt(q[:, 3] ** 2 + (0.5 * q[:, 4]) ** 2))
        ground = np.array([0.0 if self.z0 is None else self.z0, 0.0 if self.z0 is None else 1.0], np.float64)
        albedo = np.concatenate([self.albedo, [self.ground_albedo]]).astype(np.float32)
        class_id = np.concatenate([self.class_id, [GROUND]]).astype(np.int32)
        return prims, kind, ground, albedo, class_id

    def to_device(self, device=None) -> "SceneDevice":
        return SceneDevice(self, device)


class SceneDevice:
    """a Scene's arrays on the GPU"""

    def __init__(self, scene: Scene, device=None):
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        prims, kind, ground, albedo, class_id = scene.arrays()
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.prims, self.kind, self.ground, self.albedo, self.class_id = up(prims), up(kind), up(ground), up(albedo), up(class_id)
        self.P, self.device = scene.P, dev


def street_scene(seed: int, blocks=(2, 2), block: float = 44.0, road: float = 12.0, cars: int = 6, poles: int = 4,
                 trunks: int = 3, z0: float = 0.0) -> Scene:
    """A grid of blocks[0] x blocks[1] city blocks of side `block` m between roads `road` m wide (road centre lines at
    multiples of block + road, the outermost roads included).  Per block: buildings along its four sides (yaw within a few
    degrees of the road), `cars` parked cars in the roads beside it, `poles` poles and `trunks` trunks on its pavement."""
    rng = np.random.Generator(np.random.PCG64(int(seed)))
    u = lambda a, b: a + (b - a) * float(rng.random())
    nx, ny = int(blocks[0]), int(blocks[1])
    if nx < 1 or ny < 1:
        raise ValueError("blocks: at least 1 x 1")
    pitch = block + road
    scene = Scene(z0=z0, ground_albedo=0.2)
    for bi in range(nx):
        for bj in range(ny):
            x0, y0 = bi * pitch + 0.5 * road, bj * pitch + 0.5 * road      # the block's corner
            pave = 2.5                                                     # pavement between kerb and facades
            # buildings: walk along each side, facade on the pavement line, depth into the block
            for side in range(4):
                s = pave
                while s < block - pave - 6.0:
                    width = min(u(7.0, 16.0), block - pave - s)
                    depth, height = u(6.0, 12.0), u(5.0, 22.0)
                    mid, inn = s + 0.5 * width, pave + 0.5 * depth
                    cx, cy = [(x0 + mid, y0 + inn), (x0 + block - inn, y0 + mid), (x0 + block - mid, y0 + block - inn),
                              (x0 + inn, y0 + block - mid)][side]
                    yaw = side * 0.5 * math.pi + u(-0.04, 0.04)
                    scene.add_box((cx, cy, z0 + 0.5 * height), (0.5 * width - 0.3, 0.5 * depth, 0.5 * height), yaw, BUILDING,
                                  u(0.3, 0.8))
                    s += width + u(0.5, 3.0)
            # parked cars: in the road, 1.3 m off the kerb, along the side they stand at
            for _ in range(int(cars)):
                side, along = int(4 * rng.random()) % 4, u(4.0, block - 4.0)
                off = -1.3
                cx, cy = [(x0 + along, y0 + off), (x0 + block - off, y0 + along), (x0 + block - along, y0 + block - off),
                          (x0 + off, y0 + block - along)][side]
                scene.add_box((cx, cy, z0 + 0.78), (u(2.0, 2.5), u(0.85, 0.95), 0.75), side * 0.5 * math.pi + u(-0.05, 0.05),
                              VEHICLE, u(0.2, 0.9))
            for n, cls, (r0, r1), (h0, h1) in ((poles, POLE, (0.08, 0.15), (6.0, 9.0)), (trunks, TRUNK, (0.2, 0.45), (3.0, 6.0))):
                for _ in range(int(n)):
                    side, along = int(4 * rng.random()) % 4, u(1.0, block - 1.0)
                    off = u(0.6, 1.6)
                    cx, cy = [(x0 + along, y0 + off), (x0 + block - off, y0 + along), (x0 + block - along, y0 + block - off),
                              (x0 + off, y0 + block - along)][side]
                    scene.add_cylinder((cx, cy, z0), u(r0, r1), u(h0, h1), cls, u(0.2, 0.6))
    scene.layout = dict(blocks=(nx, ny), block=float(block), road=float(road), pitch=float(pitch), z0=float(z0))
    return scene


def _loop_point(s, w, h, r):
    """arc-length s on a w x h rectangle with corners rounded at radius r, counter-clockwise from (r, 0): (x, y, heading)"""
    quarter = 0.5 * math.pi * r
    legs = [w - 2 * r, quarter, h - 2 * r, quarter, w - 2 * r, quarter, h - 2 * r, quarter]
    starts = [(r, 0.0, 0.0), None, (w, r, 0.5 * math.pi), None, (w - r, h, math.pi), None, (0.0, h - r, 1.5 * math.pi), None]
    centres = [None, (w - r, r), None, (w - r, h - r), None, (r, h - r), None, (r, r)]
    for k, leg in enumerate(legs):
        if s <= leg or k == 7:
            if k % 2 == 0:
                x, y, th = starts[k]
                return x + s * math.cos(th), y + s * math.sin(th), th
            th0 = (k // 2) * 0.5 * math.pi
            a = th0 - 0.5 * math.pi + s / r
            cx, cy = centres[k]
            return cx + r * math.cos(a), cy + r * math.sin(a), th0 + s / r
        s -= leg
    raise AssertionError


def circuit_length(scene: Scene, radius: float = 6.0) -> float:
    lay = scene.layout
    w, h = lay["blocks"][0] * lay["pitch"], lay["blocks"][1] * lay["pitch"]
    return 2 * (w - 2 * radius) + 2 * (h - 2 * radius) + 2 * math.pi * radius


def circuit(scene: Scene, spacing: float = 2.0, laps: int = 1, radius: float = 6.0) -> np.ndarray:
    """(F,4,4) float64 sensor-to-world poses round the outermost roads of a street_scene, counter-clockwise, F =
    laps * round(length / spacing): consecutive poses are length / round(length / spacing) apart along the path, and the
    pose after the last of a lap is the first of that lap again.  Lap k runs 0.3 k m further out, so `laps > 1` revisits
    every place without repeating a pose.  R = Rz(heading) Ry(pitch) Rx(roll) with the heading along the tangent and
    roll, pitch within 0.03 rad, nowhere both zero; the sensor rides SENSOR_HEIGHT above the ground."""
    lay = scene.layout
    if lay is None:
        raise ValueError("circuit needs a scene made by street_scene")
    w, h = lay["blocks"][0] * lay["pitch"], lay["blocks"][1] * lay["pitch"]
    L = circuit_length(scene, radius)
    per_lap = max(int(round(L / float(spacing))), 3)
    out = np.zeros((per_lap * int(laps), 4, 4), np.float64)
    for i in range(out.shape[0]):
        lap, k = divmod(i, per_lap)
        s = k * (L / per_lap)
        x, y, th = _loop_point(s, w, h, radius)
        x, y = x + 0.3 * lap * math.sin(th), y - 0.3 * lap * math.cos(th)     # to the right of the heading = outwards
        roll = 0.02 * math.sin(2 * math.pi * 3 * s / L + 0.5) + 0.004
        pitch = 0.015 * math.cos(2 * math.pi * 5 * s / L) + 0.006
        cz, sz, cy, sy, cx, sx = math.cos(th), math.sin(th), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
        Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
        Ry = np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
        Rx = np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
        out[i, :3, :3] = Rz @ Ry @ Rx
        out[i, :3, 3] = (x, y, lay["z0"] + SENSOR_HEIGHT)
        out[i, 3, 3] = 1.0
    return out


# ------------------------------------------------------------------------------------------------------------
# sweep motion (module docstring; csrc/sweep_motion.h is the same definition for the kernels)
# ------------------------------------------------------------------------------------------------------------
def _rot_log(R):
    """the rotation vector of R (3,3), angle below pi: from the antisymmetric part sin(angle) k and the trace"""
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], np.float64)
    n = float(np.sqrt(v @ v))
    if n == 0.0:
        return np.zeros(3)
    return v / n * math.atan2(n, 0.5 * (float(np.trace(R)) - 1.0))


def _rot_exp(w):
    """Rodrigues' formula with 1 - cos a = 2 sin^2(a / 2)"""
    a = float(np.sqrt(w @ w))
    if a == 0.0:
        return np.eye(3)
    k = w / a
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + math.sin(a) * K + 2.0 * math.sin(0.5 * a) ** 2 * (K @ K)


def sweep_delta(P0, P1) -> np.ndarray:
    """D = P0^-1 P1 for poses (4,4) or (F,4,4) float64: the sensor's pose at the end of the sweep in its frame at the start"""
    P0, P1 = np.asarray(P0, np.float64), np.asarray(P1, np.float64)
    if P0.shape != P1.shape or P0.shape[-2:] != (4, 4):
        raise ValueError("start and end poses: (4,4) or (F,4,4), alike")
    D = np.zeros_like(P0)
    Rt = np.swapaxes(P0[..., :3, :3], -1, -2)
    D[..., :3, :3] = Rt @ P1[..., :3, :3]
    D[..., :3, 3] = (Rt @ (P1[..., :3, 3] - P0[..., :3, 3])[..., None])[..., 0]
    D[..., 3, 3] = 1.0
    return D


def motion_at(D, s: float) -> np.ndarray:
    """D(s) = (Exp(s Log R_D), s t_D) as (4,4) float64: D(0) = I, D(1) = D"""
    D = np.asarray(D, np.float64).reshape(4, 4)
    out = np.eye(4)
    out[:3, :3] = _rot_exp(float(s) * _rot_log(D[:3, :3]))
    out[:3, 3] = float(s) * D[:3, 3]
    return out


def sweep_poses(poses):
    """(P0, P1), each (F,4,4), for a trajectory whose sensor turns once between consecutive poses: P1[f] = poses[f + 1], the
    last frame goes on by its previous delta (a single pose stands still)"""
    P0 = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    P1 = np.empty_like(P0)
    P1[:-1] = P0[1:]
    P1[-1] = P0[-1] @ sweep_delta(P0[-2], P0[-1]) if P0.shape[0] > 1 else P0[-1]
    return P0, P1


# ------------------------------------------------------------------------------------------------------------
# sensor
# ------------------------------------------------------------------------------------------------------------
class LidarModel:
    """elevations_deg: one angle per beam (ring), positive up; azimuth_steps columns per turn, column c looks along azimuth
    2 pi c / azimuth_steps from the sensor's +x towards +y.  Returns nearer than min_range or beyond max_range are lost.
    range_sigma (m) and drop_prob are what LidarSimulator draws with; the kernels take the draws as arguments."""

    def __init__(self, elevations_deg, azimuth_steps: int, min_range: float, max_range: float, range_sigma: float = 0.02,
                 drop_prob: float = 0.0):
        self.elevations_deg = np.asarray(elevations_deg, np.float64).reshape(-1)
        self.azimuth_steps = int(azimuth_steps)
        self.min_range, self.max_range = float(min_range), float(max_range)
        self.range_sigma, self.drop_prob = float(range_sigma), float(drop_prob)
        if self.elevations_deg.size < 1 or self.azimuth_steps < 1:
            raise ValueError("at least one beam and one azimuth step")
        if not 0.0 <= self.min_range < self.max_range:
            raise ValueError("0 <= min_range < max_range")
        if not 0.0 <= self.drop_prob <= 1.0 or self.range_sigma < 0:
            raise ValueError("drop_prob in [0, 1], range_sigma >= 0")
        if self.rays > ops.LIDAR_MAX_RAYS:
            raise ValueError(f"at most {ops.LIDAR_MAX_RAYS} rays")
        self._dirs = None

    @property
    def beams(self) -> int:
        return self.elevations_deg.size

    @property
    def rays(self) -> int:
        return self.beams * self.azimuth_steps

    def directions(self) -> np.ndarray:
        """(rays,3) float32 unit directions, ray = beam * azimuth_steps + column: float64 trigonometry rounded once"""
        if self._dirs is None:
            e = np.deg2rad(self.elevations_deg)[:, None]
            a = (2.0 * np.pi * np.arange(self.azimuth_steps, dtype=np.float64) / self.azimuth_steps)[None, :]
            d = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e) * np.ones_like(a)], axis=-1)
            self._dirs = np.ascontiguousarray(d.reshape(-1, 3).astype(np.float32))
        return self._dirs

    def with_(self, **kw) -> "LidarModel":
        args = dict(elevations_deg=self.elevations_deg, azimuth_steps=self.azimuth_steps, min_range=self.min_range,
                    max_range=self.max_range, range_sigma=self.range_sigma, drop_prob=self.drop_prob)
        args.update(kw)
        return LidarModel(**args)


HDL64E = LidarModel(np.linspace(2.0, -24.8, 64), 2048, 0.9, 120.0)
SMALL16 = LidarModel(np.linspace(10.0, -20.0, 16), 512, 0.9, 80.0)     # the small preset (tests, quick looks)


# ------------------------------------------------------------------------------------------------------------
# functional layer
# ------------------------------------------------------------------------------------------------------------
OVERFLOW = "more than max_kept={} primitives within max_range of a frame; raise max_kept"


def _poses(poses, dev):
    p = torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float64)) if isinstance(poses, np.ndarray) else poses
    if p.dim() != 3 or p.shape[1:] != (4, 4) or p.shape[0] < 1:
        raise ValueError("poses: (F,4,4)")
    return p.to(device=dev, dtype=torch.float64).contiguous()


def _dirs(model: LidarModel, dev):
    return torch.from_numpy(model.directions()).to(dev)


class Cast(tuple):
    """(range, prim, cos_inc), each (F,rays), with `status` (F,2) = (primitives in range, overflow flag) of the cull,
    `max_kept` and, of a cast with sweep motion, the column `table` (F,azimuth_steps,12), else None.  check() reads the flags
    back (a host synchronisation) and raises ValueError on an overflow."""

    def __new__(cls, rng, prim, cos_inc, status, max_kept, table=None):
        self = super().__new__(cls, (rng, prim, cos_inc))
        self.status, self.max_kept, self.table = status, max_kept, table
        return self

    def check(self):
        if bool(self.status[:, 1].any().item()):
            raise ValueError(OVERFLOW.format(self.max_kept))


def cast_rays(scene_dev: SceneDevice, poses, model: LidarModel, max_kept: Optional[int] = None, dirs=None,
              poses_end=None) -> Cast:
    """two launches, no host synchronisation.  poses (F,4,4) float64 sensor-to-world (numpy or tensor); max_kept: room for
    the primitives within max_range of one frame (default: all of them, which cannot overflow).  poses_end (F,4,4): the
    sensor moves from poses[f] to poses_end[f] during frame f (module docstring); range is then measured from the sensor's
    origin at the ray's own time, and max_kept counts the primitives within max_range + the travel."""
    dev = scene_dev.device
    max_kept = max(scene_dev.P, 1) if max_kept is None else int(max_kept)
    with torch.cuda.device(dev):
        poses = _poses(poses, dev)
        dirs = _dirs(model, dev) if dirs is None else dirs
        if poses_end is None:
            kept, plane, status = ops.lidar_cull(scene_dev.prims, scene_dev.kind, scene_dev.ground, poses, model.max_range, max_kept)
            rng, prim, cos_inc = ops.lidar_cast(kept, plane, status, scene_dev.P, dirs, model.min_range, model.max_range)
            return Cast(rng, prim, cos_inc, status, max_kept)
        poses_end = _poses(poses_end, dev)
        if poses_end.shape != poses.shape:
            raise ValueError("poses_end: one end pose per frame")
        kept, plane, status, table = ops.lidar_cull_sweep(scene_dev.prims, scene_dev.kind, scene_dev.ground, poses, poses_end,
                                                          model.azimuth_steps, model.max_range, max_kept)
        rng, prim, cos_inc = ops.lidar_cast_sweep(kept, plane, status, table, scene_dev.P, dirs, model.min_range, model.max_range)
    return Cast(rng, prim, cos_inc, status, max_kept, table)


def emit_frames(rng, prim, cos_inc, model: LidarModel, poses, noise=None, u=None, *, scene: SceneDevice, status=None,
                max_kept=None, dirs=None, poses_end=None):
    """one launch, no host synchronisation: -> (frames, intensity (F,rays), label (F,rays)).  Frame f is an
    augment.PointCloud over xyz (rays,3), idx (rays,) = ray indices, count (1,) with R, T = the pose (poses on the HOST:
    numpy or a CPU tensor) and host_n=None.  noise (F,rays) metres along the ray; u (F,rays) uniform draws, a ray with
    u < model.drop_prob is dropped.  `scene` carries the albedo and class tables; `status` = Cast.status arms the frames'
    deferred overflow error.  poses_end: the end poses of a cast with sweep motion; the frames keep R, T = the START pose and
    carry `sweep_motion` = D (4,4) float64 numpy (None otherwise): the rows are raw, each in the sensor's frame at its time."""
    from .augment import PointCloud
    as_host = lambda p: (p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)).astype(np.float64).reshape(-1, 4, 4)
    host = as_host(poses)
    if host.shape[0] != rng.shape[0]:
        raise ValueError("one pose per frame")
    motion = None
    if poses_end is not None:
        if as_host(poses_end).shape != host.shape:
            raise ValueError("poses_end: one end pose per frame")
        motion = sweep_delta(host, as_host(poses_end))
    with torch.cuda.device(rng.device):
        dirs = _dirs(model, rng.device) if dirs is None else dirs
        xyz, idx, count, intensity, label = ops.lidar_emit(rng, prim, cos_inc, dirs, scene.albedo, scene.class_id, noise=noise,
                                                           u=u, drop_prob=model.drop_prob if u is not None else 0.0)
    frames = []
    for f in range(host.shape[0]):
        pcd = PointCloud.from_buffers(xyz[f], idx[f], count[f:f + 1], R=host[f, :3, :3].copy(), T=host[f, :3, 3:].copy(),
                                      host_n=None)
        if status is not None:
            pcd._flags.append((status[f], OVERFLOW.format(max_kept)))
        if motion is not None:
            pcd.sweep_motion = motion[f].copy()
        frames.append(pcd)
    return frames, intensity, label


# ------------------------------------------------------------------------------------------------------------
# class layer
# ------------------------------------------------------------------------------------------------------------
class LidarSimulator:
    """scene: a Scene (uploaded here) or a SceneDevice.  rng=None: clean scans; a torch.Generator(device="cuda"): range
    noise N(0, model.range_sigma) along the ray and, with model.drop_prob > 0, a drop mask, both drawn on the device."""

    def __init__(self, scene, model: LidarModel, rng: Optional[torch.Generator] = None, device=None,
                 max_kept: Optional[int] = None):
        if rng is not None and (not isinstance(rng, torch.Generator) or rng.device.type != "cuda"):
            raise ValueError("rng is None or a torch.Generator on the GPU")
        if device is None and rng is not None:
            device = rng.device
        self.scene = scene if isinstance(scene, SceneDevice) else scene.to_device(device)
        self.model, self.rng, self.max_kept = model, rng, max_kept
        self.dirs = _dirs(model, self.scene.device)

    def frames(self, poses, return_channels: bool = False, *, poses_end=None):
        """poses (F,4,4) on the host -> F frames for transform_frames / collate_frames; with return_channels also
        intensity and label (F,rays), indexed by RAY (a frame's idx picks its rows).  poses_end (F,4,4): sweep motion
        (module docstring): raw frames under their start pose, `sweep_motion` set for augment.Deskew("frame")."""
        dev, m = self.scene.device, self.model
        with torch.cuda.device(dev):
            cast = cast_rays(self.scene, poses, m, self.max_kept, dirs=self.dirs, poses_end=poses_end)
            noise = u = None
            if self.rng is not None:
                shape = cast[0].shape
                if m.range_sigma > 0:
                    noise = torch.randn(shape, device=dev, generator=self.rng) * m.range_sigma
                if m.drop_prob > 0:
                    u = torch.rand(shape, device=dev, generator=self.rng)
            frames, intensity, label = emit_frames(*cast, m, poses, noise=noise, u=u, scene=self.scene, status=cast.status,
                                                   max_kept=cast.max_kept, dirs=self.dirs, poses_end=poses_end)
        return (frames, intensity, label) if return_channels else frames


# ------------------------------------------------------------------------------------------------------------
# dataset writer
# ------------------------------------------------------------------------------------------------------------
def _agent_sizes(agents, F):
    if agents is None:
        return [F]
    if isinstance(agents, (int, np.integer)):
        n = int(agents)
        if not 1 <= n <= F:
            raise ValueError("agents: between 1 and the number of frames")
        return [F // n + (k < F % n) for k in range(n)]
    sizes = [int(a) for a in agents]
    if sum(sizes) != F or min(sizes) < 1:
        raise ValueError("agents: frames per agent, all positive, adding up to the number of frames")
    return sizes


def write_scene(root, dataset: str, scene_name: str, sim, poses, agents=None, fmt: str = "npz",
                refined_distance: Optional[float] = None, batch: int = 8, poses_end=None, deskew: Optional[float] = None) -> List[str]:
    """Writes root/<dataset>/<scene_name>/<agent>/<n>.npz (lidar_pcd (N,4) float32 = x y z intensity, ego_rotation (3,3),
    ego_translation (3,1) float64) for every pose, n = the frame's index in the scene; -> the files in frame order.
    sim: a LidarSimulator, or the scans themselves, one (N,4) array per pose.  agents: None (one agent `0`), a number of
    agents (contiguous, near-equal shares) or the frames per agent; folder names sort in agent order.
    fmt="bin": KITTI records (N,4) float32 in <n>.bin; that format carries no pose, so the poses go to `poses.txt` (one row
    of 12 numbers per frame) and the frame distances, which SlamDatasets would read from the npz files, are written as its
    `frame_dis.npy` cache.  refined_distance: also write refined_SE3.pkl through refine.write_refined_table with the EXACT
    relative pose of every pair i < j whose positions are within that distance.
    poses_end (with a simulator): sweep motion from poses[f] to poses_end[f].  By default the RAW clouds are written under
    the start pose, as a spinning sensor delivers them; deskew=s_ref writes the clouds compensated with the true motion
    (augment.deskew by column) under the pose P(s_ref) = P0 D(s_ref).  The files have the same keys either way."""
    from . import refine
    from .dataset import pairwise_frame_dis
    if fmt not in ("npz", "bin"):
        raise ValueError("fmt is 'npz' or 'bin'")
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    F = poses.shape[0]
    starts = poses
    if poses_end is not None:
        if not hasattr(sim, "frames"):
            raise ValueError("poses_end needs a simulator: scans given as arrays are written as they are")
        poses_end = np.asarray(poses_end, np.float64).reshape(-1, 4, 4)
        if poses_end.shape != poses.shape:
            raise ValueError("poses_end: one end pose per frame")
        if deskew is not None:      # the pose the compensated cloud belongs to
            poses = np.stack([P0 @ motion_at(D, deskew) for P0, D in zip(starts, sweep_delta(starts, poses_end))])
    elif deskew is not None:
        raise ValueError("deskew needs poses_end")
    sizes = _agent_sizes(agents, F)
    width = len(str(len(sizes) - 1))
    scene_root = os.path.join(str(root), dataset, scene_name)
    folder = []
    for k, n in enumerate(sizes):
        d = os.path.join(scene_root, str(k).zfill(width))
        os.makedirs(d, exist_ok=True)
        folder += [d] * n
    simulated = hasattr(sim, "frames")
    if not simulated and len(sim) != F:
        raise ValueError("one scan per pose")
    files = []
    for a in range(0, F, batch):
        b = min(a + batch, F)
        if simulated:
            if poses_end is None:
                frames, intensity, _ = sim.frames(poses[a:b], return_channels=True)
            else:
                frames, intensity, _ = sim.frames(starts[a:b], return_channels=True, poses_end=poses_end[a:b])
            scans = []
            for f, pcd in enumerate(frames):
                if deskew is not None:
                    from .augment import deskew as _deskew
                    pcd = _deskew(pcd, pcd.sweep_motion, time="column", azimuth_steps=sim.model.azimuth_steps, reference=deskew)
                n = pcd.nbr_point
                rows = torch.cat([pcd.xyz[:n], intensity[f][pcd.idx[:n].long()].unsqueeze(1)], dim=1)
                scans.append(rows.cpu().numpy())
        else:
            scans = [np.ascontiguousarray(s, dtype=np.float32) for s in sim[a:b]]
        for k, rows in zip(range(a, b), scans):
            if rows.ndim != 2 or rows.shape[1] != 4:
                raise ValueError("a scan is (N,4): x y z intensity")
            path = os.path.join(folder[k], f"{k}.{fmt}")
            if fmt == "npz":
                np.savez(path, lidar_pcd=rows.astype(np.float32), ego_rotation=poses[k, :3, :3].copy(),
                         ego_translation=poses[k, :3, 3:].copy())
            else:
                rows.astype(np.float32).tofile(path)
            files.append(path)
    if fmt == "bin":
        np.savetxt(os.path.join(scene_root, "poses.txt"), poses[:, :3, :].reshape(F, 12), fmt="%.17g")
        np.save(os.path.join(scene_root, "frame_dis.npy"), pairwise_frame_dis(poses[:, :3, 3].astype(np.float32)))
    if refined_distance is not None:
        pairs = refine.candidate_pairs(poses[:, :3, 3], float(refined_distance))
        rel = refine.relative_poses(poses[:, :3, :3], poses[:, :3, 3], pairs)
        refine.write_refined_table(os.path.join(scene_root, "refined_SE3.pkl"),
                                   {(int(i), int(j)): M for (i, j), M in zip(pairs, rel)})
    return files


def tree_config(root, scenes: dict, fmt: str = "npz", distance: float = 10.0, loop_distance: float = 6.0, K: int = 6,
                K_max: int = 12) -> dict:
    """the `dataset` and `train` sections of a config for the tree write_scene made: scenes = {dataset: [scene names]}"""
    return {
        "dataset": [{"name": name, "root": os.path.join(str(root), name), "scenes": list(names), "reader": {"type": fmt}}
                    for name, names in scenes.items()],
        "train": {"registration": {"K": K, "K_max": K_max, "fill": True, "distance": float(distance), "map_size_max": 4},
                  "loop_detection": {"distance": float(loop_distance)}},
    }
