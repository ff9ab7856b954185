"""The training transforms on the GPU (reference dataloader/transforms.py; kernels in csrc/augment.hip).

A frame -- `PointCloud` -- is a fixed-capacity buffer plus a count that lives in device memory: `xyz (cap,3)` fp32,
`idx (cap,)` int32 (the original index of every row) and `count (1,)` int32, with the pose `R`, `T` and `calib` as
float32 host tensors.  No transform needs the host to know a frame's current length, so a whole chain over a whole batch
is queued without a host synchronisation; `collate_frames` reads every length and every deferred error flag back at once.

Two layers:

* the FUNCTIONAL layer, one function per transform, every random quantity an explicit argument (`u`, `jitter`, `perm`,
  `wedges`, `R_aug`, `T_aug`): pure functions of their arguments, pinned to the reference by tests/test_gpu_augment.py;
* the CLASS layer under the reference's names and constructor signatures (`Compose`, `RandomChoice`, the 17 names of
  `pointcloud_transforms`, `get_transforms`, `PointCloudTransforms`), which asks a `DrawSource` for its random numbers.

`DrawSource` is the only place that calls `random.*` or a torch generator.  Select one with `with draws(rng) as src:`
or `Compose.__call__(pcd, rng=..., return_draws=True)`:

* `rng="reference"` (the default) makes exactly the reference's calls, in the reference's order, on Python's `random`
  and torch's default CPU generator; seeded alike it replays a reference run.  Draws whose size is the current point
  count (drop, jitter, shuffle, sample) need that count on the host: this mode synchronises ONCE PER SUCH TRANSFORM.
* `rng=torch.Generator(device="cuda")` (the training mode) makes per-point draws at capacity on the device; shuffle and
  sample become a stable key sort with the keys past the count set to +inf; the scalar draws (gates, ratios, wedges,
  R_aug, T_aug) come from a host stream derived from the generator's seed and offset.  The chain issues no host
  synchronisation until the batch is packed.  (FarthestPointSample is allowed to synchronise; as written it does not.)

What is defined HERE rather than by the reference: GroundFilter keeps points in ascending input position and represents a
sparse cell by its point of lowest input position (the reference's order comes from an unstable np.argsort and depends on
the numpy build; the kept SETS are equal).  VoxelSample(num=...) raises NotImplementedError: np.argpartition's choice among
equal counts is undefined.  VerticalCorrect turns a point on the z axis into NaN, as the reference does.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import random as _pyrandom
import threading
from typing import List, Sequence

import numpy as np
import torch

from . import _lib, ops

MAX_CELLS = 1 << 25      # voxel grid of the class layer's VoxelSample (12 bytes a cell for 'center')
MAX_WEDGES = 16
_SYNCS = [0]             # host synchronisations issued by this module (scripts/augment_bench.py reports them)


def host_syncs() -> int:
    return _SYNCS[0]


def _device():
    return torch.device("cuda", torch.cuda.current_device())


# ------------------------------------------------------------------------------------------------------------
# the frame
# ------------------------------------------------------------------------------------------------------------
class PointCloud:
    """xyz (N,3|4) numpy / tensor -> a frame on the GPU.  `rotation` (3,3) / `translation` (3,1) as in the reference;
    `norm`, `label`, `image`, `uvd` are not carried (NotImplementedError).  `capacity` >= N reserves room (rows past
    N are never read)."""

    def __init__(self, xyz, rotation=None, translation=None, norm=None, label=None, image=None, uvd=None, capacity=None):
        for name, v in (("norm", norm), ("label", label), ("image", image), ("uvd", uvd)):
            if v is not None:
                raise NotImplementedError(f"PointCloud({name}=...) is not carried by the GPU transforms")

        def host(a):
            a = torch.from_numpy(a) if isinstance(a, np.ndarray) else a
            return a.detach().to("cpu", torch.float32)

        xyz = torch.from_numpy(xyz) if isinstance(xyz, np.ndarray) else xyz
        if xyz.dim() != 2 or xyz.shape[1] < 3:
            raise ValueError("xyz must be (N,3) or (N,>=3)")
        dev = xyz.device if xyz.is_cuda else _device()
        n = xyz.shape[0]
        cap = max(int(capacity) if capacity is not None else n, n)
        self.xyz = torch.zeros(cap, 3, device=dev, dtype=torch.float32)   # always a buffer of its own: the maps act in place
        self.xyz[:n] = xyz[:, :3].to(device=dev, dtype=torch.float32)
        self.idx = torch.arange(cap, device=dev, dtype=torch.int32)
        self.count = torch.full((1,), n, device=dev, dtype=torch.int32)
        self._host_n = n
        self.R = host(rotation) if rotation is not None else torch.eye(3, dtype=torch.float32)
        self.T = host(translation) if translation is not None else torch.zeros(3, 1, dtype=torch.float32)
        self.calib = torch.eye(4, dtype=torch.float32)
        self._flags = []      # (status tensor [n, flag], message): errors found on the device, raised at the next read-back
        self._stream = None
        self.has_norm = self.has_label = self.has_image = self.has_uvd = False

    norm = label = image = uvd = None
    sweep_motion = None       # D (4,4) float64 numpy of a raw frame taken by a moving sensor (lidar_sim.py); `deskew` clears it

    @classmethod
    def from_buffers(cls, xyz, idx, count, R=None, T=None, host_n=None):
        """a frame over buffers that exist already (views of ops.ingest_frames' arena): xyz (cap,3) fp32, idx (cap,) int32,
        count (1,) int32 on the GPU, nothing copied.  `host_n` = the length when the host knows it (nothing can have been
        dropped), else None: the first reader of `nbr_point` synchronises.  R / T as in the constructor."""
        ops._chk(xyz, torch.float32, "xyz"), ops._chk(idx, torch.int32, "idx"), ops._chk(count, torch.int32, "count")
        if xyz.dim() != 2 or xyz.shape[1] != 3 or idx.shape != xyz.shape[:1] or count.numel() != 1:
            raise ValueError("from_buffers takes xyz (cap,3), idx (cap,), count (1,)")
        host = lambda a: (torch.from_numpy(a) if isinstance(a, np.ndarray) else a).detach().to("cpu", torch.float32)
        self = cls.__new__(cls)
        self.xyz, self.idx, self.count = xyz, idx, count.reshape(1)
        self._host_n = None if host_n is None else int(host_n)
        self.R = host(R) if R is not None else torch.eye(3, dtype=torch.float32)
        self.T = host(T) if T is not None else torch.zeros(3, 1, dtype=torch.float32)
        self.calib = torch.eye(4, dtype=torch.float32)
        self._flags = []
        self._stream = None
        self.has_norm = self.has_label = self.has_image = self.has_uvd = False
        return self

    @property
    def device(self):
        return self.xyz.device

    @property
    def cap(self) -> int:
        return self.xyz.shape[0]

    @property
    def nbr_point(self) -> int:
        """the current length: a host synchronisation unless it is already known"""
        if self._host_n is None:
            _SYNCS[0] += 1
            self._host_n = int(self.count.item())
            self.check(sync=False)
        return self._host_n

    def check(self, sync=True):
        """raise what the device flagged (a voxel grid past max_cells)"""
        if not self._flags:
            return
        if sync:
            _SYNCS[0] += 1
        flags, self._flags = self._flags, []
        for st, msg in flags:
            if int(st[1].item()):
                raise ValueError(msg)

    def points(self) -> torch.Tensor:
        return self.xyz[:self.nbr_point]

    def indices(self) -> torch.Tensor:
        return self.idx[:self.nbr_point]

    def _set(self, xyz, idx, count):
        self.xyz, self.idx, self.count, self._host_n = xyz, idx, count, None

    def to_tensor(self, use_norm=False, use_uvd=False, use_image=False, use_calib=False, padding_to=-1):
        return to_tensor(self, padding_to=padding_to, use_calib=use_calib, use_norm=use_norm, use_uvd=use_uvd, use_image=use_image)

    def to_gpu(self):
        pass

    def to_cpu(self):
        pass


def _outputs(pcd):
    dev = pcd.device
    return (torch.empty(pcd.cap, 3, device=dev, dtype=torch.float32), torch.empty(pcd.cap, device=dev, dtype=torch.int32),
            torch.zeros(1, device=dev, dtype=torch.int32))


def _workspace(pcd, cells):
    return torch.empty(_lib.load().dpm_augment_workspace_bytes(pcd.cap, int(cells)), device=pcd.device, dtype=torch.uint8)


# ------------------------------------------------------------------------------------------------------------
# functional layer
# ------------------------------------------------------------------------------------------------------------
def ground_filter(pcd, img_len, img_width, grid_width, ground_height, preserve_sparse_ground=True):
    """GroundFilter (transforms.py:174-227).  Kept points come in ascending input position; a sparse cell is represented
    by its point of lowest input position (defined here: the reference's order is not reproducible)."""
    if ground_height <= 0 or pcd.cap == 0:
        return pcd
    with torch.cuda.device(pcd.device):
        xo, io, no = _outputs(pcd)
        ws = _workspace(pcd, int(img_len) * int(img_width))
        _lib.check(_lib.load().dpm_ground_filter(ops._ptr(pcd.xyz), ops._ptr(pcd.idx), ops._ptr(pcd.count), pcd.cap, int(img_len),
                                                 int(img_width), float(grid_width), float(ground_height),
                                                 int(bool(preserve_sparse_ground)), ops._ptr(xo), ops._ptr(io), ops._ptr(no),
                                                 ops._ptr(ws), ops._stream(pcd.xyz)), "dpm_ground_filter")
    pcd._set(xo, io, no)
    return pcd


def voxel_sample(pcd, voxel_size, retention="center", num=None, max_cells=MAX_CELLS):
    """VoxelSample (transforms.py:322-356).  A grid past `max_cells` empties the frame and raises ValueError at the next
    read-back (PointCloud.check / nbr_point / collate_frames)."""
    if retention not in ("first", "center"):
        raise ValueError(f"'{retention}' is not a supported retention method, please use 'first' or 'center'")
    if num is not None:
        raise NotImplementedError("VoxelSample(num=...): np.argpartition's choice among equal voxel counts is undefined")
    if pcd.cap == 0:
        return pcd
    with torch.cuda.device(pcd.device):
        xo, io, _ = _outputs(pcd)
        status = torch.zeros(2, device=pcd.device, dtype=torch.int32)
        ws = _workspace(pcd, max_cells)
        _lib.check(_lib.load().dpm_voxel_select(ops._ptr(pcd.xyz), ops._ptr(pcd.idx), ops._ptr(pcd.count), pcd.cap,
                                                float(voxel_size), int(retention == "center"), int(max_cells), ops._ptr(xo),
                                                ops._ptr(io), ops._ptr(status), ops._ptr(ws), ops._stream(pcd.xyz)),
                   "dpm_voxel_select")
    pcd._flags.append((status, f"voxel grid exceeds max_cells={max_cells}; crop the scan or raise max_cells"))
    pcd._set(xo, io, status[:1])
    return pcd


def _wedge_block(wedges):
    if wedges is None:
        return None, 0
    w = np.ascontiguousarray(np.asarray(wedges, dtype=np.float32).reshape(-1, 4))
    if w.shape[0] > MAX_WEDGES:
        raise ValueError(f"at most {MAX_WEDGES} occlusion wedges, got {w.shape[0]}")
    return w, w.shape[0]


def mask_select(pcd, min_dis=None, max_dis=None, u=None, ratio=0.0, wedges=None):
    """the shared keep-flag compaction: distance crop AND u >= ratio AND outside every wedge (start, end, wraps, dis)"""
    if pcd.cap == 0:
        return pcd
    use_dist = min_dis is not None
    if u is not None:
        ops._chk(u, torch.float32, "u")
        if u.numel() < pcd.cap:
            raise ValueError(f"u needs one entry per row of capacity ({pcd.cap}), got {u.numel()}")
    w, nw = _wedge_block(wedges)
    with torch.cuda.device(pcd.device):
        xo, io, no = _outputs(pcd)
        ws = _workspace(pcd, 0)
        _lib.check(_lib.load().dpm_mask_select(ops._ptr(pcd.xyz), ops._ptr(pcd.idx), ops._ptr(pcd.count), pcd.cap, int(use_dist),
                                               float(min_dis) if use_dist else 0.0, float(max_dis) if use_dist else 0.0,
                                               ops._ptr(u), float(ratio), w.ctypes.data if nw else None, nw, ops._ptr(xo),
                                               ops._ptr(io), ops._ptr(no), ops._ptr(ws), ops._stream(pcd.xyz)), "dpm_mask_select")
    pcd._set(xo, io, no)
    return pcd


def distance_sample(pcd, min_dis, max_dis):
    """DistanceSample (transforms.py:387-397)"""
    return mask_select(pcd, min_dis=min_dis, max_dis=max_dis)


def random_drop(pcd, ratio, u):
    """RandomDrop (transforms.py:429-434): keep u[i] >= ratio (float32); u (cap,) on the GPU"""
    return mask_select(pcd, u=u, ratio=ratio)


def random_shield(pcd, wedges):
    """RandomShield / RandomOcclusion (transforms.py:447-474): wedges (k,4) = (start, end, wraps, dis_threshold) in degrees /
    metres, `end` already reduced by 360 where the wedge wraps"""
    return mask_select(pcd, wedges=wedges)


def _affine(pcd, mode, params=None, jitter=None):
    if pcd.cap == 0:
        return pcd
    p = (ctypes.c_double * 12)(*([float(v) for v in params] + [0.0] * (12 - len(params)))) if params is not None else None
    with torch.cuda.device(pcd.device):
        _lib.check(_lib.load().dpm_points_affine(ops._ptr(pcd.xyz), ops._ptr(pcd.count), pcd.cap, mode,
                                                 ctypes.cast(p, ctypes.c_void_p) if p is not None else None, ops._ptr(jitter),
                                                 ops._stream(pcd.xyz)), "dpm_points_affine")
    return pcd


def random_rt(pcd, R_aug, T_aug):
    """RandomRT (transforms.py:529-546) with the drawn R_aug (3,3), T_aug (3,1): the points on the GPU, the pose algebra
    R_new = R R_aug^T, T_new = T - R_new T_aug, calib <- [R_aug|T_aug] calib in float32 on the host"""
    R_aug = torch.as_tensor(R_aug, dtype=torch.float32).cpu().reshape(3, 3)
    T_aug = torch.as_tensor(T_aug, dtype=torch.float32).cpu().reshape(3, 1)
    _affine(pcd, 0, R_aug.flatten().tolist() + T_aug.flatten().tolist())
    R_new = pcd.R @ R_aug.T
    T_new = pcd.T - R_new @ T_aug
    se3 = torch.eye(4, dtype=torch.float32)
    se3[:3, :3], se3[:3, 3:] = R_aug, T_aug
    pcd.calib = se3 @ pcd.calib
    pcd.R, pcd.T = R_new, T_new
    return pcd


def random_pos_jitter(pcd, jitter):
    """RandomPosJitter (transforms.py:561-563): xyz += jitter; jitter (cap,3) on the GPU, already clamped"""
    ops._chk(jitter, torch.float32, "jitter")
    if jitter.numel() < 3 * pcd.cap:
        raise ValueError(f"jitter needs one row per row of capacity ({pcd.cap})")
    return _affine(pcd, 1, jitter=jitter)


def coordinates_normalization(pcd, ratio):
    """CoordinatesNormalization (transforms.py:400-407)"""
    return _affine(pcd, 2, [ratio])


def vertical_correct(pcd, angle):
    """VerticalCorrect (transforms.py:300-319); a point on the z axis becomes NaN, as in the reference"""
    if angle == 0:
        return pcd
    a = math.radians(angle)
    return _affine(pcd, 3, [math.sin(a), math.cos(a)])


_TIME_MODES = {"column": ops.DESKEW_COLUMN, "azimuth": ops.DESKEW_AZIMUTH, "times": ops.DESKEW_TIMES}


def deskew(pcd, motion, time="column", azimuth_steps=None, times=None, reference=0.0):
    """Remove the distortion of a sweep taken by a moving sensor (lidar_sim.py's motion model; no counterpart in the
    reference, which assumes compensated scans).  motion (4,4) = D, the sensor's pose at the end of the sweep in its frame at
    the start.  A row p measured at sweep fraction s becomes D(reference)^-1 D(s) p, the point in the sensor's frame at the
    reference time, with s from
      time="column":  (idx % azimuth_steps) / azimuth_steps -- right anywhere in a chain: idx survives sampling and shuffles;
      time="azimuth": the row's own azimuth, rounded to a column when azimuth_steps is given -- RAW frames only;
      time="times":   times[idx], fp32 fractions on the GPU indexed by the original row.
    In place, one launch, no host synchronisation.  The frame's pose moves to P(reference) = P D(reference) (float32, like
    every pose a frame carries) and its `sweep_motion` is cleared."""
    from .lidar_sim import motion_at
    if time not in _TIME_MODES:
        raise ValueError("time is 'column', 'azimuth' or 'times'")
    if time == "column" and (azimuth_steps is None or int(azimuth_steps) < 1):
        raise ValueError("time='column' needs azimuth_steps >= 1")
    if time == "times" and times is None:
        raise ValueError("time='times' needs times")
    if not 0.0 <= float(reference) <= 1.0:
        raise ValueError("reference in [0, 1]")
    D = np.asarray(motion, dtype=np.float64)
    if D.shape != (4, 4):
        raise ValueError("motion: (4,4)")
    if pcd.cap:
        ops.points_deskew(pcd.xyz, pcd.idx, pcd.count, D, _TIME_MODES[time], int(azimuth_steps or 0),
                          times if time == "times" else None, float(reference))
    if reference != 0.0:
        ref = torch.from_numpy(motion_at(D, reference)).to(torch.float32)
        pcd.R, pcd.T = pcd.R @ ref[:3, :3], pcd.T + pcd.R @ ref[:3, 3:]
    pcd.sweep_motion = None
    return pcd


def constant_velocity_motion(P_prev, P_cur):
    """the motion a caller WITHOUT ground truth predicts for the sweep that starts at P_cur: the previous relative pose
    P_prev^-1 P_cur (4,4) float64, i.e. the sensor goes on as it did between the last two sweeps"""
    from .lidar_sim import sweep_delta
    return sweep_delta(np.asarray(P_prev, np.float64).reshape(4, 4), np.asarray(P_cur, np.float64).reshape(4, 4))


def gather_points(pcd, sel, limit=-1):
    """rows sel[0], sel[1], ... of the frame; limit >= 0: a frame of at most `limit` points stays untouched, a longer one
    keeps `limit` rows (RandomSample, FarthestPointSample); limit < 0: every row (RandomShuffle)"""
    if pcd.cap == 0:
        return pcd
    sel = sel.to(device=pcd.device, dtype=torch.int32).contiguous()
    with torch.cuda.device(pcd.device):
        xo, io, no = _outputs(pcd)
        _lib.check(_lib.load().dpm_gather_points(ops._ptr(pcd.xyz), ops._ptr(pcd.idx), ops._ptr(pcd.count), pcd.cap, ops._ptr(sel),
                                                 sel.numel(), int(limit), ops._ptr(xo), ops._ptr(io), ops._ptr(no),
                                                 ops._stream(pcd.xyz)), "dpm_gather_points")
    pcd._set(xo, io, no)
    return pcd


def random_shuffle(pcd, perm):
    """RandomShuffle (transforms.py:418-419)"""
    return gather_points(pcd, perm, -1)


def random_sample(pcd, num, perm):
    """RandomSample (transforms.py:381-383)"""
    return gather_points(pcd, perm, int(num))


def farthest_point_sample(pcd, num):
    """FarthestPointSample (transforms.py:367-372) through the encoder's FPS kernels, first pick = point 0 (pytorch3d's
    default).  The reference needs pytorch3d here, so parity with it is unpinned."""
    num = int(num)
    if pcd.cap <= num:
        return pcd
    with torch.cuda.device(pcd.device):
        live = torch.arange(pcd.cap, device=pcd.device).unsqueeze(1) < pcd.count     # rows past the count hold anything: zero them
        sel = ops.fps(torch.where(live, pcd.xyz, torch.zeros_like(pcd.xyz)).unsqueeze(0), pcd.count, num)[0][0]
    return gather_points(pcd, sel, num)


def _filter_workspace(pcd, K):
    return torch.empty(_lib.load().dpm_filter_dc_workspace_bytes(pcd.cap, int(K)), device=pcd.device, dtype=torch.uint8)


def outlier_filter(pcd, nb_neighbors, std_ratio):
    """OutlierFilter (transforms.py:230-246) with the length read on the device: no host synchronisation.  A frame of
    at most nb_neighbors points passes through (decided on the device)."""
    from .preprocess import KNN_CELL
    if pcd.cap == 0:
        return pcd
    with torch.cuda.device(pcd.device):
        xo, io, no = _outputs(pcd)
        ws = _filter_workspace(pcd, nb_neighbors)
        _lib.check(_lib.load().dpm_outlier_filter_dc(ops._ptr(pcd.xyz), ops._ptr(pcd.idx), ops._ptr(pcd.count), pcd.cap,
                                                     int(nb_neighbors), float(std_ratio), KNN_CELL, 1.0, ops._ptr(xo),
                                                     ops._ptr(io), ops._ptr(no), ops._ptr(ws), ops._stream(pcd.xyz)),
                   "dpm_outlier_filter_dc")
    pcd._set(xo, io, no)
    return pcd


def lowpass_filter(pcd, normals_radius, normals_num, filter_std, flux=2, max_remain=-1):
    """LowPassFilter (transforms.py:256-289) with the length read on the device: no host synchronisation.  A frame of
    at most normals_num points passes through (decided on the device)."""
    from .preprocess import KNN_CELL
    if max_remain > 0:
        raise NotImplementedError("max_remain > 0 is not used by any shipped config and is not implemented")
    if pcd.cap == 0:
        return pcd
    with torch.cuda.device(pcd.device):
        xo, io, no = _outputs(pcd)
        ws = _filter_workspace(pcd, normals_num)
        _lib.check(_lib.load().dpm_lowpass_filter_dc(ops._ptr(pcd.xyz), ops._ptr(pcd.idx), ops._ptr(pcd.count), pcd.cap,
                                                     float(normals_radius), int(normals_num), float(filter_std), int(flux),
                                                     KNN_CELL, 1.0, ops._ptr(xo), ops._ptr(io), ops._ptr(no), ops._ptr(ws),
                                                     ops._stream(pcd.xyz)), "dpm_lowpass_filter_dc")
    pcd._set(xo, io, no)
    return pcd


def _pack(frames, P, dev):
    S = len(frames)
    points = torch.empty(S, 3, P, device=dev, dtype=torch.float32)
    padding = torch.empty(S, P, device=dev, dtype=torch.uint8)
    status = torch.zeros(S, 2, device=dev, dtype=torch.int32)
    xs = (ctypes.c_void_p * S)(*[f.xyz.data_ptr() for f in frames])
    cs = (ctypes.c_void_p * S)(*[f.count.data_ptr() for f in frames])
    caps = (ctypes.c_int * S)(*[f.cap for f in frames])
    _lib.check(_lib.load().dpm_pack_frames(ctypes.cast(xs, ctypes.c_void_p), ctypes.cast(cs, ctypes.c_void_p),
                                           ctypes.cast(caps, ctypes.c_void_p), S, P, ops._ptr(points), ops._ptr(padding),
                                           ops._ptr(status), torch.cuda.current_stream(dev).cuda_stream), "dpm_pack_frames")
    return points, padding.view(torch.bool), status


def collate_frames(frames: Sequence[PointCloud], padding_to: int = -1):
    """ToTensor(use_calib=True, padding_to) on every frame + map_collate_fn (body.py:155-161): (pcd (S,3,P), R (S,3,3),
    T (S,3,1), padding (S,P) bool, calib (S,4,4)), all on the GPU, P = padding_to or the longest frame.  ONE host
    synchronisation per batch: the lengths and every deferred error flag come back together.  A frame longer than
    `padding_to` raises the reference's RuntimeError (transforms.py:79-81)."""
    frames = list(frames)
    if not frames:
        raise ValueError("no frames")
    dev = frames[0].device
    with torch.cuda.device(dev):
        cur = torch.cuda.current_stream(dev)
        for f in frames:
            if f._stream is not None and f._stream != cur:
                cur.wait_stream(f._stream)
                for t in (f.xyz, f.count):
                    t.record_stream(cur)
                f._stream = None
        flags = [(st, msg) for f in frames for st, msg in f._flags]
        live = [f for f in frames if f.cap > 0]
        if padding_to > 0:
            P = int(padding_to)
            if live:
                points, padding, status = _pack(live, P, dev)
        if padding_to <= 0 or flags or len(live) != len(frames):
            rows = [torch.cat([f.count, f.count.new_zeros(1)]) for f in frames] + [st for st, _ in flags]
            _SYNCS[0] += 1
            host = torch.cat(rows).cpu().tolist()          # the one host sync of the batch
            lengths = host[0:2 * len(frames):2]
            for k, (_, msg) in enumerate(flags):
                if host[2 * len(frames) + 2 * k + 1]:
                    raise ValueError(msg)
            if padding_to <= 0:
                P = max(max(lengths), 1)
                if live:
                    points, padding, status = _pack(live, P, dev)
            over = [n > P for n in lengths]
        else:
            _SYNCS[0] += 1
            host = status.cpu().tolist()                    # the one host sync of the batch
            lengths, over = [n for n, _ in host], [bool(o) for _, o in host]
        for f in frames:
            f._flags = []
        for n, o in zip(lengths, over):
            if o:
                raise RuntimeError(f"The number of Point Cloud ({n}) is greater than `padding_to` ({P})")
        for f, n in zip(frames, lengths):
            f._host_n = n
        if len(live) != len(frames):   # frames of capacity 0 are rows of padding
            full_p = torch.zeros(len(frames), 3, P, device=dev, dtype=torch.float32)
            full_m = torch.ones(len(frames), P, device=dev, dtype=torch.bool)
            rows = [k for k, f in enumerate(frames) if f.cap > 0]
            if live:
                full_p[rows], full_m[rows] = points, padding
            points, padding = full_p, full_m
        if max(lengths) == 0 and padding_to <= 0:
            points, padding = points[:, :, :0], padding[:, :0]
        up = lambda ts: torch.stack(ts).to(dev)
        return points, up([f.R for f in frames]), up([f.T for f in frames]), padding, up([f.calib for f in frames])


def collate_each(frames: Sequence[PointCloud], padding_to: int = -1, extra=None):
    """ToTensor(padding_to) on every frame ON ITS OWN, for a group of frames at once: -> (per frame (pcd (3,P), padding (P,)
    bool) on the GPU, the lengths, `extra` on the host).  P = padding_to, or with padding_to <= 0 the frame's own length, as
    the reference's ToTensor pads (transforms.py:69-98) -- so frame f equals collate_frames([f], padding_to), but the whole
    group costs ONE host synchronisation: the lengths, every deferred error flag and `extra` (an int32 tensor on the GPU the
    caller wants on the host: the ingest counts of a scene loader) come back together."""
    frames = list(frames)
    if not frames:
        raise ValueError("no frames")
    dev = frames[0].device
    with torch.cuda.device(dev):
        cur = torch.cuda.current_stream(dev)
        for f in frames:
            if f._stream is not None and f._stream != cur:
                cur.wait_stream(f._stream)
                for t in (f.xyz, f.count):
                    t.record_stream(cur)
                f._stream = None
        flags = [(st, msg) for f in frames for st, msg in f._flags]
        live = [k for k, f in enumerate(frames) if f.cap > 0]
        P = int(padding_to) if padding_to > 0 else max([frames[k].cap for k in live] + [1])
        rows = [st.flatten() for st, _ in flags]
        if live:
            points, padding, status = _pack([frames[k] for k in live], P, dev)
            rows.append(status.flatten())
        if extra is not None:
            rows.append(extra.flatten().to(torch.int32))
        _SYNCS[0] += 1
        host = torch.cat(rows).cpu().tolist() if rows else []      # the one host sync of the group
        for f in frames:
            f._flags = []
        for k, (_, msg) in enumerate(flags):
            if host[2 * k + 1]:
                raise ValueError(msg)
        base = 2 * len(flags)
        lengths = [0] * len(frames)
        for j, k in enumerate(live):
            lengths[k] = host[base + 2 * j]
            if padding_to > 0 and host[base + 2 * j + 1]:
                raise RuntimeError(f"The number of Point Cloud ({lengths[k]}) is greater than `padding_to` ({P})")
        extra_host = host[base + 2 * len(live):]
        out, row = [], {k: j for j, k in enumerate(live)}
        for k, (f, n) in enumerate(zip(frames, lengths)):
            f._host_n = n
            if k not in row:
                Pk = P if padding_to > 0 else 0
                out.append((torch.zeros(3, Pk, device=dev), torch.ones(Pk, device=dev, dtype=torch.bool)))
            elif padding_to > 0:
                out.append((points[row[k]], padding[row[k]]))
            else:
                out.append((points[row[k], :, :n].contiguous(), padding[row[k], :n].contiguous()))
        return out, lengths, extra_host


def to_tensor(pcd, padding_to=-1, use_calib=False, use_norm=False, use_uvd=False, use_image=False):
    """PointCloud.to_tensor (transforms.py:69-98) for one frame: (pcd (3,P), R, T, padding (P,)[, calib]) on the GPU"""
    if use_norm or use_uvd or use_image:
        raise NotImplementedError("ToTensor(use_norm | use_uvd | use_image) is not carried by the GPU transforms")
    pts, R, T, pad, calib = collate_frames([pcd], padding_to)
    return (pts[0], R[0], T[0], pad[0], calib[0]) if use_calib else (pts[0], R[0], T[0], pad[0])


def transform_frames(pcds: Sequence[PointCloud], transform, streams: int = 4, rng="reference", return_draws=False):
    """run `transform` (a chain WITHOUT its ToTensor) over every frame, the frames' kernels spread over `streams` HIP
    streams as preprocess_scans does; hand the result to collate_frames, which joins the streams.  One DrawSource serves
    the whole batch in frame order (a paired RandomRT sees the frames in that order)."""
    pcds = list(pcds)
    if not pcds:
        return ([], []) if return_draws else []
    dev = pcds[0].device
    with torch.cuda.device(dev), draws(rng, record=return_draws) as src:
        cur = torch.cuda.current_stream(dev)
        side = [torch.cuda.Stream(device=dev) for _ in range(max(1, min(streams, len(pcds))))]
        for st in side:
            st.wait_stream(cur)
        for b, pcd in enumerate(pcds):
            st = side[b % len(side)]
            for t in (pcd.xyz, pcd.idx, pcd.count):
                t.record_stream(st)
            with torch.cuda.stream(st):
                src.mark(b)
                out = transform(pcd)
                assert out is pcd or isinstance(out, PointCloud), "transform_frames runs the chain without its ToTensor"
                pcds[b] = out
                out._stream = st
    return (pcds, src.records) if return_draws else pcds


# ------------------------------------------------------------------------------------------------------------
# the draw source
# ------------------------------------------------------------------------------------------------------------
class DrawSource:
    """Where every random number of the class layer comes from (module docstring).  With `record`, `records` lists what
    was applied as (functional name, keyword arguments): `replay(pcd, records)` repeats it through the functional layer."""

    def __init__(self, rng="reference", record=False):
        self.reference = isinstance(rng, str)
        if self.reference:
            if rng != "reference":
                raise ValueError("rng is 'reference' or a torch.Generator on the GPU")
            self._py, self._cpu, self._gen = _pyrandom, None, None
        else:
            if not isinstance(rng, torch.Generator) or rng.device.type != "cuda":
                raise ValueError("rng is 'reference' or a torch.Generator on the GPU")
            # host stream for the scalar draws: a function of the generator's seed and offset (no device read); the offset
            # moves on so that the next source of this generator draws other numbers
            state = rng.get_state()                       # host bytes: [seed, philox offset]
            seed, off = state.view(torch.int64).tolist()[:2]
            state.view(torch.int64)[1] = off + 4
            rng.set_state(state)
            self._py = _pyrandom.Random(seed * 0x9E3779B97F4A7C15 + off)
            self._cpu = torch.Generator().manual_seed(self._py.getrandbits(62))
            self._gen = rng
        self.record = record
        self.records = []

    def mark(self, frame):
        if self.record:
            self.records.append(("frame", {"index": frame}))

    def note(self, name, **kw):
        if self.record:
            self.records.append((name, kw))

    # ---- scalar draws (host)
    def random(self):
        return self._py.random()

    def uniform(self, a, b):
        return self._py.uniform(a, b)

    def randint(self, a, b):
        return self._py.randint(a, b)

    def choices(self, population, weights=None):
        return self._py.choices(population, weights=weights)

    def rand3(self):
        return torch.rand(size=(3,)) if self.reference else torch.rand(size=(3,), generator=self._cpu)

    def normal31(self, mean, std):
        if self.reference:
            return torch.normal(size=(3, 1), mean=mean, std=std)
        return torch.normal(mean, std, size=(3, 1), generator=self._cpu)

    # ---- per-point draws.  `n` = a callable giving the frame's current length (a host synchronisation in the reference
    # mode, never called in the generator mode), cap = its capacity, count = its device count
    def _up(self, host, cap, dev, fill):
        buf = torch.full((cap,) + tuple(host.shape[1:]), fill, device=dev, dtype=host.dtype)
        buf[:host.shape[0]] = host.to(dev)
        return buf

    def rand_points(self, n, cap, dev):
        if self.reference:
            return self._up(torch.rand(size=(n(),)), cap, dev, 1.0)
        return torch.rand(cap, device=dev, generator=self._gen)

    def normal_points(self, n, cap, dev, mean, std):
        if self.reference:
            j = torch.normal(size=(n(), 3), mean=mean, std=std).clamp(min=-3 * std, max=3 * std)
            return self._up(j, cap, dev, 0.0)
        return torch.normal(mean, std, size=(cap, 3), generator=self._gen, device=dev).clamp(min=-3 * std, max=3 * std)

    def perm(self, n, cap, dev, count):
        if self.reference:
            return torch.randperm(n()).to(device=dev, dtype=torch.int32)
        keys = torch.rand(cap, device=dev, generator=self._gen)
        keys = torch.where(torch.arange(cap, device=dev) < count, keys, torch.full_like(keys, float("inf")))
        return torch.sort(keys, stable=True).indices.to(torch.int32)


_ACTIVE = threading.local()    # .stack: the `draws()` blocks open in THIS thread (the loader's thread has a stack of its own)


def _stack() -> List[DrawSource]:
    try:
        return _ACTIVE.stack
    except AttributeError:
        _ACTIVE.stack = []
        return _ACTIVE.stack


def _source() -> DrawSource:
    stack = _stack()
    return stack[-1] if stack else _DEFAULT


@contextlib.contextmanager
def draws(rng="reference", record=False):
    """the DrawSource the class layer uses inside the block, in the calling thread"""
    src = rng if isinstance(rng, DrawSource) else DrawSource(rng, record)
    stack = _stack()
    stack.append(src)
    try:
        yield src
    finally:
        stack.pop()


def replay(pcd, records):
    """apply what a DrawSource recorded through the functional layer"""
    for name, kw in records:
        if name != "frame":
            pcd = globals()[name](pcd, **kw)
    return pcd


# ------------------------------------------------------------------------------------------------------------
# class layer: the reference's names and constructor signatures
# ------------------------------------------------------------------------------------------------------------
class _Repr:
    def __repr__(self):
        return f"{self.__class__.__name__}({', '.join(f'{k}={v}' for k, v in vars(self).items() if not k.startswith('_'))})"


class Compose:
    def __init__(self, transforms: List):
        self.transforms = transforms

    def __call__(self, pcd, rng=None, return_draws=False):
        if rng is None and not return_draws:
            for t in self.transforms:
                pcd = t(pcd)
            return pcd
        with draws("reference" if rng is None else rng, record=return_draws) as src:
            for t in self.transforms:
                pcd = t(pcd)
        return (pcd, src.records) if return_draws else pcd

    def __repr__(self):
        return self.__class__.__name__ + "(" + "".join(f"\n    {t}" for t in self.transforms) + "\n)"


class RandomChoice:
    def __init__(self, transforms, p=None):
        if p is not None and not isinstance(p, Sequence):
            raise TypeError("Argument p should be a sequence")
        self.transforms, self.p = transforms, p

    def __call__(self, pcd):
        return _source().choices(self.transforms, weights=self.p)[0](pcd)

    def __repr__(self):
        return self.__class__.__name__ + "(" + "".join(f"\n    {t}" for t in self.transforms) + f"\n)(p={self.p})"


def _apply(name, pcd, **kw):
    _source().note(name, **kw)
    return globals()[name](pcd, **kw)


class GroundFilter(_Repr):
    def __init__(self, img_len: int, img_width: int, grid_width: float, ground_height: float, preserve_sparse_ground: bool = True):
        self.img_len, self.img_width, self.grid_width = img_len, img_width, grid_width
        self.ground_height, self.preserve_sparse_ground = ground_height, preserve_sparse_ground

    def __call__(self, pcd):
        return _apply("ground_filter", pcd, img_len=self.img_len, img_width=self.img_width, grid_width=self.grid_width,
                      ground_height=self.ground_height, preserve_sparse_ground=self.preserve_sparse_ground)


class OutlierFilter(_Repr):
    def __init__(self, nb_neighbors: int, std_ratio: float):
        self.nb_neighbors, self.std_ratio = nb_neighbors, std_ratio

    def __call__(self, pcd):
        return _apply("outlier_filter", pcd, nb_neighbors=self.nb_neighbors, std_ratio=self.std_ratio)


class LowPassFilter(_Repr):
    def __init__(self, normals_radius: float, normals_num: int, filter_std: float, flux: int = 2, max_remain: int = -1):
        self.normals_radius, self.normals_num, self.filter_std = normals_radius, normals_num, filter_std
        self.flux, self.max_remain = flux, max_remain

    def __call__(self, pcd):
        return _apply("lowpass_filter", pcd, normals_radius=self.normals_radius, normals_num=self.normals_num,
                      filter_std=self.filter_std, flux=self.flux, max_remain=self.max_remain)


class VerticalCorrect(_Repr):
    def __init__(self, angle: float):
        self.angle = angle

    def __call__(self, pcd):
        return _apply("vertical_correct", pcd, angle=self.angle)


class VoxelSample(_Repr):
    def __init__(self, voxel_size: float, retention="center", num: int = None):
        assert retention in ["first", "center"], f"'{retention}' is not a supported retention method, " \
                                                 f"please use 'first' or 'center'"
        self.voxel_size, self.retention, self.num = voxel_size, retention, num

    def __call__(self, pcd):
        return _apply("voxel_sample", pcd, voxel_size=self.voxel_size, retention=self.retention, num=self.num)


class FarthestPointSample(_Repr):
    def __init__(self, num):
        self.num = num

    def __call__(self, pcd):
        return _apply("farthest_point_sample", pcd, num=self.num)


class RandomSample(_Repr):
    def __init__(self, num):
        self.num = num

    def __call__(self, pcd):
        src = _source()
        if src.reference and pcd.nbr_point <= self.num:   # the reference draws nothing for a short frame
            return pcd
        if pcd.cap <= self.num:
            return pcd
        perm = src.perm(lambda: pcd.nbr_point, pcd.cap, pcd.device, pcd.count)
        return _apply("random_sample", pcd, num=self.num, perm=perm)


class DistanceSample(_Repr):
    def __init__(self, min_dis: float, max_dis: float):
        self.min_dis, self.max_dis = min_dis, max_dis

    def __call__(self, pcd):
        return _apply("distance_sample", pcd, min_dis=self.min_dis, max_dis=self.max_dis)


class CoordinatesNormalization(_Repr):
    def __init__(self, ratio: float):
        self.ratio = ratio

    def __call__(self, pcd):
        return _apply("coordinates_normalization", pcd, ratio=self.ratio)


class RandomShuffle(_Repr):
    def __init__(self, p: float = 1.0):
        self.p = p

    def __call__(self, pcd):
        src = _source()
        if src.random() > self.p:
            return pcd
        return _apply("random_shuffle", pcd, perm=src.perm(lambda: pcd.nbr_point, pcd.cap, pcd.device, pcd.count))


class RandomDrop(_Repr):
    def __init__(self, max_ratio: float, p: float = 1.0):
        self.max_ratio, self.p = max_ratio, p

    def __call__(self, pcd):
        src = _source()
        if src.random() > self.p:
            return pcd
        ratio = src.uniform(0, self.max_ratio)
        return _apply("random_drop", pcd, ratio=ratio, u=src.rand_points(lambda: pcd.nbr_point, pcd.cap, pcd.device))


def shield_wedges(src, angle_range, dis_range, max_num):
    """the wedges of one RandomShield call (transforms.py:457-469) in the reference's float32 tensor arithmetic:
    rows (start, end, wraps, dis_threshold), `end` reduced by 360 where the wedge passes 180 degrees"""
    rows = []
    for i in range(src.randint(1, max_num)):
        angle, dis, direction = src.rand3()
        angle = (angle * (angle_range[1] - angle_range[0]) + angle_range[0]) / (i + 1)
        dis = dis * (dis_range[1] - dis_range[0]) + dis_range[0]
        start = direction * 360 - 180
        end = start + angle
        wraps = not bool(end <= 180)
        rows.append([float(start), float(end - 360) if wraps else float(end), float(wraps), float(dis)])
    return np.asarray(rows, dtype=np.float32)


class RandomOcclusion(_Repr):
    def __init__(self, angle_range: list, dis_range: list, max_num: int, p: float = 0.1):
        if max_num > MAX_WEDGES:
            raise ValueError(f"max_num is at most {MAX_WEDGES}")
        self.angle_range, self.dis_range, self.max_num, self.p = angle_range, dis_range, max_num, p

    def __call__(self, pcd):
        src = _source()
        if src.random() > self.p:
            return pcd
        return _apply("random_shield", pcd, wedges=shield_wedges(src, self.angle_range, self.dis_range, self.max_num))


def euler_matrix(x, y, z):
    """R_x(x) R_y(y) R_z(z) as the reference builds it: cos / sin of the float32 angles in Python doubles, the three
    matrices rounded to float32, the products in float32 (transforms.py:502-505)"""
    cx, sx, cy, sy, cz, sz = math.cos(x), math.sin(x), math.cos(y), math.sin(y), math.cos(z), math.sin(z)
    R_x = torch.tensor([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    R_y = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    R_z = torch.tensor([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return R_x @ R_y @ R_z


class RandomRT(_Repr):
    def __init__(self, r_mean: float = 0, r_std: float = 3.14, t_mean: float = 0, t_std: float = 1, p: float = 1.0,
                 pair: bool = True):
        self.r_mean, self.r_std, self.t_mean, self.t_std, self.p, self.pair = r_mean, r_std, t_mean, t_std, p, pair
        self.flag = True

    def __call__(self, pcd):
        src = _source()
        if src.random() > self.p:
            return pcd
        first = self.pair and self.flag          # the first frame of a pair turns freely about z, the second within r_std of it
        x, y, z = (src.rand3() - 0.5) * 2 * (torch.pi if first else self.r_std)
        R_aug = euler_matrix(x / 10, y / 10, z)
        if self.pair:
            if first:
                self.random_R = R_aug
            else:
                R_aug = R_aug @ self.random_R
            self.flag = not self.flag
        if self.t_std > 0:
            T_aug = src.normal31(self.t_mean, self.t_std)
            T_aug[2] /= 2
        else:
            T_aug = torch.zeros(size=(3, 1))
        return _apply("random_rt", pcd, R_aug=R_aug, T_aug=T_aug)


class RandomPosJitter(_Repr):
    def __init__(self, mean: float = 0, std: float = 0.05, p: float = 1.0):
        self.mean, self.std, self.p = mean, std, p

    def __call__(self, pcd):
        src = _source()
        if src.random() > self.p:
            return pcd
        jitter = src.normal_points(lambda: pcd.nbr_point, pcd.cap, pcd.device, self.mean, self.std)
        return _apply("random_pos_jitter", pcd, jitter=jitter)


class Deskew(_Repr):
    """motion: "frame" (the frame's own `sweep_motion`, as lidar_sim sets it on frames simulated with sweep motion), a (4,4)
    array, or a callable pcd -> (4,4) (constant_velocity_motion of the caller's last two poses, for one).  Not one of the
    reference's transforms: it assumes compensated scans."""

    def __init__(self, motion="frame", time="column", azimuth_steps=None, reference=0.0):
        self.motion, self.time, self.azimuth_steps, self.reference = motion, time, azimuth_steps, reference

    def __call__(self, pcd):
        if isinstance(self.motion, str):
            if self.motion != "frame":
                raise ValueError("motion is 'frame', a (4,4) array or a callable pcd -> (4,4)")
            if pcd.sweep_motion is None:
                raise ValueError("Deskew('frame'): this frame carries no sweep_motion (it was not taken with sweep motion, or "
                                 "it has been deskewed already)")
            motion = pcd.sweep_motion
        else:
            motion = self.motion(pcd) if callable(self.motion) else self.motion
        return _apply("deskew", pcd, motion=np.asarray(motion, np.float64), time=self.time, azimuth_steps=self.azimuth_steps,
                      reference=self.reference)


class ToGPU(_Repr):
    """accepted and does nothing: the frame lives on the GPU until ToTensor"""

    def __init__(self):
        self.has_gpu = True

    def __call__(self, pcd):
        return pcd


class ToCPU(_Repr):
    """accepted and does nothing: the frame lives on the GPU until ToTensor"""

    def __call__(self, pcd):
        return pcd


class ToTensor(_Repr):
    def __init__(self, use_norm: bool = False, use_uvd: bool = False, padding_to: int = -1, use_image: bool = False,
                 use_calib: bool = False):
        if use_norm or use_uvd or use_image:
            raise NotImplementedError("ToTensor(use_norm | use_uvd | use_image) is not carried by the GPU transforms")
        self.use_norm, self.use_uvd, self.padding_to, self.use_image, self.use_calib = use_norm, use_uvd, padding_to, use_image, use_calib

    def __call__(self, pcd):
        return to_tensor(pcd, padding_to=self.padding_to, use_calib=self.use_calib)


pointcloud_transforms = {
    "GroundFilter": GroundFilter,
    "OutlierFilter": OutlierFilter,
    "LowPassFilter": LowPassFilter,
    "VerticalCorrect": VerticalCorrect,
    "VoxelSample": VoxelSample,
    "FarthestPointSample": FarthestPointSample,
    "RandomSample": RandomSample,
    "DistanceSample": DistanceSample,
    "CoordinatesNormalization": CoordinatesNormalization,
    "RandomShuffle": RandomShuffle,
    "RandomDrop": RandomDrop,
    "RandomShield": RandomOcclusion,
    "RandomRT": RandomRT,
    "RandomPosJitter": RandomPosJitter,
    "ToGPU": ToGPU,
    "ToCPU": ToCPU,
    "ToTensor": ToTensor,
}


def get_transforms(args_dict: dict, return_list: bool = False):
    """the chain a config's `transforms` dict names; 'RandomChoice' nests {'transforms': {...}, 'p': [...]}"""
    out = []
    for key, value in args_dict.items():
        if key == "RandomChoice":
            out.append(RandomChoice(transforms=get_transforms(value["transforms"], return_list=True), p=value["p"]))
        else:
            out.append(pointcloud_transforms[key](**value))
    return out if return_list else Compose(transforms=out)


class PointCloudTransforms:
    """args.transforms -> the chain.  mode 'train': chain(pcd); mode 'infer': (*chain(pcd), original xyz (N,3))."""

    def __init__(self, args, mode="train"):
        assert mode in ["train", "infer"]
        self.args, self.mode = args, mode
        self.transforms = get_transforms(args.transforms)

    def __call__(self, pcd):
        if self.mode == "train":
            return self.transforms(pcd)
        original = pcd.points().clone()
        return (*self.transforms(pcd), original)


_DEFAULT = DrawSource("reference")
