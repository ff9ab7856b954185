"""Geometric loop closure: Scan Context place recognition on the GPU (csrc/scan_context.hip), verification of the candidates
with the batched ICP (refine.icp), and correction of the trajectory with the pose-graph optimiser
(posegraph_optim.global_optimization).  The reference has no counterpart: it detects loops with its learned loop head only,
which runs on untrained weights here.  This gives evaluate.py a complete classical SLAM to judge, the learned loop head a
baseline, and refine.build_refined_table loop pairs that no ground truth picked.

`ScanContext` holds a descriptor's geometry and host tables, `ScanContextDB` preallocated device tensors of descriptors and
the exhaustive search over them.  `LoopCloser.add(pcd, pose)` takes a frame and its pose from ANY source (an odometry, a
learned pipeline, ground truth with drift), looks for earlier frames of the same place, verifies them and grows a pose graph;
`optimise()` returns the corrected trajectory.  `close_loops` is the offline form, `GeometricSlam` the odometry
(odometry.LidarOdometry, composed) with the loop closer behind it; with rewrite_map a correction also reaches the map the next
frame is registered against (LocalMap.rebuild from the stored frames, LidarOdometry.rebase).
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import augment, ops, posegraph_optim, refine
from .odometry import LidarOdometry, _copy
from .refine import CONVERGED, MAX_ITER, IcpResult


class ScanContext:
    """The descriptor of Kim & Kim (IROS 2018): a polar grid of rings x sectors cells out to max_range around the sensor, a cell
    holding the greatest height z + z_offset > 0 of its points (z_offset: the sensor's height above the ground, so that
    ground returns sit near 0).  Points nearer than min_range are left out."""

    def __init__(self, rings: int = 20, sectors: int = 60, max_range: float = 80.0, min_range: float = 1.0, z_offset: float = 2.0):
        self.rings, self.sectors = int(rings), int(sectors)
        self.max_range, self.min_range, self.z_offset = float(max_range), float(min_range), float(z_offset)
        if not 0.0 <= self.min_range <= self.max_range:
            raise ValueError("0 <= min_range <= max_range")
        self.tables = ops.scan_context_tables(self.rings, self.sectors, self.max_range)     # raises on rings / sectors

    def _kw(self):
        return dict(rings=self.rings, sectors=self.sectors, max_range=self.max_range, min_range=self.min_range,
                    z_offset=self.z_offset, tables=self.tables)

    def describe(self, pcd, out=None):
        """an augment.PointCloud in the sensor frame -> (raw (1,rings,sectors), norm (1,rings,sectors) fp32, mask (1,) int64)
        on the device; three launches, no host synchronisation"""
        return ops.scan_context_build(pcd.xyz, pcd.count, out=out, **self._kw())

    def describe_batch(self, pcd: torch.Tensor, lengths: torch.Tensor, out=None):
        """pcd (F,3,N) fp32, lengths (F,) int32 -> (raw, norm (F,rings,sectors), mask (F,))"""
        return ops.scan_context_build_batched(pcd, lengths, out=out, **self._kw())

    def yaw(self, shift) -> float:
        """the query frame's yaw in the candidate's frame for a search result's shift"""
        return float(shift) * 2.0 * math.pi / self.sectors


class ScanContextDB:
    """`capacity` descriptors in preallocated device tensors (raw, norm (capacity,rings,sectors) fp32, mask (capacity,)
    int64) and the search over the first `count` of them."""

    def __init__(self, sc: ScanContext, capacity: int, device=None):
        self.sc, self.capacity, self.count = sc, int(capacity), 0
        if self.capacity < 1:
            raise ValueError("capacity >= 1")
        self.device = torch.device(device) if device is not None else augment._device()
        new = lambda: torch.zeros(self.capacity, sc.rings, sc.sectors, device=self.device, dtype=torch.float32)
        self.raw, self.norm = new(), new()
        self.mask = torch.zeros(self.capacity, device=self.device, dtype=torch.int64)

    def _rows(self, n: int):
        if self.count + n > self.capacity:
            raise ValueError(f"the descriptor database is full (capacity={self.capacity})")
        a, b = self.count, self.count + n
        self.count = b
        return a, (self.raw[a:b], self.norm[a:b], self.mask[a:b])

    def add(self, pcd) -> int:
        """describes an augment.PointCloud into the next row -> the row"""
        row, out = self._rows(1)
        self.sc.describe(pcd, out=out)
        return row

    def add_batch(self, pcd: torch.Tensor, lengths: torch.Tensor) -> int:
        """describes pcd (F,3,N) / lengths (F,) into the next F rows -> the first of them"""
        row, out = self._rows(int(pcd.shape[0]))
        self.sc.describe_batch(pcd, lengths, out=out)
        return row

    def search(self, queries, limits, k: int):
        """queries: (norm (Q,rings,sectors), mask (Q,)) on the device, or rows of this database (a list / range of ints);
        limits (Q,) int32 on the device or ints: query q sees rows 0 .. limits[q]-1 -> dist (Q,k) fp32, row (Q,k) int32,
        shift (Q,k) int32 on the device, ascending, padded with (inf, -1, -1).  No host synchronisation."""
        if self.count < 1:
            raise ValueError("the descriptor database is empty")
        if isinstance(queries, tuple):
            qn, qm = queries
        else:
            rows = list(queries)
            if rows and rows == list(range(rows[0], rows[0] + len(rows))):
                qn, qm = self.norm[rows[0]:rows[0] + len(rows)], self.mask[rows[0]:rows[0] + len(rows)]
            else:
                at = torch.tensor(rows, device=self.device, dtype=torch.long)
                qn, qm = self.norm[at].contiguous(), self.mask[at].contiguous()
        if not isinstance(limits, torch.Tensor):
            limits = torch.tensor([int(v) for v in limits], device=self.device, dtype=torch.int32)
        return ops.scan_context_search(qn, qm, self.norm, self.mask, limits, int(k), rows=self.count)

    def search_all(self, exclude_recent: int, k: int):
        """every row i as a query against the rows below i - exclude_recent: the offline search"""
        limits = torch.clamp(torch.arange(self.count, device=self.device, dtype=torch.int32) - int(exclude_recent), min=0)
        return self.search(range(self.count), limits, k)


class LoopEdge(NamedTuple):
    source: int               # the later frame (the query)
    target: int               # the earlier frame (the candidate)
    pose: np.ndarray          # (4,4) float64: the source frame in the target's frame (source-scan coordinates -> target frame)
    fitness: float
    rmse: float
    distance: float           # the Scan Context distance that proposed the pair
    shift: int


def _rz(a: float) -> np.ndarray:
    out = np.eye(4)
    c, s = math.cos(a), math.sin(a)
    out[:2, :2] = [[c, -s], [s, c]]
    return out


def yaw_between(A, B) -> np.ndarray:
    """(P,) the rotation about z that takes A's heading to B's, in (-pi, pi]: A, B (P,4,4) or (P,3,3)"""
    R = np.swapaxes(np.asarray(A, np.float64)[..., :3, :3], -1, -2) @ np.asarray(B, np.float64)[..., :3, :3]
    return np.arctan2(R[..., 1, 0] - R[..., 0, 1], R[..., 0, 0] + R[..., 1, 1])


def accept_loops(result: IcpResult, init, min_fitness: float, max_offset: float, max_yaw_change: float) -> np.ndarray:
    """(P,) bool: status CONVERGED or MAX_ITER, fitness >= min_fitness, |t| <= max_offset (the two frames see one place), and
    the yaw within max_yaw_change of where the descriptor's shift put it (a registration that turned further than a few
    sectors did not confirm the proposal, it found something else).  result / init: tensors anywhere or numpy."""
    host = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    status, fitness, pose, init = host(result.status), host(result.fitness), host(result.pose).astype(np.float64), host(init)
    ok = ((status == CONVERGED) | (status == MAX_ITER)) & np.isfinite(pose).all(axis=(1, 2))
    safe = np.where(ok[:, None, None], pose, np.eye(4))
    return ok & (fitness >= min_fitness) & (np.linalg.norm(safe[:, :3, 3], axis=1) <= max_offset) & \
        (np.abs(yaw_between(init, safe)) <= max_yaw_change)


def _Rt(X: np.ndarray, dev) -> torch.Tensor:
    """(12,) fp32 on the device: R row-major, then T"""
    return torch.from_numpy(np.concatenate([X[:3, :3].reshape(9), X[:3, 3]]).astype(np.float32)).to(dev)


class LoopCloser:
    """Place recognition, verification and the pose graph.  sc: the descriptor (a ScanContext or its keyword arguments);
    capacity: frames; points_per_frame: room per stored frame (the first that many valid rows of the thinned frame are kept);
    exclude_recent: a frame is compared with frames at least that many before it; k: candidates a frame; max_distance: the
    Scan Context distance up to which a candidate is verified; sample: augment.voxel_sample edge the stored copy is thinned
    with (None: as it is); schedule / metric / normals_radius: refine.icp's; min_fitness, max_offset (m), max_yaw_change
    (rad): accept_loops'; info_radius: ops.information_matrix's.  The defaults of the four thresholds are what
    profiles/sim_loop_closure_eval.md was recorded with.

    `add` synchronises with the host once for the search results, and once more only when there is something to verify;
    both are counted in augment.host_syncs().  The caller's frame keeps its bytes."""

    def __init__(self, sc=None, capacity: int = 4096, points_per_frame: int = 8192, exclude_recent: int = 50, k: int = 4,
                 max_distance: float = 0.1, sample: Optional[float] = 0.5,
                 schedule: Sequence[Tuple[float, int]] = ((3.0, 20), (1.0, 20), (0.3, 20)), metric: str = "plane",
                 min_fitness: float = 0.4, max_offset: float = 5.0, max_yaw_change: float = 0.2, normals_radius: float = 1.0,
                 info_radius: float = 1.0, device=None):
        self.sc = sc if isinstance(sc, ScanContext) else ScanContext(**(sc or {}))
        if metric not in ("point", "plane"):
            raise ValueError("metric is 'point' or 'plane'")
        if not 1 <= int(k) <= ops.SC_MAX_K or exclude_recent < 1 or points_per_frame < 1:
            raise ValueError(f"k in 1..{ops.SC_MAX_K}, exclude_recent >= 1, points_per_frame >= 1")
        self.capacity, self.P, self.exclude_recent, self.k = int(capacity), int(points_per_frame), int(exclude_recent), int(k)
        self.max_distance, self.sample = float(max_distance), sample
        self.schedule, self.metric = [(float(d), int(n)) for d, n in schedule], metric
        self.min_fitness, self.max_offset, self.max_yaw_change = float(min_fitness), float(max_offset), float(max_yaw_change)
        self.normals_radius, self.info_radius = float(normals_radius), float(info_radius)
        self.device = torch.device(device) if device is not None else None
        self.db: Optional[ScanContextDB] = None
        self.poses: List[np.ndarray] = []
        self.counts: List[int] = []          # stored points per frame, known to the host after the frame's read-back
        self.loops: List[LoopEdge] = []
        self.candidates: List[Tuple[int, int, float, int]] = []     # (source, target, distance, shift) of every verified pair
        self._odometry_info: List[torch.Tensor] = []                # (6,6) fp32 on the device, edge i -> i-1 at [i-1]
        self._loop_info: List[torch.Tensor] = []
        self._has_normals: set = set()

    # -- plumbing
    def _ready(self, dev):
        if self.db is None:
            self.device = dev if self.device is None else self.device
            self.db = ScanContextDB(self.sc, self.capacity, self.device)
            self.store = torch.zeros(self.capacity, 3, self.P, device=self.device, dtype=torch.float32)
            self.lengths = torch.zeros(self.capacity, device=self.device, dtype=torch.int32)
            self.normals = torch.zeros(self.capacity, self.P, 3, device=self.device, dtype=torch.float32) if self.metric == "plane" else None

    def _keep(self, pcd, row: int):
        """a thinned copy's first P valid rows -> store[row], lengths[row]; -> the copy's deferred error flags"""
        work = _copy(pcd)
        if self.sample:
            augment.voxel_sample(work, self.sample)
        n = min(work.cap, self.P)
        self.store[row, :, :n] = work.xyz[:n].t()
        self.lengths[row:row + 1] = torch.clamp(work.count, min=0, max=n)
        return work._flags

    def _info(self, source: int, target: int, X: np.ndarray) -> torch.Tensor:
        """ops.information_matrix of the two stored clouds under X (source -> target); the lengths are known to the host"""
        a = self.store[source, :, :self.counts[source]].contiguous()
        b = self.store[target, :, :self.counts[target]].contiguous()
        if a.shape[1] == 0 or b.shape[1] == 0:
            return torch.zeros(6, 6, device=self.device, dtype=torch.float32)
        return ops.information_matrix(a, b, _Rt(X, self.device), self.info_radius)

    def _normals_for(self, frames, force: bool = False):
        """the normals of the stored frames that become ICP targets, once each; no host read (the lengths are known).  force:
        also under the point metric, whose closer holds no normals until somebody asks (GeometricSlam.surface_map)"""
        new = sorted(set(int(f) for f in frames) - self._has_normals)
        if force and new and self.normals is None:
            self.normals = torch.zeros(self.capacity, self.P, 3, device=self.device, dtype=torch.float32)
        if (self.metric == "plane" or force) and new:
            counts = self.counts + [0] * (self.capacity - len(self.counts))
            ops.icp_target_normals(self.store, self.lengths, self.lengths[:0], self.normals_radius, host=(new, counts), out=self.normals)
            self._has_normals.update(new)

    def _verify(self, pairs) -> List[LoopEdge]:
        """pairs [(source, target, distance, shift)] -> the accepted edges: ONE refine.icp call from Rz(shift 2 pi / sectors),
        t = 0, one read-back"""
        if not pairs:
            return []
        self.candidates += pairs
        dev = self.device
        src = torch.tensor([p[0] for p in pairs], device=dev, dtype=torch.int32)
        dst = torch.tensor([p[1] for p in pairs], device=dev, dtype=torch.int32)
        init = np.stack([_rz(self.sc.yaw(p[3])) for p in pairs])
        self._normals_for(p[1] for p in pairs)
        res = refine.icp(self.store, self.lengths, src, dst, torch.from_numpy(init), schedule=self.schedule, metric=self.metric,
                         normals=self.normals)
        back = torch.cat([res.pose.reshape(-1), res.fitness.double(), res.rmse.double(), res.status.double()])
        augment._SYNCS[0] += 1
        host = back.cpu().numpy()
        n = len(pairs)
        pose, fitness, rmse, status = host[:16 * n].reshape(n, 4, 4), host[16 * n:17 * n], host[17 * n:18 * n], host[18 * n:]
        ok = accept_loops(IcpResult(pose, fitness, rmse, None, status.astype(np.int64)), init, self.min_fitness, self.max_offset,
                          self.max_yaw_change)
        return [LoopEdge(p[0], p[1], pose[i].copy(), float(fitness[i]), float(rmse[i]), float(p[2]), int(p[3]))
                for i, p in enumerate(pairs) if ok[i]]

    def _take(self, edges: List[LoopEdge]):
        for e in edges:
            self.loops.append(e)
            self._loop_info.append(self._info(e.source, e.target, e.pose))

    # -- online
    def add(self, pcd, pose) -> List[LoopEdge]:
        """a frame (augment.PointCloud, sensor frame) and its pose (4,4; sensor -> world) -> the loop edges accepted for it"""
        self._ready(pcd.device)
        row = len(self.poses)
        if row >= self.capacity:
            raise ValueError(f"the loop closer is full (capacity={self.capacity})")
        k = self.k
        with torch.cuda.device(self.device):
            flags = self._keep(pcd, row)
            self.db.add_batch(self.store[row:row + 1], self.lengths[row:row + 1])
            dist, cand, shift = self.db.search([row], [max(row - self.exclude_recent, 0)], k)
            back = torch.cat([dist.reshape(-1).double(), cand.reshape(-1).double(), shift.reshape(-1).double(),
                              self.lengths[row:row + 1].double()] + [st[1:2].double() for st, _ in flags])
            augment._SYNCS[0] += 1
            host = back.cpu().numpy()          # the search results, the stored length and the thinning's error flags
            for flag, (_, msg) in zip(host[3 * k + 1:], flags):
                if flag:
                    raise ValueError(msg)
            self.counts.append(int(host[3 * k]))
            self.poses.append(np.array(pose, np.float64).reshape(4, 4))
            if row:
                X = np.linalg.inv(self.poses[row - 1]) @ self.poses[row]
                self._odometry_info.append(self._info(row, row - 1, X))
            pairs = [(row, int(host[k + i]), float(host[i]), int(host[2 * k + i])) for i in range(k)
                     if host[k + i] >= 0 and host[i] <= self.max_distance]
            accepted = self._verify(pairs)
            self._take(accepted)
        return accepted

    def keyframes_near(self, position, radius: float, poses=None, skip=()) -> List[int]:
        """the stored rows whose pose's translation lies within `radius` of `position` (3,), the boundary included, ascending;
        poses (n,4,4): the poses to judge by (a corrected trajectory, say; default: the ones `add` was given); skip: rows
        left out.  Host arithmetic on host poses: no synchronisation."""
        poses = self.poses if poses is None else poses
        if len(poses) == 0:
            return []
        t = np.asarray(poses, np.float64).reshape(-1, 4, 4)[:len(self.poses), :3, 3]
        near = np.linalg.norm(t - np.asarray(position, np.float64).reshape(3), axis=1) <= float(radius)
        skip = set(int(s) for s in skip)
        return [int(i) for i in np.nonzero(near)[0] if int(i) not in skip]

    # -- the graph
    def edges(self):
        """(source, target, X, information) of posegraph_optim.global_optimization: X takes source-scan coordinates into the
        target's frame.  Reads the information matrices back: one host synchronisation."""
        infos = self._odometry_info + self._loop_info
        if not infos:
            return []
        augment._SYNCS[0] += 1
        host = torch.stack(infos).double().cpu().numpy()
        out = []
        for i in range(1, len(self.poses)):
            out.append((i, i - 1, np.linalg.inv(self.poses[i - 1]) @ self.poses[i], _usable(host[i - 1])))
        for e, info in zip(self.loops, host[len(self._odometry_info):]):
            out.append((e.source, e.target, e.pose, _usable(info)))
        return out

    def optimise(self) -> np.ndarray:
        """(n,4,4) float64: the poses after posegraph_optim.global_optimization over the odometry and loop edges, node 0 held"""
        if not self.poses:
            return np.zeros((0, 4, 4))
        poses = np.stack(self.poses)
        if not self.loops:
            return poses
        return optimise_graph(poses, self.edges())


def _usable(info: np.ndarray) -> np.ndarray:
    """an information matrix the optimiser can take: a pair without a single correspondence (all zeros) or with a non-finite
    entry would leave its edge without weight and the graph in pieces; it gets the identity"""
    if not np.isfinite(info).all() or not info.any():
        return np.eye(6)
    return info


def optimise_graph(poses, edges) -> np.ndarray:
    """posegraph_optim.global_optimization with reference node 0 on poses (n,4,4) and edges (source, target, X, info)"""
    return posegraph_optim.global_optimization(np.asarray(poses, np.float64), edges, reference_node=0)


def close_loops(frames, poses, batch_pairs: int = 64, return_closer: bool = False, **kw):
    """The offline form: frames (augment.PointCloud, sensor frame) and their poses (n,4,4) from any source -> (corrected poses
    (n,4,4) float64, accepted edges [LoopEdge]).  One describe_batch, one search_all, ICP in batches of batch_pairs, one
    optimisation; kw: LoopCloser's.  The edges are pairs refine.build_refined_table(pairs=[(e.target, e.source) ...]) can take.
    return_closer: also the LoopCloser that did the work (its candidates, for reports)."""
    frames = list(frames)
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    if len(frames) != len(poses):
        raise ValueError("one pose per frame")
    kw.setdefault("capacity", max(len(frames), 1))
    lc = LoopCloser(**kw)
    if not frames:
        return (poses.copy(), [], lc) if return_closer else (poses.copy(), [])
    if len(frames) > lc.capacity:
        raise ValueError(f"the loop closer is full (capacity={lc.capacity})")
    lc._ready(frames[0].device)
    n, k = len(frames), lc.k
    with torch.cuda.device(lc.device):
        flags = []
        for row, f in enumerate(frames):
            flags += lc._keep(f, row)
        lc.db.add_batch(lc.store[:n], lc.lengths[:n])
        dist, cand, shift = lc.db.search_all(lc.exclude_recent, k)
        back = torch.cat([dist.reshape(-1).double(), cand.reshape(-1).double(), shift.reshape(-1).double(), lc.lengths[:n].double()]
                         + [st[1:2].double() for st, _ in flags])
        augment._SYNCS[0] += 1
        host = back.cpu().numpy()
        for flag, (_, msg) in zip(host[3 * n * k + n:], flags):
            if flag:
                raise ValueError(msg)
        dist, cand, shift = (host[i * n * k:(i + 1) * n * k].reshape(n, k) for i in range(3))
        lc.counts = [int(v) for v in host[3 * n * k:3 * n * k + n]]
        lc.poses = [p.copy() for p in poses]
        for row in range(1, n):
            lc._odometry_info.append(lc._info(row, row - 1, np.linalg.inv(poses[row - 1]) @ poses[row]))
        pairs = [(row, int(cand[row, i]), float(dist[row, i]), int(shift[row, i])) for row in range(n) for i in range(k)
                 if cand[row, i] >= 0 and dist[row, i] <= lc.max_distance]
        for a in range(0, len(pairs), int(batch_pairs)):
            lc._take(lc._verify(pairs[a:a + int(batch_pairs)]))
    out = (lc.optimise(), list(lc.loops))
    return out + (lc,) if return_closer else out


class GeometricSlam:
    """LidarOdometry with a LoopCloser behind it: `step(pcd)` runs LidarOdometry.step, then LoopCloser.add with the pose it
    returned, and optimises the graph after an accepted loop.  `poses` is the corrected trajectory, `odometry.poses` the raw
    one.  odometry / loop: the keyword arguments of LidarOdometry and LoopCloser.

    rewrite_map=False: the local map keeps running in the odometry's frame, so the odometry neither gains nor loses from a
    loop; only the reported trajectory does.  rewrite_map=True: after an accepted loop whose correction of the current pose
    (the corrected pose Pc against the odometry's P) reaches rewrite_min_shift = (metres, radians) in translation OR in
    rotation, the local map is rebuilt (LocalMap.rebuild) from the loop closer's stored frames within keyframe_radius
    (default: the map's max_range) of Pc under their corrected poses, frames whose registration failed left out, and the
    odometry is rebased by C = Pc P^-1 (LidarOdometry.rebase): the next frame is registered against the corrected geometry of
    every earlier visit.  The loop closer never sees the jump: from the first rebase on it is handed the un-rebased chain
    chain_k = chain_{k-1} P'_{k-1}^-1 P'_k (both P' in the odometry's current frame).  LIMIT: the rebuilt map consists of the
    loop closer's thinned copies, at most points_per_frame a frame (and `sample`d), not of the odometry's own inserts; they
    are not deskewed, so rewrite_map with the odometry's deskew raises ValueError."""

    def __init__(self, odometry: Optional[dict] = None, loop: Optional[dict] = None, rewrite_map: bool = False,
                 keyframe_radius: Optional[float] = None, rewrite_min_shift: Tuple[float, float] = (0.0, 0.0)):
        if rewrite_map and (odometry or {}).get("deskew"):
            raise ValueError("rewrite_map with deskew: the loop closer's stored frames are not deskewed")
        self.odometry = LidarOdometry(**(odometry or {}))
        self.loop_closer = LoopCloser(**(loop or {}))
        self.rewrite_map, self.keyframe_radius = bool(rewrite_map), keyframe_radius
        self.rewrite_min_shift = (float(rewrite_min_shift[0]), float(rewrite_min_shift[1]))
        self._corrected: List[np.ndarray] = []
        self._shifted = False       # a correction has happened: later poses follow it
        self._chain: Optional[np.ndarray] = None     # the last pose handed to the loop closer, once the odometry was rebased

    def _rewrite(self, pose: np.ndarray):
        """the map rebuilt around the current frame's corrected pose and the odometry rebased, if the correction is large enough"""
        Pc = self._corrected[-1]
        C = Pc @ np.linalg.inv(pose)
        shift = float(np.linalg.norm(Pc[:3, 3] - pose[:3, 3]))
        turn = float(np.arccos(np.clip((np.trace(C[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))
        if not (shift >= self.rewrite_min_shift[0] or turn >= self.rewrite_min_shift[1]):
            return
        lc, lm = self.loop_closer, self.odometry.local_map
        failed = [i for i, st in enumerate(self.odometry.steps) if st.status not in (CONVERGED, MAX_ITER)]
        corrected = np.stack(self._corrected)
        rows = lc.keyframes_near(Pc[:3, 3], lm.max_range if self.keyframe_radius is None else self.keyframe_radius,
                                 poses=corrected, skip=failed)
        lm.rebuild(lc.store, lc.lengths, rows, corrected[rows], centre=Pc)
        if self._chain is None:
            self._chain = lc.poses[-1]
        self.odometry.rebase(C)

    def step(self, pcd):
        """-> (odometry.OdometryStep, the loop edges accepted for this frame)"""
        previous = self.odometry._pose(-1) if self.odometry.poses else None     # in the odometry's current frame, as st.pose
        st = self.odometry.step(pcd)
        if self._chain is not None:
            self._chain = self._chain @ (np.linalg.inv(previous) @ st.pose)
        accepted = self.loop_closer.add(pcd, st.pose if self._chain is None else self._chain)
        if accepted:
            self._corrected = list(self.loop_closer.optimise())
            self._shifted = True
            if self.rewrite_map:
                self._rewrite(st.pose)
        elif self._shifted:
            # no new loop: the last correction carries on along the odometry's own motion
            self._corrected.append(self._corrected[-1] @ (np.linalg.inv(previous) @ st.pose))
        else:
            self._corrected.append(st.pose.copy())     # nothing corrected yet: the odometry's pose, byte for byte
        return st, accepted

    @property
    def poses(self) -> np.ndarray:
        return np.stack(self._corrected) if self._corrected else np.zeros((0, 4, 4))

    @property
    def loops(self) -> List[LoopEdge]:
        return self.loop_closer.loops

    def surface_rows(self) -> List[int]:
        """the stored frames `surface_map` fuses: all but those whose registration failed (as `_rewrite` leaves them out)"""
        steps = self.odometry.steps
        return [i for i in range(len(self._corrected)) if i >= len(steps) or steps[i].status in (CONVERGED, MAX_ITER)]

    def surface_map(self, voxel_size: float = 0.2, distance: str = "ray", carve: float = 0.0, archive=None, slack: float = 10.0,
                    **kw):
        """-> tsdf.TsdfMap(voxel_size, distance=distance, **kw) holding the loop closer's stored frames fused under the
        corrected `poses`, in one TsdfMap.integrate_frames call and without a host synchronisation.  distance="plane": the
        distance to the tangent plane at each return, with the loop closer's normals of the stored frames (dpm_point_normals
        at its normals_radius; computed here, one launch a frame, for the rows that have none yet).  carve > 0: afterwards one
        TsdfMap.carve_frames call over the same rows with that weight (in full-weight samples).  LIMIT: these are the loop
        closer's thinned copies, at most points_per_frame a frame (and `sample`d), not the frames `step` was given.
        archive: a tsdf.TsdfArchive makes the map ROLL, so that the run may be longer than max_voxels covers: the rows are cut
        into consecutive chunks whose poses stay within `slack` metres of the chunk's first, and per chunk the map is rolled
        to that pose (`TsdfMap.roll` with its default radii and this slack: one synchronisation) and the chunk integrated.
        carve > 0: a second pass over the chunks, roll and carve_frames -- a carve reaches only the voxels that exist, and
        every frame's have to exist before any is carved, as in the call without an archive.  The map comes back with the
        archive filled, and by `roll`'s guarantee tsdf.merged_export(map, archive) is the export of the call without an
        archive, byte for byte; tsdf.merged_mesh and merged_surface give its surface.  Without an archive nothing changes."""
        from .tsdf import TsdfMap
        out = TsdfMap(voxel_size=voxel_size, distance=distance, **kw)
        if not carve >= 0:
            raise ValueError("carve >= 0")
        rows, lc = self.surface_rows(), self.loop_closer
        if rows:
            normals = None
            if distance == "plane":
                lc._normals_for(rows, force=True)
                normals = lc.normals
            if archive is None:
                out.integrate_frames(lc.store, lc.lengths, rows, self.poses[rows], normals=normals)
                if carve > 0:
                    out.carve_frames(lc.store, lc.lengths, rows, self.poses[rows], weight=carve)
                return out
            if not float(slack) > 0.0:
                raise ValueError("slack > 0")
            poses, chunks = self.poses, []
            for r in rows:
                if not chunks or np.linalg.norm(poses[r][:3, 3] - poses[chunks[-1][0]][:3, 3]) > float(slack):
                    chunks.append([])
                chunks[-1].append(r)
            for chunk in chunks:
                out.roll(poses[chunk[0]], archive, slack=slack)
                out.integrate_frames(lc.store, lc.lengths, chunk, poses[chunk], normals=normals)
            for chunk in chunks if carve > 0 else ():
                out.roll(poses[chunk[0]], archive, slack=slack)
                out.carve_frames(lc.store, lc.lengths, chunk, poses[chunk], weight=carve)
        return out
