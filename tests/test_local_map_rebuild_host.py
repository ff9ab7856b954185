"""CPU: the host side of rebuilding the local map from stored keyframes (DESIGN §7k "Rebuilding the map").

  identity        the restatement (tests/local_map_rebuild_restated.py): insert_frames with a centre equals Map.insert of each
                  list entry followed by Map.prune, in every list order, on general poses and random clouds.
  cases           the constructed cases tests/test_gpu_local_map_rebuild.py runs are built here, and their decisions are
                  clear in float64: no offered voxel's centre lies within 1e-3 of the radius unless exactly on it.
  keyframes_near  hand-made poses: the boundary included, `skip`, an empty result, other poses than the closer's own.
  chain rule      GeometricSlam over a scripted odometry with one rebase: the loop closer's consecutive relative poses are the
                  odometry's motions, recorded poses keep their bytes, the prediction survives the rebase.
  entry point     dpm_local_map_insert_frames refuses bad arguments before any HIP call; F = 0 is a no-op.
"""
import itertools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restated as I  # noqa: E402
import lidar_odometry_restated as L  # noqa: E402
import local_map_rebuild_restated as R  # noqa: E402


def _rotations():
    """the 24 rotations with entries in {-1, 0, 1}: fp32 transforms of lattice points under them are exact"""
    out = []
    for p in itertools.permutations(range(3)):
        for sign in itertools.product((1.0, -1.0), repeat=3):
            M = np.zeros((3, 3))
            for r in range(3):
                M[r, p[r]] = sign[r]
            if np.linalg.det(M) > 0:
                out.append(M)
    return out


ROTATIONS = _rotations()
PLANTED = np.array([[1, 0, 0], [5, 12, 0], [5, 12.25, 0], [np.nan, 0, 0], [0.75, 0, 0]], np.float32)   # both gates at equality


def lattice(rng, shape, step=0.25, half=6.0):
    k = int(round(half / step))
    return (rng.integers(-k, k + 1, shape) * step).astype(np.float32)


def list_case(F, P, s=3, seed=0, voxel=1.0, radius=5.0):
    """F list entries over a store of F + 2 rows of P columns: lattice points (voxel and sub-cell faces, negative coordinates),
    lengths 0 / below P / above P / negative, NaN columns, points exactly on both range gates (1 and 13 m), exact poses,
    scattered stamps, a centre whose distances to the voxel centres are square roots of multiples of voxel^2 / 4"""
    rng = np.random.default_rng(1000 * F + 10 * P + s + seed)
    cap = F + 2
    store = lattice(rng, (cap, 3, P))
    lengths = np.array([[P, P - P // 3, 0, P + 5, -3][(r + 1) % 5] for r in range(cap)], np.int32)
    for r in range(cap):
        store[r, :, r % P] = PLANTED[r % 5]
        if P >= 8:
            for j in range(5):
                store[r, :, (r + 1 + j) % P] = PLANTED[j]
    frames = rng.permutation(cap)[:F].astype(np.int32)
    poses = np.tile(np.eye(4), (F, 1, 1))
    for f in range(F):
        poses[f, :3, :3] = ROTATIONS[int(rng.integers(len(ROTATIONS)))]
        poses[f, :3, 3] = rng.integers(-16, 17, 3) * 0.25
    stamps = rng.permutation(4 * cap + 7)[:F].astype(np.int64)
    centre = I.se3([0, 0, 0.3], np.array([0.5, 0.5, 0.5]) * voxel + np.array([1.0, -2.0, 0.0]) * voxel)
    return SimpleNamespace(store=store, lengths=lengths, frames=frames, poses=poses, stamps=stamps, centre=centre, radius=radius,
                           voxel=voxel, s=s, min_range=1.0, max_range=13.0, origin=np.zeros(3))


def boundary_case():
    """voxel 1, the centre at (0.5, 0.5, 0.5), four points in the voxel centred (3.5, 4.5, 0.5) -- exactly 5 away -- and four
    in its neighbour (3.5, 5.5, 0.5); radius 5 and the next float32 below it"""
    store = np.zeros((1, 3, 8), np.float32)
    store[0, :, :4] = np.array([[3.2, 4.2, 0.2], [3.7, 4.2, 0.2], [3.2, 4.7, 0.7], [3.9, 4.9, 0.1]], np.float32).T
    store[0, :, 4:] = np.array([[3.2, 5.2, 0.2], [3.7, 5.2, 0.2], [3.2, 5.7, 0.7], [3.9, 5.9, 0.1]], np.float32).T
    below = float(np.nextafter(np.float32(5.0), np.float32(0.0)))
    return SimpleNamespace(store=store, lengths=np.array([8], np.int32), frames=np.array([0], np.int32), poses=np.eye(4)[None],
                           stamps=np.array([3]), centre=I.se3([0, 0, 0.3], [0.5, 0.5, 0.5]), radius=5.0, below=below, voxel=1.0,
                           s=2, min_range=0.0, max_range=100.0, origin=np.zeros(3))


def table_case():
    """a row of 100 voxels along x, one point each, in two frames: 11 of them lie within 5 m of the centre"""
    store = np.zeros((2, 3, 50), np.float32)
    store[:, 0, :] = (np.arange(100, dtype=np.float32) - 50 + 0.5).reshape(2, 50)
    store[:, 1:, :] = 0.5
    return SimpleNamespace(store=store, lengths=np.array([50, 50], np.int32), frames=np.array([0, 1], np.int32),
                           poses=np.stack([np.eye(4)] * 2), stamps=np.array([0, 1]), centre=I.se3([0, 0, 0], [0.5, 0.5, 0.5]),
                           radius=5.0, voxel=1.0, s=1, min_range=0.0, max_range=1e4, origin=np.zeros(3))


def restated(c, centre="case", radius=None, order=None, sequential=False):
    m = L.Map(c.voxel, c.s, c.origin, c.min_range, c.max_range, np.float32)
    order = np.arange(len(c.frames)) if order is None else order
    centre = c.centre if isinstance(centre, str) else centre
    fn = R.sequential if sequential else R.insert_frames
    offered = fn(m, c.store, c.lengths, c.frames[order], c.poses[order], c.stamps[order], centre, c.radius if radius is None else radius)
    return m, offered


def centre_margin(c, radius=None):
    """over every voxel the case offers, the smallest | |centre - t| - radius | that is not exactly 0, in float64"""
    m, _ = restated(c, centre=None)
    keys = np.array(sorted(m.vox), np.int64)
    ctr = (L.unpack_key(keys).astype(np.float64) + 0.5) * c.voxel
    d = np.linalg.norm(ctr - (c.centre[:3, 3] - c.origin), axis=1) - (c.radius if radius is None else radius)
    return float(np.abs(d[d != 0]).min()) if (d != 0).any() else np.inf, int((d == 0).sum()), len(keys)


# ------------------------------------------------------------------------------------------------------------------- identity
def same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a.export(), b.export()))


def test_restated_insert_frames_is_the_inserts_and_the_prune_in_every_order():
    rng = np.random.default_rng(7)
    F, P = 9, 700
    c = SimpleNamespace(store=rng.uniform(-9, 9, (F, 3, P)).astype(np.float32), lengths=rng.integers(P // 2, P + 1, F).astype(np.int32),
                        frames=np.arange(F, dtype=np.int32), stamps=np.arange(F) + 4, voxel=1.0, s=3, min_range=1.0, max_range=12.0,
                        origin=np.array([100.0, -50.0, 3.0]), radius=6.0,
                        poses=np.stack([I.se3(rng.normal(0, 0.2, 3), rng.uniform(-3, 3, 3) + [100.0, -50.0, 3.0]) for _ in range(F)]),
                        centre=I.se3([0, 0, 0.4], [101.0, -49.5, 3.25]))
    want, _ = restated(c, sequential=True)
    assert len(want.export()[0]) > 500
    for order in (np.arange(F), np.arange(F)[::-1], rng.permutation(F)):
        got, offered = restated(c, order=order)
        assert same(got, want) and got.outside == want.outside and offered >= len(got.export()[0])
        assert same(restated(c, order=order, sequential=True)[0], want)
    # without a centre: the inserts alone, which hold more
    free, _ = restated(c, centre=None)
    assert same(free, restated(c, centre=None, sequential=True)[0]) and len(free.export()[0]) > len(want.export()[0])


@pytest.mark.parametrize("F,P,s", [(1, 1, 3), (3, 255, 1), (3, 256, 2), (17, 257, 3), (3, 1000, 3), (17, 255, 2)])
def test_constructed_cases_are_clear_in_float64_and_obey_the_identity(F, P, s):
    c = list_case(F, P, s)
    margin, on_it, voxels = centre_margin(c)
    assert margin > 1e-3, margin
    got, want = restated(c)[0], restated(c, sequential=True)[0]
    assert same(got, want)
    if F == 17:
        assert on_it >= 1 and 0 < len({k for k in got.vox}) < voxels     # the filter drops voxels, and some sit on the radius


def test_boundary_case_in_float64():
    c = boundary_case()
    margin, on_it, voxels = centre_margin(c)
    assert (margin, on_it, voxels) == (pytest.approx(np.hypot(3.0, 5.0) - 5.0), 1, 2)
    assert np.float32(c.below * c.below) < np.float32(25.0) == np.float32(c.radius * c.radius) and c.below < 5.0
    assert len(restated(c)[0].export()[0]) == 4 and len(restated(c, radius=c.below)[0].export()[0]) == 0
    assert centre_margin(c, c.below)[0] > 4e-7          # at the smaller radius the voxel lies outside by one float32 step of 5


def test_table_case_counts():
    c = table_case()
    got, offered = restated(c)
    assert offered == len(got.vox) == 11 and len(restated(c, centre=None)[0].vox) == 100


# ------------------------------------------------------------------------------------------------------------- keyframes_near
def test_keyframes_near_on_hand_made_poses():
    from deeppointmap_amd import loop_closure as LC
    lc = LC.LoopCloser(capacity=8, points_per_frame=8)
    assert lc.keyframes_near([0, 0, 0], 10.0) == []
    at = [(0, 0, 0), (3, 4, 0), (3, 4, 0.001), (-5, 0, 0), (0, 0, 6), (1, 1, 1)]
    lc.poses = [I.se3([0, 0, 0.1 * k], t) for k, t in enumerate(at)]
    assert lc.keyframes_near([0, 0, 0], 5.0) == [0, 1, 3, 5]                    # exactly 5 away is in, 5.0000001 is not
    assert lc.keyframes_near([0, 0, 0], 5.0, skip=(1, 5, 7)) == [0, 3]
    assert lc.keyframes_near([100, 0, 0], 5.0) == [] and lc.keyframes_near([0, 0, 6], 0.0) == [4]
    moved = np.stack(lc.poses)
    moved[:, :3, 3] += [100.0, 0, 0]
    assert lc.keyframes_near([100, 0, 0], 5.0, poses=moved) == [0, 1, 3, 5]
    assert lc.keyframes_near([100, 0, 0], 5.0, poses=list(moved) + [np.eye(4)]) == [0, 1, 3, 5]     # poses beyond the stored frames


# ----------------------------------------------------------------------------------------------------------------- chain rule
def scripted_slam(motions, loop_at, correction):
    """GeometricSlam(rewrite_map=True) whose odometry follows `motions` in its current frame and whose loop closer accepts a loop
    at frame `loop_at` and then answers optimise() with correction @ its poses; the map records what rebuild was given"""
    from deeppointmap_amd import loop_closure as LC
    from deeppointmap_amd.odometry import CONVERGED, LidarOdometry, OdometryStep

    class Odometry(LidarOdometry):
        def step(self, pcd):
            pose = self.first_pose.copy() if not self.poses else self._pose(-1) @ motions[len(self.poses) - 1]
            out = OdometryStep(pose, 1.0, 0.0, 1, CONVERGED)
            self.poses.append(pose)
            self.steps.append(out)
            return out

    class Closer(LC.LoopCloser):
        store = lengths = None

        def add(self, pcd, pose):
            self.poses.append(np.array(pose, np.float64))
            return ["edge"] if len(self.poses) - 1 == loop_at else []

        def optimise(self):
            return np.stack([correction @ p for p in self.poses])

    class Map:
        max_range = 3.5

        def __init__(self):
            self.calls = []

        def rebuild(self, *a, **kw):
            self.calls.append((a, kw))

    slam = LC.GeometricSlam(loop=dict(capacity=64, points_per_frame=8), rewrite_map=True)
    slam.odometry, slam.loop_closer = Odometry(first_pose=I.se3([0, 0, 0.2], [1.0, 2.0, 0.0])), Closer(capacity=64, points_per_frame=8)
    slam.odometry.local_map = Map()
    return slam


def test_chain_rule_across_a_rebase():
    rng = np.random.default_rng(3)
    n, loop_at = 12, 6
    motions = [I.se3(rng.normal(0, 0.02, 3), [1.0 + 0.1 * rng.normal(), 0.05 * rng.normal(), 0.0]) for _ in range(n - 1)]
    correction = I.se3([0.0, 0.0, 0.05], [0.4, -0.3, 0.02])
    slam = scripted_slam(motions, loop_at, correction)
    odo, lc = slam.odometry, slam.loop_closer
    before = None
    for k in range(n):
        if k == loop_at + 1:
            before = [p.copy() for p in odo.poses]
            predicted = odo.predicted_motion()
            assert np.abs(predicted - motions[loop_at - 1]).max() < 1e-12      # the prediction survived the rebase
        st, accepted = slam.step(None)
        assert bool(accepted) == (k == loop_at)
    assert len(odo.rebases) == 1 and odo.rebases[0][0] == loop_at + 1
    C = odo.rebases[0][1]
    assert np.abs(C - correction).max() < 1e-12                                # Pc P^-1 with Pc = correction @ P
    assert all(np.array_equal(a, b) for a, b in zip(before, odo.poses))        # recorded poses keep their bytes
    # the odometry jumped ...
    jump = np.linalg.inv(odo.poses[loop_at]) @ odo.poses[loop_at + 1]
    assert np.abs(jump - motions[loop_at]).max() > 0.1
    # ... and the loop closer never saw it: its consecutive relative poses are the odometry's motions
    for k in range(1, n):
        rel = np.linalg.inv(lc.poses[k - 1]) @ lc.poses[k]
        assert np.abs(rel - motions[k - 1]).max() < 1e-12, k
    assert all(np.array_equal(a, b) for a, b in zip(lc.poses[:loop_at + 1], odo.poses[:loop_at + 1]))   # before: st.pose itself
    # after the rebase the odometry runs in the corrected frame, and `poses` follows it
    assert np.abs(slam.poses[-1] - odo.poses[-1]).max() < 1e-9
    (args, kw), = odo.local_map.calls
    rows = args[2]
    near = [i for i in range(loop_at + 1) if np.linalg.norm(slam.poses[i][:3, 3] - slam.poses[loop_at][:3, 3]) <= 3.5]
    assert list(rows) == near and 1 < len(near) < loop_at + 1
    assert np.array_equal(kw["centre"], correction @ odo.poses[loop_at]) and np.array_equal(args[3], np.stack([correction @ odo.poses[i] for i in near]))


def test_rewrite_needs_a_shift_and_refuses_deskew():
    from deeppointmap_amd import loop_closure as LC
    with pytest.raises(ValueError, match="deskew"):
        LC.GeometricSlam(odometry=dict(deskew=True, azimuth_steps=64), loop=dict(capacity=4, points_per_frame=8), rewrite_map=True)
    motions = [I.se3([0, 0, 0], [1.0, 0, 0])] * 5
    slam = scripted_slam(motions, 3, I.se3([0, 0, 0.01], [0.05, 0, 0]))
    slam.rewrite_min_shift = (1.0, 0.1)                 # the correction is smaller than both: nothing is rewritten
    for _ in range(6):
        slam.step(None)
    assert slam.odometry.rebases == [] and slam.odometry.local_map.calls == []


# ---------------------------------------------------------------------------------------------------------------- the C entry
def test_entry_point_refuses_bad_arguments_before_any_hip_call():
    import ctypes
    from deeppointmap_amd import _lib
    lib = _lib.load()
    assert "dpm_local_map_insert_frames" in _lib.SIGNATURES and hasattr(lib, "dpm_local_map_insert_frames")
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) & ~255   # never dereferenced: every call below is refused first, or is a no-op
    o = (ctypes.c_double * 3)(0, 0, 0)
    bad_o = (ctypes.c_double * 3)(0, float("nan"), 0)
    names = ("map", "cap_vox", "s", "half", "voxel", "origin", "store", "lengths", "capacity", "P", "frames", "poses", "stamps", "F",
             "centre", "radius", "lo", "hi", "stream")
    good = dict(map=p, cap_vox=64, s=3, half=0, voxel=1.0, origin=ctypes.addressof(o), store=p, lengths=p, capacity=4, P=8, frames=p,
                poses=p, stamps=p, F=2, centre=p, radius=5.0, lo=0.0, hi=10.0, stream=None)
    call = lambda **k: lib.dpm_local_map_insert_frames(*[{**good, **k}[n] for n in names])
    for k in (dict(map=None), dict(map=p + 8), dict(cap_vox=65), dict(s=4), dict(half=2), dict(voxel=0.0), dict(origin=None),
              dict(origin=ctypes.addressof(bad_o)), dict(store=None), dict(lengths=None), dict(capacity=0), dict(P=0), dict(frames=None),
              dict(poses=None), dict(stamps=None), dict(F=-1), dict(F=65536), dict(radius=-1.0), dict(radius=float("nan")),
              dict(lo=-1.0), dict(lo=11.0), dict(hi=float("inf"))):
        assert call(**k) == -1, k
    # an empty list is a no-op whatever the list's pointers are; without a centre the radius is not looked at
    assert call(F=0, store=None, lengths=None, frames=None, poses=None, stamps=None) == 0
    assert call(F=0, centre=None, radius=float("nan")) == 0
