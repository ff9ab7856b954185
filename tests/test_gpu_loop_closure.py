"""GPU: the loop closer end to end (deeppointmap_amd/loop_closure.py) on two laps of a simulated circuit.

lidar_sim.street_scene(2, blocks=(1, 1)) seen by 16 beams x 256 columns without noise from circuit(spacing=4, laps=2), about
106 frames: lap 2 passes every place of lap 1 0.3 m further out.  LoopCloser.add is fed the TRUE poses with a yaw drift of
0.002 rad injected into every step, so nothing here depends on the odometry surviving a corner.  At least one loop must be
accepted; no accepted edge may join places further apart in truth than max_offset; every accepted edge must lie within 3 times
the largest distance between refine.icp STARTED FROM THE TRUE RELATIVE POSE and the truth over the same pairs (two starts end
a stop rule apart at the same minimum); the corrected ATE must be strictly below the drifted one; close_loops must accept the
same edges; GeometricSlam must leave LidarOdometry's poses byte for byte.  Recall and precision are logged, not asserted
(test_logs/loop_closure.log).
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_loop_closure_host import drifted  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DRIFT = 0.002


def log(line):
    os.makedirs(os.path.join(ROOT, "test_logs"), exist_ok=True)
    with open(os.path.join(ROOT, "test_logs", "loop_closure.log"), "a") as f:
        f.write(line + "\n")
    print(line)


@pytest.fixture(scope="module")
def world():
    from deeppointmap_amd import lidar_sim as LS
    scene = LS.street_scene(2, blocks=(1, 1))
    model = LS.LidarModel(np.linspace(10.0, -20.0, 16), 256, 0.9, 80.0, range_sigma=0.0, drop_prob=0.0)
    truth = LS.circuit(scene, spacing=4.0, laps=2)
    sim = LS.LidarSimulator(scene, model, device=DEV)
    frames = sim.frames(truth)
    kw = dict(capacity=len(truth), points_per_frame=model.rays, sc=dict(max_range=model.max_range, z_offset=LS.SENSOR_HEIGHT))
    return SimpleNamespace(scene=scene, model=model, truth=truth, sim=sim, frames=frames, given=drifted(truth, DRIFT), kw=kw)


@pytest.fixture(scope="module")
def online(world):
    """the online run over the drifted poses, once: the closer, the corrected poses, host synchronisations per add"""
    from deeppointmap_amd import augment
    from deeppointmap_amd.loop_closure import LoopCloser
    before = [(f.xyz.clone(), f.idx.clone(), f.count.clone()) for f in world.frames[:3]]
    lc = LoopCloser(**world.kw)
    syncs = []
    for f, p in zip(world.frames, world.given):
        s0, c0 = augment.host_syncs(), len(lc.candidates)
        lc.add(f, p)
        syncs.append((augment.host_syncs() - s0, len(lc.candidates) - c0))
    for f, (x, i, c) in zip(world.frames, before):
        assert torch.equal(f.xyz, x) and torch.equal(f.idx, i) and torch.equal(f.count, c)     # the caller's frames keep their bytes
    return SimpleNamespace(lc=lc, corrected=lc.optimise(), syncs=syncs)


def edge_errors(edges, truth):
    from deeppointmap_amd import evaluate
    out = []
    for e in edges:
        X = np.linalg.inv(truth[e.target]) @ truth[e.source]
        D = np.linalg.inv(X) @ e.pose
        out.append((float(np.linalg.norm(X[:3, 3])), float(np.linalg.norm(D[:3, 3])), float(evaluate.rotation_angle(D[:3, :3]))))
    return out


def test_loops_are_found_between_the_laps_and_only_there(world, online):
    lc = online.lc
    assert len(world.truth) >= 100 and len(lc.poses) == len(world.truth)
    assert len(lc.loops) >= 1
    errs = edge_errors(lc.loops, world.truth)
    for e, (sep, t, r) in zip(lc.loops, errs):
        assert e.source - e.target > lc.exclude_recent and sep <= lc.max_offset, (e.source, e.target, sep)
    # recall and precision, logged: frames with an earlier frame (older than exclude_recent) within max_offset in truth
    F = len(world.truth)
    could = [i for i in range(F) if i - lc.exclude_recent > 0 and
             np.linalg.norm(world.truth[:i - lc.exclude_recent, :3, 3] - world.truth[i, :3, 3], axis=1).min() <= lc.max_offset]
    have = {e.source for e in lc.loops}
    log(f"loops: {len(lc.candidates)} candidates verified, {len(lc.loops)} accepted; {len(could)} frames could close a loop, "
        f"{len(have & set(could))} did (recall {len(have & set(could)) / max(len(could), 1):.2f}); accepted edges between places within "
        f"max_offset {sum(sep <= lc.max_offset for sep, _, _ in errs)} of {len(errs)} (precision); largest true separation "
        f"{max(sep for sep, _, _ in errs):.2f} m, fitness {min(e.fitness for e in lc.loops):.2f}..{max(e.fitness for e in lc.loops):.2f}, "
        f"SC distance up to {max(e.distance for e in lc.loops):.4f}")


def test_host_synchronisations_per_add(online):
    for syncs, verified in online.syncs:
        assert syncs == (2 if verified else 1), (syncs, verified)
    assert any(v for _, v in online.syncs) and not all(v for _, v in online.syncs)


def test_accepted_edges_are_where_icp_from_the_truth_ends(world, online):
    from deeppointmap_amd import refine
    lc = online.lc
    src = torch.tensor([e.source for e in lc.loops], device=DEV, dtype=torch.int32)
    dst = torch.tensor([e.target for e in lc.loops], device=DEV, dtype=torch.int32)
    init = np.stack([np.linalg.inv(world.truth[e.target]) @ world.truth[e.source] for e in lc.loops])
    ref = refine.icp(lc.store, lc.lengths, src, dst, torch.from_numpy(init), schedule=lc.schedule, metric=lc.metric, normals=lc.normals)
    assert bool(((ref.status == refine.CONVERGED) | (ref.status == refine.MAX_ITER)).all())
    ref_edges = [e._replace(pose=p) for e, p in zip(lc.loops, ref.pose.cpu().numpy())]
    ref_errs, errs = edge_errors(ref_edges, world.truth), edge_errors(lc.loops, world.truth)
    bound_t, bound_r = 3 * max(t for _, t, _ in ref_errs), 3 * max(r for _, _, r in ref_errs)
    for e, (_, t, r), (_, t0, r0) in zip(lc.loops, errs, ref_errs):
        log(f"edge {e.source} -> {e.target}: from the descriptor's shift {t:.4f} m {r:.5f} rad, from the truth {t0:.4f} m {r0:.5f} rad "
            f"(bounds {bound_t:.4f} m {bound_r:.5f} rad), fitness {e.fitness:.3f}, SC distance {e.distance:.4f}, shift {e.shift}")
    for e, (_, t, r) in zip(lc.loops, errs):
        assert t <= bound_t and r <= bound_r, (e.source, e.target, t, r, bound_t, bound_r)


def test_a_yawed_revisit_is_found_at_its_shift_and_registered(world):
    """lap 2 driven with the sensor turned by ten sectors and a bit: the search must say shift 10 (query column j matches
    candidate column j + s: the query's yaw in the candidate's frame is s * 2 pi / sectors), and the registration started
    there must end where one started from the truth ends"""
    from deeppointmap_amd import refine
    from deeppointmap_amd.augment import PointCloud
    from deeppointmap_amd.loop_closure import _rz, close_loops
    n, per_lap = 30, len(world.truth) // 2
    yaw = 10 * 2 * np.pi / 60 + 0.02
    turned, poses = [], []
    for k in range(n):
        f = world.frames[per_lap + k]
        pts = f.xyz[:int(f.count.item())].double() @ torch.from_numpy(_rz(yaw)[:3, :3]).to(DEV)     # p' = Rz(-yaw) p, as rows
        turned.append(PointCloud(pts.float()))
        poses.append(world.truth[per_lap + k] @ _rz(yaw))
    truth = np.concatenate([world.truth[:n], np.stack(poses)])
    _, edges, lc = close_loops(world.frames[:n] + turned, truth, return_closer=True, **dict(world.kw, exclude_recent=25))
    assert len(edges) >= 1
    assert all(e.shift == 10 and e.target == e.source - n for e in edges), [(e.source, e.target, e.shift) for e in edges]
    src = torch.tensor([e.source for e in edges], device=DEV, dtype=torch.int32)
    dst = torch.tensor([e.target for e in edges], device=DEV, dtype=torch.int32)
    init = np.stack([np.linalg.inv(truth[e.target]) @ truth[e.source] for e in edges])
    ref = refine.icp(lc.store, lc.lengths, src, dst, torch.from_numpy(init), schedule=lc.schedule, metric=lc.metric, normals=lc.normals)
    ref_errs = edge_errors([e._replace(pose=p) for e, p in zip(edges, ref.pose.cpu().numpy())], truth)
    errs = edge_errors(edges, truth)
    bound_t, bound_r = 3 * max(t for _, t, _ in ref_errs), 3 * max(r for _, _, r in ref_errs)
    log(f"yawed revisit: {len(edges)} edges at shift 10; worst error {max(t for _, t, _ in errs):.4f} m {max(r for _, _, r in errs):.5f} rad "
        f"(bounds {bound_t:.4f} m {bound_r:.5f} rad)")
    assert all(t <= bound_t and r <= bound_r for _, t, r in errs)


def test_database_add_describes_like_the_batch_and_every_query_form_searches_alike(world, online):
    from deeppointmap_amd.loop_closure import ScanContext, ScanContextDB
    lc = online.lc
    db = ScanContextDB(ScanContext(**world.kw["sc"]), 8)
    rows = [db.add(f) for f in world.frames[:3]]                       # whole frames, one at a time
    pts = torch.zeros(3, 3, world.model.rays, device=DEV)
    lengths = torch.zeros(3, device=DEV, dtype=torch.int32)
    for k, f in enumerate(world.frames[:3]):
        pts[k] = f.xyz.t()
        lengths[k:k + 1] = f.count
    assert rows == [0, 1, 2] and db.add_batch(pts, lengths) == 3 and db.count == 6
    assert torch.equal(db.raw[:3], db.raw[3:6]) and torch.equal(db.norm[:3], db.norm[3:6]) and torch.equal(db.mask[:3], db.mask[3:6])
    with pytest.raises(ValueError):
        db.add_batch(pts, lengths)
    # rows of the database, scattered rows and explicit descriptors are one search
    want = lc.db.search(range(60, 63), [5, 8, 10], 3)
    for queries in ([60, 61, 62], (lc.db.norm[60:63].clone(), lc.db.mask[60:63].clone())):
        got = lc.db.search(queries, torch.tensor([5, 8, 10], device=DEV, dtype=torch.int32), 3)
        assert all(torch.equal(a, b) for a, b in zip(want, got))
    scattered = lc.db.search([62, 60], [10, 5], 3)
    assert all(torch.equal(a[[2, 0]], b) for a, b in zip(want, scattered))
    every = lc.db.search_all(lc.exclude_recent, lc.k)
    one = lc.db.search([70], [70 - lc.exclude_recent], lc.k)
    assert all(torch.equal(a[70:71], b) for a, b in zip(every, one))


def test_the_correction_lowers_the_ate(world, online):
    from deeppointmap_amd import evaluate
    before, after = evaluate.ate(world.given, world.truth), evaluate.ate(online.corrected, world.truth)
    first = evaluate.ate(world.given, world.truth, "first")["rmse"], evaluate.ate(online.corrected, world.truth, "first")["rmse"]
    log(f"ATE rmse against the exact poses: drifted {before['rmse']:.4f} m (max {before['max']:.4f}), corrected {after['rmse']:.4f} m "
        f"(max {after['max']:.4f}); aligned at the first pose only: {first[0]:.4f} -> {first[1]:.4f} m")
    assert np.isfinite(online.corrected).all() and np.array_equal(online.corrected[0], world.given[0])
    assert after["rmse"] < before["rmse"]


def test_close_loops_accepts_the_same_edges(world, online):
    from deeppointmap_amd.loop_closure import close_loops
    poses, edges = close_loops(world.frames, world.given, **world.kw)
    assert [(e.source, e.target, e.shift) for e in edges] == [(e.source, e.target, e.shift) for e in online.lc.loops]
    worst = max(np.abs(a.pose - b.pose).max() for a, b in zip(edges, online.lc.loops))
    log(f"close_loops: {len(edges)} edges, the same as online; largest difference of an edge pose {worst:.3e}, of a corrected pose "
        f"{np.abs(poses - online.corrected).max():.3e}")
    assert worst < 1e-6 and np.abs(poses - online.corrected).max() < 1e-4


def test_geometric_slam_keeps_the_odometrys_poses_byte_for_byte(world):
    from deeppointmap_amd import lidar_sim as LS
    from deeppointmap_amd.loop_closure import GeometricSlam
    from deeppointmap_amd.odometry import LidarOdometry
    truth = LS.circuit(world.scene, spacing=1.0)[:12]
    frames = world.sim.frames(truth)
    kw = dict(max_range=world.model.max_range, first_pose=truth[0], initial_motion=LS.sweep_delta(truth[0], truth[1]), sample_map=0.25,
              sample_register=0.75, metric="plane")
    odo = LidarOdometry(**kw)
    for f in frames:
        odo.step(f)
    slam = GeometricSlam(odometry=kw, loop=dict(world.kw, capacity=12))
    for f in frames:
        st, accepted = slam.step(f)
        assert accepted == []
    assert len(slam.odometry.poses) == 12 and all(np.array_equal(a, b) for a, b in zip(slam.odometry.poses, odo.poses))
    assert slam.poses.shape == (12, 4, 4) and np.array_equal(slam.poses, np.stack(odo.poses)) and slam.loops == []
