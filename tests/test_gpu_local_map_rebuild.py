"""GPU: rebuilding the local map from stored keyframes (dpm_local_map_insert_frames, LocalMap.insert_frames / rebuild,
LidarOdometry.rebase, GeometricSlam(rewrite_map=True); DESIGN §7k "Rebuilding the map").

  restatement   the sorted export against tests/local_map_rebuild_restated.py byte for byte on the constructed cases of
                tests/test_local_map_rebuild_host.py (exact poses, lattice points on voxel faces, lengths 0 / below P / above P /
                negative, NaN columns, both range gates at equality), with and without a centre; `outside` equals the restatement's.
  identity      on general poses and clouds: insert_frames = insert of each entry + prune, the list permuted, twice, one replay
                of a captured graph, and without a centre the inserts alone -- all the same bytes.
  contention    64 entries of one cloud under one pose: every sub-cell ends with stamp 0.
  boundary      a voxel exactly on the radius is kept; at the next float32 below it is dropped.
  table size    a 64-slot table holds what lies within the radius of frames that cover 100 voxels.
  host          no synchronisation in insert_frames and rebuild; planes of a rebuilt map are those of the sequential one.
  the gain      a lap-2 frame registered against a map rebuilt from lap-1 frames under the CORRECTED poses lands, relative to
                its lap-1 partner, within the bound test_gpu_loop_closure derives for loop edges, and strictly nearer the truth
                than against a map rebuilt under the drifted poses.
  slam          GeometricSlam(rewrite_map=True) with one forced rebase: same host synchronisations as without the rewrite, and
                the loop closer's odometry edges are the odometry's own motions.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restated as I  # noqa: E402
import lidar_odometry_restated as L  # noqa: E402
from test_local_map_rebuild_host import boundary_case, list_case, restated, table_case  # noqa: E402
from test_loop_closure_host import drifted  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DRIFT = 0.002


def log(line):
    print(line)
    try:
        os.makedirs(os.path.join(ROOT, "test_logs"), exist_ok=True)
        with open(os.path.join(ROOT, "test_logs", "local_map_rebuild.log"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def gpu_map(c, cap_vox=1 << 12):
    from deeppointmap_amd.odometry import LocalMap
    return LocalMap(c.voxel, c.s, cap_vox, c.max_range, c.min_range, origin=c.origin, device=DEV)


def on_device(c):
    return torch.from_numpy(c.store).to(DEV), torch.from_numpy(c.lengths).to(DEV)


def run_frames(g, c, centre="case", radius=None, order=None):
    order = np.arange(len(c.frames)) if order is None else order
    store, lengths = on_device(c)
    return g.insert_frames(store, lengths, c.frames[order], c.poses[order], c.stamps[order],
                           centre=c.centre if isinstance(centre, str) else centre, radius=c.radius if radius is None else radius)


def run_sequential(g, c, centre="case", radius=None, order=None):
    """LocalMap.insert of each list entry with its stamp, then LocalMap.prune"""
    from deeppointmap_amd.augment import PointCloud
    order = np.arange(len(c.frames)) if order is None else order
    store, lengths = on_device(c)
    P = store.shape[2]
    idx = torch.arange(P, device=DEV, dtype=torch.int32)
    for f in order:
        row = int(c.frames[f])
        g.stamp = int(c.stamps[f])
        g.insert(PointCloud.from_buffers(store[row].t().contiguous(), idx, lengths[row:row + 1].clone()), c.poses[f])
    centre = c.centre if isinstance(centre, str) else centre
    if centre is not None:
        g.prune(centre, c.radius if radius is None else radius)
    return g


def exported(m):
    """(the sorted export's bytes, its length)"""
    e = m.export()
    return [a.tobytes() for a in e], len(e[0])


def same_export(g, r, what=""):
    a, b = g.export(), r.export()
    for x, y, name in zip(a, b, ("keys", "sub-cells", "owner words", "coordinates")):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name, x.dtype, y.dtype, x.shape, y.shape)
        assert x.tobytes() == y.tobytes(), (what, name)
    return a


def header(g):
    return g.table[:8].view(torch.int32).cpu().numpy()     # [overflow, outside]


# ---------------------------------------------------------------------------------------------------------------- restatement
SHAPES = [(F, P, 1 + (i + j) % 3) for i, F in enumerate((0, 1, 3, 17)) for j, P in enumerate((1, 255, 256, 257, 1000))]
SHAPES += [(17, 257, 2), (17, 257, 3), (3, 256, 3)]


@pytest.mark.parametrize("F,P,s", SHAPES)
def test_insert_frames_is_the_restatement_byte_for_byte(F, P, s):
    c = list_case(F, P, s)
    for centre in ("case", None):
        g = run_frames(gpu_map(c), c, centre=centre)
        r, _ = restated(c, centre=centre)
        keys = same_export(g, r, f"centre {centre}")[0]
        assert header(g).tolist() == [0, r.outside]
        assert g.stamp == (int(c.stamps.max()) + 1 if F else 0) and g.half == 0
        if F >= 3 and P >= 255:
            assert len(keys) > 50
    if F == 17:
        assert len(restated(c)[0].vox) < len(restated(c, centre=None)[0].vox)     # the filter had something to drop


def test_rows_outside_the_key_range_are_counted_before_the_filter():
    c = list_case(3, 257, 2)
    c.max_range = 1e7
    far = np.array([[2.0e6, 0, 0], [-2.0e6, 1, 1], [0, 3.0e6, 0]], np.float32)
    for f in range(3):
        c.store[c.frames[f], :, 20:23] = far.T
    c.lengths[c.frames] = 257
    g = run_frames(gpu_map(c), c)
    r, _ = restated(c)
    same_export(g, r)
    assert header(g).tolist() == [0, r.outside] and r.outside == 9


# ------------------------------------------------------------------------------------------------------------------- identity
def general_case(F=6, P=1500, seed=5, span=14.0):
    """random clouds in a cube of +-span under general poses, a kilometre from the world's zero with the map's origin there"""
    rng = np.random.default_rng(seed)
    origin = np.array([1000.0, -500.0, 20.0])
    return SimpleNamespace(store=rng.uniform(-span, span, (F + 1, 3, P)).astype(np.float32),
                           lengths=rng.integers(P // 2, P + 1, F + 1).astype(np.int32), frames=rng.permutation(F + 1)[:F].astype(np.int32),
                           stamps=rng.permutation(50)[:F], voxel=0.5, s=3, min_range=2.0, max_range=20.0, origin=origin, radius=7.0,
                           poses=np.stack([I.se3(rng.normal(0, 0.3, 3), rng.uniform(-4, 4, 3) + origin) for _ in range(F)]),
                           centre=I.se3([0.1, 0, 0.4], origin + [0.3, -0.2, 0.1]))


def test_identity_on_the_gpu_in_any_order_twice_and_from_a_captured_graph():
    from deeppointmap_amd import ops
    c = general_case(span=6.0)
    rng = np.random.default_rng(1)
    want = run_sequential(gpu_map(c, 1 << 15), c)
    ref, n = exported(want)
    assert n > 500 and want.overflow == 0
    perm = rng.permutation(len(c.frames))
    for what, m in (("the list", run_frames(gpu_map(c, 1 << 15), c)), ("again", run_frames(gpu_map(c, 1 << 15), c)),
                    ("permuted", run_frames(gpu_map(c, 1 << 15), c, order=perm)),
                    ("sequential, permuted", run_sequential(gpu_map(c, 1 << 15), c, order=perm))):
        assert exported(m)[0] == ref, what
        assert header(m).tolist() == header(want).tolist(), what
    # without a centre: the inserts alone
    free, alone = run_frames(gpu_map(c, 1 << 15), c, centre=None), run_sequential(gpu_map(c, 1 << 15), c, centre=None)
    assert exported(free)[0] == exported(alone)[0] and exported(free)[1] > n
    # one replay of a captured graph: clear + insert_frames on tensors that are on the device already
    g = gpu_map(c, 1 << 15)
    g._ready(torch.device(DEV))
    store, lengths = on_device(c)
    rows, poses = torch.from_numpy(c.frames).to(DEV), torch.from_numpy(c.poses).to(DEV)
    stamps, centre = torch.from_numpy(c.stamps.astype(np.int32)).to(DEV), torch.from_numpy(c.centre).to(DEV)

    def work():
        ops.local_map_clear(g.table, g.max_voxels, g.subdivisions)
        ops.local_map_insert_frames(*g._args(), store, lengths, rows, poses, stamps, centre, c.radius, c.min_range, c.max_range)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        work()
    g.table.zero_()                 # not a map any more: the replay has to make it one
    graph.replay()
    torch.cuda.synchronize()
    assert exported(g)[0] == ref, "replayed from a captured graph"


def test_contention_every_sub_cell_ends_with_the_smallest_stamp():
    rng = np.random.default_rng(9)
    cloud = rng.uniform(-6, 6, (1, 3, 2048)).astype(np.float32)
    pose = I.se3([0.1, -0.2, 0.3], [0.5, 0.25, -1.0])
    c = SimpleNamespace(store=cloud, lengths=np.array([2048], np.int32), frames=np.zeros(64, np.int32), poses=np.stack([pose] * 64),
                        stamps=np.arange(63, -1, -1), centre=None, radius=0.0, voxel=1.0, s=2, min_range=0.0, max_range=100.0,
                        origin=np.zeros(3))
    g = run_frames(gpu_map(c), c)
    one = SimpleNamespace(**dict(vars(c), frames=c.frames[:1], poses=c.poses[:1], stamps=np.array([0])))
    keys, sub, owner, xyz = g.export()
    assert len(keys) > 500 and (owner >> 32 == 0).all() and g.stamp == 64
    assert exported(g)[0] == exported(run_frames(gpu_map(one), one))[0]      # the words AND the coordinates of that entry
    same_export(g, restated(c, centre=None)[0])


def test_boundary_voxel_on_the_radius_is_kept_and_dropped_one_float32_below():
    c = boundary_case()
    for radius, n in ((c.radius, 4), (c.below, 0)):
        g = run_frames(gpu_map(c), c, radius=radius)
        keys = same_export(g, restated(c, radius=radius)[0], f"radius {radius!r}")[0]
        assert len(keys) == n and (keys == L.pack_key([3, 4, 0])).all()
        seq = run_sequential(gpu_map(c), c, radius=radius)
        assert exported(seq)[0] == exported(g)[0]


def test_a_small_table_holds_what_lies_within_the_radius():
    c = table_case()
    g = run_frames(gpu_map(c, 64), c)
    keys = same_export(g, restated(c)[0])[0]
    assert len(keys) == 11 and header(g)[0] == 0
    seq = run_sequential(gpu_map(c, 64), c)
    assert seq.overflow > 0                                  # the per-frame inserts need a slot for all 100 voxels first
    free = run_frames(gpu_map(c, 64), c, centre=None)
    assert free.overflow == 100 - 64
    with pytest.raises(ValueError, match="local map is full"):
        free.check()


# ----------------------------------------------------------------------------------------------------------------------- host
def test_no_host_synchronisation_rebuild_empties_first_and_planes_follow():
    from deeppointmap_amd import augment
    c = general_case(F=5, P=900, seed=8, span=3.5)          # dense enough for planes
    store, lengths = on_device(c)
    g = gpu_map(c, 1 << 14)
    other = general_case(F=3, P=400, seed=2)
    run_frames(g, SimpleNamespace(**dict(vars(other), origin=c.origin, voxel=c.voxel, s=c.s)), centre=None)
    g.prune(c.centre, 1e3)                                   # content from elsewhere, and the map on half 1
    assert g.half == 1 and g.n_points > 0
    g.planes()
    before = augment.host_syncs()
    g.insert_frames(store, lengths, c.frames[:2], c.poses[:2], c.stamps[:2], centre=c.centre, radius=c.radius)
    g.rebuild(store, lengths, c.frames, c.poses, c.centre, c.radius)
    assert augment.host_syncs() == before
    assert g.half == 0 and g._planes_stale and g.stamp >= int(c.frames.max()) + 1     # rebuild stamps with the rows
    rows = SimpleNamespace(**dict(vars(c), stamps=c.frames))
    want = run_sequential(gpu_map(c, 1 << 14), rows)
    assert exported(g)[0] == exported(want)[0] and exported(g)[1] > 500 and header(g).tolist() == [0, 0]
    a, b = g.export_planes(), want.export_planes()
    assert len(a[0]) > 100 and int((a[3] >= 0).sum()) > 20
    for x, y, name in zip(a, b, ("keys", "counts", "normals", "w")):
        assert x.tobytes() == y.tobytes(), name
    # radius None is max_range
    g.rebuild(store, lengths, c.frames, c.poses, c.centre)
    assert exported(g)[0] == exported(run_sequential(gpu_map(c, 1 << 14), rows, radius=c.max_range))[0]


def test_the_python_layer_refuses_bad_lists():
    c = list_case(3, 16)
    store, lengths = on_device(c)
    g = gpu_map(c)
    for kw in (dict(frames=[0, 1], stamps=[4, 4]), dict(frames=[0, 99]), dict(frames=[0, 1], stamps=[1]), dict(frames=[-1]),
               dict(frames=[0], stamps=[0xFFFFFFFF]), dict(frames=torch.zeros(1, dtype=torch.int32, device=DEV)),
               dict(frames=[0] * 65536, stamps=list(range(65536)))):      # more entries than a launch takes: 65535
        kw.setdefault("poses", np.tile(np.eye(4), (len(kw["frames"]), 1, 1)))
        with pytest.raises(ValueError):
            g.insert_frames(store, lengths, **kw)
    with pytest.raises(ValueError):
        g.insert_frames(store, lengths, [0, 1], np.eye(4)[None])
    assert g.n_points == 0 and g.stamp == 0


# ------------------------------------------------------------------------------------------------------------------- the gain
@pytest.fixture(scope="module")
def world():
    from deeppointmap_amd import lidar_sim as LS
    from deeppointmap_amd.loop_closure import LoopCloser
    scene = LS.street_scene(2, blocks=(1, 1))
    model = LS.LidarModel(np.linspace(10.0, -20.0, 16), 256, 0.9, 80.0, range_sigma=0.0, drop_prob=0.0)
    truth = LS.circuit(scene, spacing=4.0, laps=2)
    sim = LS.LidarSimulator(scene, model, device=DEV)
    frames = sim.frames(truth)
    given = drifted(truth, DRIFT)
    kw = dict(capacity=len(truth), points_per_frame=model.rays, sc=dict(max_range=model.max_range, z_offset=LS.SENSOR_HEIGHT))
    lc = LoopCloser(**kw)
    for f, p in zip(frames, given):
        lc.add(f, p)
    return SimpleNamespace(scene=scene, model=model, truth=truth, sim=sim, frames=frames, given=given, kw=kw, lc=lc, corrected=lc.optimise())


def relative_error(X, truth, source, target):
    """(metres, radians) between X (source -> target's frame) and the truth's relative pose"""
    from deeppointmap_amd import evaluate
    D = np.linalg.inv(np.linalg.inv(truth[target]) @ truth[source]) @ X
    return float(np.linalg.norm(D[:3, 3])), float(evaluate.rotation_angle(D[:3, :3]))


def test_a_map_rebuilt_under_the_corrected_poses_registers_lap_2_where_lap_1_was(world):
    """Observed on an MI355X (test_logs/local_map_rebuild.log): six frames, corrected 0.013 .. 0.056 m / 0.0005 .. 0.0018 rad,
    drifted 0.68 .. 3.98 m, bounds 0.434 m / 0.0239 rad."""
    from deeppointmap_amd import refine
    from deeppointmap_amd.odometry import LocalMap
    lc, truth = world.lc, world.truth
    per_lap = len(truth) // 2
    assert len(lc.loops) >= 1
    # the bound of test_accepted_edges_are_where_icp_from_the_truth_ends, computed the same way: 3 x the worst of refine.icp
    # started from the true relative pose over the accepted pairs
    src = torch.tensor([e.source for e in lc.loops], device=DEV, dtype=torch.int32)
    dst = torch.tensor([e.target for e in lc.loops], device=DEV, dtype=torch.int32)
    init = np.stack([np.linalg.inv(truth[e.target]) @ truth[e.source] for e in lc.loops])
    ref = refine.icp(lc.store, lc.lengths, src, dst, torch.from_numpy(init), schedule=lc.schedule, metric=lc.metric, normals=lc.normals)
    assert bool(((ref.status == refine.CONVERGED) | (ref.status == refine.MAX_ITER)).all())
    ref_errs = [relative_error(p, truth, e.source, e.target) for e, p in zip(lc.loops, ref.pose.cpu().numpy())]
    bound_t, bound_r = 3 * max(t for t, _ in ref_errs), 3 * max(r for _, r in ref_errs)
    partner = {}
    for e in lc.loops:                                      # the first accepted lap-1 partner of every lap-2 frame
        if e.source >= per_lap and e.target < per_lap:
            partner.setdefault(e.source, e.target)
    sources = sorted(partner)
    chosen = [sources[k] for k in sorted(set(np.linspace(0, len(sources) - 1, min(6, len(sources))).round().astype(int)))]
    assert len(chosen) >= 1
    results = []
    for i in chosen:
        j, errs = partner[i], {}
        for name, poses in (("corrected", world.corrected), ("drifted", world.given)):
            m = LocalMap(1.0, 3, 1 << 17, world.model.max_range, device=DEV)
            rows = [r for r in lc.keyframes_near(poses[i][:3, 3], m.max_range, poses=poses) if r < per_lap]
            m.rebuild(lc.store, lc.lengths, rows, poses[rows], poses[i])
            res = m.register(world.frames[i], poses[i], [(1.0, 30)], kernel_scale=0.1, metric="plane")
            m.check()
            errs[name] = relative_error(np.linalg.inv(poses[j]) @ res.pose[0].cpu().numpy(), truth, i, j) + (int(res.status), len(rows))
        (tc, rc, sc, nc), (td, rd, sd, nd) = errs["corrected"], errs["drifted"]
        log(f"gain frame {i} (partner {j}): rebuilt from {nc} lap-1 frames; relative to the partner, corrected {tc:.4f} m {rc:.5f} rad "
            f"(status {sc}), drifted {td:.4f} m {rd:.5f} rad (status {sd}); bounds {bound_t:.4f} m {bound_r:.5f} rad")
        results.append((i, tc, rc, td, rd))
    for i, tc, rc, td, rd in results:
        assert tc <= bound_t and rc <= bound_r, (i, tc, rc, bound_t, bound_r)
        assert tc < td, (i, tc, td)


# ----------------------------------------------------------------------------------------------------------------------- slam
def run_slam(world, frames, truth, rewrite, at):
    """GeometricSlam over `frames` with a loop edge (at -> 0, the truth's relative pose) taken into the closer's lists at frame
    `at`; -> the slam and the host synchronisations of every step"""
    from deeppointmap_amd import augment
    from deeppointmap_amd import lidar_sim as LS
    from deeppointmap_amd.loop_closure import GeometricSlam, LoopEdge
    kw = dict(max_range=world.model.max_range, first_pose=truth[0], initial_motion=LS.sweep_delta(truth[0], truth[1]), sample_map=0.25,
              sample_register=0.75, metric="plane")
    slam = GeometricSlam(odometry=kw, loop=dict(world.kw, capacity=len(frames)), rewrite_map=rewrite, rewrite_min_shift=(0.0, 0.0))
    lc = slam.loop_closer
    real_add = lc.add

    def add(pcd, pose):
        out = real_add(pcd, pose)
        if len(lc.poses) - 1 == at:
            edge = LoopEdge(at, 0, np.linalg.inv(truth[0]) @ truth[at], 1.0, 0.0, 0.0, 0)
            lc._take([edge])
            out = out + [edge]
        return out
    lc.add = add
    syncs = []
    for f in frames:
        s0 = augment.host_syncs()
        slam.step(f)
        syncs.append(augment.host_syncs() - s0)
    return slam, syncs


def test_geometric_slam_rewrites_the_map_and_rebases_the_odometry(world):
    from deeppointmap_amd import lidar_sim as LS
    from deeppointmap_amd.loop_closure import GeometricSlam
    from deeppointmap_amd.refine import CONVERGED, MAX_ITER
    n, at = 14, 9
    truth = LS.circuit(world.scene, spacing=1.0)[:n]
    frames = world.sim.frames(truth)
    plain, plain_syncs = run_slam(world, frames, truth, False, at)
    slam, syncs = run_slam(world, frames, truth, True, at)
    odo, lc = slam.odometry, slam.loop_closer
    assert syncs == plain_syncs, (syncs, plain_syncs)          # the rewrite costs no host synchronisation of its own
    assert plain.odometry.rebases == [] and len(odo.rebases) == 1 and odo.rebases[0][0] == at + 1
    assert all(np.array_equal(a, b) for a, b in zip(odo.poses[:at + 1], plain.odometry.poses[:at + 1]))
    assert all(st.status in (CONVERGED, MAX_ITER) for st in odo.steps)
    assert odo.local_map.overflow == 0
    C = odo.rebases[0][1]
    worst = 0.0
    for k in range(1, n):
        previous = C @ odo.poses[k - 1] if k == at + 1 else odo.poses[k - 1]
        own = np.linalg.inv(previous) @ odo.poses[k]            # the odometry's own motion, in its frame of the time
        edge = np.linalg.inv(lc.poses[k - 1]) @ lc.poses[k]
        worst = max(worst, float(np.abs(edge - own).max()))
        assert np.linalg.norm(edge[:3, 3]) <= np.linalg.norm(own[:3, 3]) + 1e-9, k
    assert worst < 1e-9, worst
    assert slam.poses.shape == (n, 4, 4) and np.isfinite(slam.poses).all()
    err = [float(np.linalg.norm(p[:3, 3] - t[:3, 3])) for p, t in zip(slam.poses, truth)]
    err_plain = [float(np.linalg.norm(p[:3, 3] - t[:3, 3])) for p, t in zip(plain.poses, truth)]
    log(f"slam with rewrite_map: rebase at {at + 1}, |C - 1| {np.abs(C - np.eye(4)).max():.3e}; largest |edge - own motion| {worst:.3e}; "
        f"position error against the truth at the end {err[-1]:.4f} m (without the rewrite {err_plain[-1]:.4f} m), worst "
        f"{max(err):.4f} m ({max(err_plain):.4f} m); host synchronisations per step {syncs}")
    with pytest.raises(ValueError, match="deskew"):
        GeometricSlam(odometry=dict(deskew=True, azimuth_steps=256), loop=dict(world.kw, capacity=4), rewrite_map=True)
