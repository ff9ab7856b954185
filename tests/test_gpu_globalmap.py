"""GPU: the global map (csrc/voxel_map.hip through globalmap.voxel_map) against the fp64 numpy restatement of open3d's
VoxelDownSample (test_globalmap_host.voxel_down_sample_ref), its determinism, limits and edge cases, and the system layer
behind `slam_system.result_maps` (ResultLogger.draw_trajectory / plot_data / export_map)."""
import os

import numpy as np
import pytest
import torch

from test_globalmap_host import read_pcd, transform_fp32, voxel_down_sample_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pose(rng, scale=20.0):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    P = np.eye(4, dtype=np.float32)
    P[:3, :3], P[:3, 3] = R, rng.uniform(-scale, scale, 3)
    return P


def _scans(rng, n_scans, n_pts, spread=15.0, sorted_like_lidar=True):
    clouds, poses = [], []
    for _ in range(n_scans):
        n = int(n_pts) if np.isscalar(n_pts) else int(rng.integers(*n_pts))
        c = rng.normal(scale=spread, size=(3, n)).astype(np.float32)
        if sorted_like_lidar:    # neighbouring points share voxels, as a LiDAR scan in ring / azimuth order does
            c = c[:, np.argsort(np.arctan2(c[1], c[0]) + 10 * np.round(c[2] / 2))]
        clouds.append(np.ascontiguousarray(c))
        poses.append(_pose(rng))
    return clouds, poses


def _world(clouds, poses):
    return np.concatenate([transform_fp32(c, p) for c, p in zip(clouds, poses)], axis=1) if clouds else np.zeros((3, 0), np.float32)


def _run(clouds, poses, vs=0.5, host=(), stats=None):
    from deeppointmap_amd.globalmap import voxel_map
    ts = [torch.from_numpy(c) if i in host else torch.from_numpy(c).to(DEV) for i, c in enumerate(clouds)]
    c, n = voxel_map(ts, torch.from_numpy(np.stack(poses)) if poses else torch.zeros(0, 4, 4), vs, device=DEV, stats=stats)
    torch.cuda.synchronize()
    assert c.device.type == "cuda" and c.dtype == torch.float32 and n.dtype == torch.int32
    return c.cpu().numpy(), n.cpu().numpy()


def _within_ulp(got, want, ulps=1):
    """within `ulps` fp32 ulps of the fp64 value, or within the 1e-9 m accuracy bound of the fixed-point sums (which is
    what decides for centroids within a millimetre of a world axis, where an fp32 ulp is smaller)"""
    tol = np.maximum(ulps * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64), 1e-9)
    return np.abs(got.astype(np.float64) - want) <= tol


def test_interior_points_match_the_restatement_exactly():
    """points >= 1e-3 m from every voxel face (faces of the grid that the transformed points themselves anchor): the same
    voxels in the same order, the same counts, centroids within one fp32 ulp of the fp64 mean"""
    rng = np.random.default_rng(11)
    clouds, poses = _scans(rng, 9, (2000, 9000))
    vs = 0.5
    world = _world(clouds, poses)
    _, _, _, ref = voxel_down_sample_ref(world, vs)
    frac = ref - np.floor(ref)
    keep = ((frac * vs > 1e-3) & ((1 - frac) * vs > 1e-3)).all(axis=0)
    a = 0
    for i, c in enumerate(clouds):
        clouds[i] = np.ascontiguousarray(c[:, keep[a:a + c.shape[1]]])
        a += c.shape[1]
    want_c, want_n, _, ref2 = voxel_down_sample_ref(_world(clouds, poses), vs)
    f2 = ref2 - np.floor(ref2)
    assert ((f2 * vs > 0.9e-3) & ((1 - f2) * vs > 0.9e-3)).all()     # the minimum did not move
    st = {}
    got_c, got_n = _run(clouds, poses, vs, stats=st)
    assert got_n.tolist() == want_n.tolist()
    assert _within_ulp(got_c, want_c).all(), np.abs(got_c - want_c).max()
    assert st["voxels"] == len(want_n) and st["n_points"] == sum(c.shape[1] for c in clouds)
    assert st["workspace_bytes"] <= 64 * st["n_points"] + 8192


def test_random_clouds_differ_only_at_faces():
    """plain random clouds: a voxel may differ only if one of its points lies within 1e-6 (in voxel units) of a face"""
    rng = np.random.default_rng(12)
    clouds, poses = _scans(rng, 12, (5000, 20000), sorted_like_lidar=False)
    vs = 0.3
    world = _world(clouds, poses)
    want_c, want_n, first, ref = voxel_down_sample_ref(world, vs)
    got_c, got_n = _run(clouds, poses, vs)
    min_b = world.astype(np.float64).min(axis=1) - vs / 2
    keyf = lambda xyz: [tuple(k) for k in np.floor((xyz.T - min_b) / vs).astype(np.int64)]
    want = dict(zip(keyf(want_c), zip(want_n, want_c.T)))
    got = dict(zip(keyf(got_c.astype(np.float64)), zip(got_n, got_c.T)))
    near = (np.abs(ref - np.round(ref)) < 1e-6).any(axis=0)
    suspect = set()
    for shift in (-2e-6, 0.0, 2e-6):     # the voxel of a point near a face, and its neighbour across that face
        suspect |= set(keyf((np.floor(ref[:, near] + shift) + 0.5) * vs + min_b[:, None]))
    ulp = np.spacing(np.abs(want_c).astype(np.float32)).astype(np.float64)
    on_face = np.abs((want_c - min_b[:, None]) / vs - np.round((want_c - min_b[:, None]) / vs)) * vs < 2 * ulp
    suspect |= set(keyf(want_c[:, on_face.any(axis=0)]))
    for k in set(want) | set(got):
        if k in suspect:
            continue
        assert k in want and k in got, k
        assert want[k][0] == got[k][0]
        assert _within_ulp(got[k][1], want[k][1]).all()


def test_two_runs_and_permuted_scans_are_bit_identical():
    rng = np.random.default_rng(13)
    clouds, poses = _scans(rng, 10, (3000, 8000))
    c1, n1 = _run(clouds, poses)
    c2, n2 = _run(clouds, poses)
    assert np.array_equal(c1.view(np.uint32), c2.view(np.uint32)) and np.array_equal(n1, n2)
    perm = rng.permutation(len(clouds))
    c3, n3 = _run([clouds[i] for i in perm], [poses[i] for i in perm])
    as_set = lambda c, n: sorted(zip(map(tuple, c.T.view(np.uint32).tolist()), n.tolist()))
    assert as_set(c1, n1) == as_set(c3, n3)
    assert not np.array_equal(c1, c3)          # the order did change: first appearance follows the scan order


def test_host_and_device_clouds_mix_bit_for_bit():
    """ScanCloudStore spills clouds to the host: those pass through the pinned staging buffers (one of them larger than a
    staging buffer, so it is split) and give the all-device result bit for bit"""
    from deeppointmap_amd import globalmap
    rng = np.random.default_rng(14)
    clouds, poses = _scans(rng, 8, (1000, 4000))
    clouds[5] = np.ascontiguousarray(rng.normal(scale=30, size=(3, globalmap.STAGING_POINTS + 12345)).astype(np.float32))
    c1, n1 = _run(clouds, poses)
    c2, n2 = _run(clouds, poses, host={0, 2, 3, 5, 7})
    c3, n3 = _run(clouds, poses, host=set(range(8)))
    for c, n in ((c2, n2), (c3, n3)):
        assert np.array_equal(c1.view(np.uint32), c.view(np.uint32)) and np.array_equal(n1, n)


def test_empty_inputs_and_one_point():
    from deeppointmap_amd.globalmap import voxel_map
    c, n = voxel_map([], torch.zeros(0, 4, 4), 0.5, device=DEV)
    assert c.shape == (3, 0) and n.shape == (0,) and c.is_cuda
    e = torch.zeros(3, 0, device=DEV)
    c, n = voxel_map([e, None, e], torch.eye(4).repeat(3, 1, 1), 0.5)
    assert c.shape == (3, 0) and n.shape == (0,)
    rng = np.random.default_rng(15)
    clouds, poses = _scans(rng, 3, 500)
    got_c, got_n = _run([np.zeros((3, 0), np.float32), clouds[0], np.zeros((3, 0), np.float32), clouds[1]],
                        [poses[2], poses[0], poses[2], poses[1]])
    want_c, want_n, _, _ = voxel_down_sample_ref(_world(clouds[:2], poses[:2]), 0.5)
    assert got_n.tolist() == want_n.tolist() and _within_ulp(got_c, want_c, 1).mean() > 0.999
    got_c, got_n = _run([np.array([[1.25], [-3.0], [7.5]], np.float32)], [np.eye(4, dtype=np.float32)])
    assert got_n.tolist() == [1] and got_c[:, 0].tolist() == [1.25, -3.0, 7.5]


def test_two_million_points_in_one_voxel():
    """contention: every point in one voxel (the run merge carries it through whole waves); the fixed-point sums stay
    exact and the centroid is the fp64 mean"""
    rng = np.random.default_rng(16)
    n = 2_000_000
    c = (np.float32(100.0) + rng.uniform(0, 0.49, size=(3, n)).astype(np.float32))
    c[:, 0] = 100.0                    # the minimum: the voxel spans [99.75, 100.25) + ... on every axis
    c = np.clip(c, 100.0, 100.24).astype(np.float32)
    st = {}
    got_c, got_n = _run([c[:, : n // 2].copy(), c[:, n // 2:].copy()], [np.eye(4, dtype=np.float32)] * 2, stats=st)
    want_c, want_n, _, _ = voxel_down_sample_ref(c, 0.5)
    assert got_n.tolist() == want_n.tolist() == [n]
    assert _within_ulp(got_c, want_c).all()
    assert st["runs"] <= n // 1024 + 2 and st["atomics_per_point"] < 0.01, st


def test_limits_raise():
    from deeppointmap_amd.globalmap import voxel_map
    c = torch.zeros(3, 10, device=DEV)
    for vs in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="voxel_size"):
            voxel_map([c], torch.eye(4)[None], vs)
    bad = c.clone()
    bad[1, 3] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        voxel_map([bad], torch.eye(4)[None], 0.5)
    inf = c.clone()
    inf[0, 0] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        voxel_map([c, inf.cpu()], torch.eye(4).repeat(2, 1, 1), 0.5)
    far = c.clone()
    far[2, 9] = 1.1e6                  # 2.2e6 voxels of 0.5 m > 2^21
    with pytest.raises(ValueError, match="extent"):
        voxel_map([far], torch.eye(4)[None], 0.5)
    with pytest.raises(ValueError, match="fixed-point"):
        voxel_map([c], torch.eye(4)[None], 2.0 ** 28)
    near = c.clone()
    near[2, 9] = 1.0e6                 # 2e6 voxels: within the packing
    cc, nn = voxel_map([near], torch.eye(4)[None], 0.5)
    assert nn.tolist() == [9, 1]


def test_twenty_million_points_against_the_restatement():
    """20 M points (40 scans, ~10 M voxels: hash-table occupancy, probe wrap-around and the 64-bit sums at scale).  The
    restatement's transform is the kernel's fp32 arithmetic bit for bit and both take floor((p - min_b) / vs) in fp64, so
    even points lying exactly on a face (hundreds here) must land in the same voxel: every voxel, in order, with its count,
    and the centroids of a random subset within one fp32 ulp"""
    rng = np.random.default_rng(17)
    clouds, poses = _scans(rng, 40, 500_000, spread=40.0)
    world = _world(clouds, poses)
    st = {}
    got_c, got_n = _run(clouds, poses, 0.5, stats=st)
    want_c, want_n, _, ref = voxel_down_sample_ref(world, 0.5)
    assert (ref == np.floor(ref)).any()        # the data does put points exactly on faces
    assert len(got_n) == len(want_n) and np.array_equal(got_n, want_n)
    sub = rng.choice(len(want_n), size=min(500_000, len(want_n)), replace=False)
    assert _within_ulp(got_c[:, sub], want_c[:, sub]).all()
    assert st["n_points"] == 20_000_000 and st["voxels"] == len(want_n) and st["workspace_bytes"] <= 64 * 20_000_000


# -- the system layer ------------------------------------------------------------------------------------------------------
def _system(cfg_full, result_maps, **kw):
    from test_gpu_consumer import TRACE_SLAM
    from deeppointmap_amd.config import Cfg
    from deeppointmap_amd.decoder import Decoder
    from deeppointmap_amd.encoder import Encoder
    from deeppointmap_amd.system import SlamSystem
    from deeppointmap_amd.weights import init_procedural
    args = Cfg(dict(cfg_full))
    slam = dict(TRACE_SLAM)
    if result_maps is not None:
        slam["result_maps"] = result_maps
    args.device, args.slam_system = DEV, Cfg(slam)
    enc, dec = init_procedural(Encoder(cfg_full)).to(DEV), init_procedural(Decoder(cfg_full)).to(DEV)
    s = SlamSystem(args, enc, dec, system_id=0, **kw)
    s.backend.optimiser = lambda nodes, es, base: None      # as test_gpu_system (the recording skipped open3d)
    return s


def _replay_scans():
    from conftest import T, load_golden
    g = load_golden("slam_trace.npz")
    frames = [T(g[f"frame{i}"]) for i in range(11)]
    for s in range(len(g["order"])):
        p = frames[int(g[f"s{s}.frame"])].unsqueeze(0)
        T_ = torch.tensor([[[0.5 * s], [0.25 * s], [0.0]]])
        yield [p, torch.eye(3).unsqueeze(0), T_, torch.zeros(1, p.shape[2], dtype=torch.bool), None]


def _finish(system):
    rl = system.result_logger
    rl.save_trajectory("trajectory"), rl.save_posegraph("trajectory")
    rl.draw_trajectory("trajectory", draft=False), rl.save_map("trajectory"), rl.export_map("trajectory")


def test_replay_with_result_maps_writes_the_map(cfg_full, tmp_path):
    on, off = tmp_path / "on", tmp_path / "off"
    s_on = _system(cfg_full, True, logger_dir=str(on))
    for d in _replay_scans():
        s_on.step(d)
    _finish(s_on)
    s_off = _system(cfg_full, None, logger_dir=str(off))
    for d in _replay_scans():
        s_off.step(d)
    _finish(s_off)
    assert sorted(os.listdir(off)) == sorted(f"trajectory.{k}" for k in ("allframes.txt", "allsteps.txt", "keyframes.txt",
                                                                          "keysteps.txt", "pg.g2o"))
    assert s_off.backend.map_clouds is None and s_off.backend.gt == {}
    assert sorted(os.listdir(on)) == sorted(os.listdir(off) + ["trajectory.map.jpg", "trajectory.fullpoints.pcd",
                                                               "trajectory.keypoints.pcd"])
    for f in os.listdir(off):
        assert (on / f).read_bytes() == (off / f).read_bytes(), f
    assert (on / "trajectory.map.jpg").stat().st_size > 10_000
    b = s_on.backend
    assert len(b.map_clouds) == len(b.type) and set(b.gt) == set(b.type)
    full, key = read_pcd(str(on / "trajectory.fullpoints.pcd")), read_pcd(str(on / "trajectory.keypoints.pcd"))
    toks = list(b.type)
    world = _world([b.map_clouds[t].cpu().numpy() for t in toks], [b.poses[t].numpy() for t in toks])
    want, want_n, _, _ = voxel_down_sample_ref(world, 0.5)
    assert full.shape == want.shape and np.abs(full - want).max() < 1e-4
    kf = [t for t in toks if b.type[t] == "full"]
    wk, _, _, _ = voxel_down_sample_ref(_world([b.desc[t][-3:].cpu().numpy() for t in kf], [b.poses[t].numpy() for t in kf]), 0.5)
    assert key.shape == wk.shape and np.abs(key - wk).max() < 1e-4
    d = s_on.result_logger.plot_data(draft=False)
    assert np.array_equal(d["full_map"], full[:2].astype(np.float64)) and np.array_equal(d["key_map"], key[:2].astype(np.float64))
    assert np.array_equal(d["gt_xy"], np.stack([0.5 * d["scan_token"], 0.25 * d["scan_token"]], axis=1))   # SE3_gt per scan


def test_multi_thread_mode_gives_step_s_plot_data(cfg_full):
    one = _system(cfg_full, True)
    for d in _replay_scans():
        one.step(d)
    mt = _system(cfg_full, True)
    mt.MT_Init()
    for d in _replay_scans():
        mt.MT_Step(d)
    mt.MT_Done()
    mt.MT_Wait()
    a, b = one.result_logger.plot_data(draft=False), mt.result_logger.plot_data(draft=False)
    assert set(a) == set(b)
    for k in a:
        assert (a[k] is None and b[k] is None) or np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert a["full_map"] is not None and a["key_map"] is not None


def test_ground_truth_crosses_the_message_bus(cfg_full, tmp_path):
    """two AgentSystems with result_maps upload their key frames (the recorded two-agent drive of test_gpu_cloud.py) and a
    cloud back end takes them: its plot_data carries every uploaded scan's SE3_gt, its map every uploaded cloud"""
    from conftest import T, load_golden
    from test_gpu_consumer import TRACE_SLAM
    from test_gpu_multiagent import LocalComm
    from deeppointmap_amd.config import Cfg
    from deeppointmap_amd.consumer import Rank0Consumer
    from deeppointmap_amd.decoder import Decoder
    from deeppointmap_amd.encoder import Encoder
    from deeppointmap_amd.system import AgentSystem, ResultLogger
    from deeppointmap_amd.weights import init_procedural
    scans = load_golden("slam_trace.npz")
    dev = torch.device(DEV)
    enc, dec = init_procedural(Encoder(cfg_full)).to(dev), init_procedural(Decoder(cfg_full)).to(dev)
    args = Cfg(dict(cfg_full))
    args.device, args.slam_system = DEV, Cfg(dict(TRACE_SLAM, result_maps=True))
    comm = LocalComm()
    comm.add_member(0)
    agents = {a: AgentSystem(args, enc, dec, system_id=a, comm_module=comm, device=dev) for a in (1, 2)}
    for a in agents.values():
        a.backend.optimiser = lambda n, e, b: None
    plan = {1: [0, 1, 2, 3, 4, 5], 2: [10, 9, 8, 7, 6, 5]}
    for i in range(6):
        for a in (1, 2):
            p = T(scans[f"frame{plan[a][i]}"]).unsqueeze(0)
            gt_T = torch.tensor([[[100.0 * a + i], [-3.0 * a], [0.5 * i]]])
            agents[a].step([p, torch.eye(3).unsqueeze(0), gt_T, torch.zeros(1, p.shape[2], dtype=torch.bool), None])
    ups = [m for _, _, c, m in comm.sent if c == "UPLOAD_SCAN"]
    assert len(ups) == 12 and all(m["new_scan"]["SE3_gt"] is not None for m in ups)
    cloud = Rank0Consumer(dec, dev, slam_args=dict(TRACE_SLAM, result_maps=True), agent_id=0, loop_targets="others",
                          optimiser=lambda n, e, b: None)
    for m in ups:
        cloud.cloud_step(m["new_scan"], m["odometer_edge"], m["neighbor_edges"])
    d = ResultLogger(cloud, str(tmp_path)).plot_data(draft=False)
    want = {m["new_scan"]["token"]: [100.0 * (m["new_scan"]["token"] >> 16) + (m["new_scan"]["token"] & 0xFFFF),
                                     -3.0 * (m["new_scan"]["token"] >> 16)] for m in ups}
    assert sorted(d["scan_token"].tolist()) == sorted(want)
    assert np.array_equal(d["gt_xy"], np.array([want[t] for t in d["scan_token"].tolist()]))
    assert len(cloud.map_clouds) == 12 and d["full_map"] is not None and d["key_map"] is not None
    for a in agents.values():      # each agent's own gt as well (its step recorded it)
        da = a.result_logger.plot_data(draft=True)
        assert np.array_equal(da["gt_xy"][:, 0], 100.0 * a.system_id + (da["scan_token"] & 0xFFFF))
