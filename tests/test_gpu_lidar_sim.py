"""GPU: the LiDAR simulator's kernels (csrc/lidar_sim.hip) against this project's own restatement (tests/lidar_sim_restated.py).

* against the float32 restatement, which follows the kernels' order of operations: every output bit for bit -- the kept
  records of the cull, range, prim, cos_inc, the emitted frames.  A difference is a finding, not a tolerance;
* against the independent float64 restatement: ids equal and |t - t64| <= 1 mm (one twentieth of the 2 cm range noise of the
  sensors modelled) on every unambiguous ray, at most 1 % of the rays ambiguous (the host test's bounds).

Every observed figure goes to test_logs/lidar_sim_errors.log (scripts/lidar_sim_bench.py --accuracy -> profiles/lidar_sim_accuracy.md).
"""
import numpy as np
import pytest
import torch

import lidar_sim_cases as C
import lidar_sim_restated as RS
from conftest import rot_angle

pytestmark = pytest.mark.gpu
DEV = "cuda"
T_BOUND = 1e-3
AMBIGUOUS_CAP = 0.01


def mods():
    from deeppointmap_amd import augment, lidar_sim, ops
    return lidar_sim, ops, augment


def bits(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.tobytes()


def restated(scene, poses, dirs, model, rays=None):
    prims, kind, ground, _, _ = scene.arrays()
    return RS.simulate32(prims, kind, ground, poses, dirs, model.min_range, model.max_range, rays=rays)


def mismatches(name, got, want):
    """print before asserting: how many entries differ and the largest difference"""
    got, want = got.cpu().numpy() if isinstance(got, torch.Tensor) else got, np.asarray(want)
    bad = got.view(np.int32) != want.view(np.int32) if got.dtype == np.float32 else got != want
    worst = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()) if got.size else 0.0
    C.log(f"kernel vs float32 restatement, {name}: {int(bad.sum())} of {bad.size} entries differ, max difference {worst:.3e}")
    return int(bad.sum())


# ---------------------------------------------------------------------------------------------------------------- float32
@pytest.fixture(scope="module")
def s600():
    scene, poses = C.scene_600()
    want = restated(scene, poses, C.MODEL_385.directions(), C.MODEL_385)
    prims, kind, ground, _, _ = scene.arrays()
    culls = [RS.cull(prims, kind, ground, p, C.MODEL_385.max_range) for p in poses]
    return scene, poses, want, culls


def test_kernels_equal_the_float32_restatement_bit_for_bit(s600):
    LS, ops, _ = mods()
    scene, poses, want, culls = s600
    m = C.MODEL_385
    counts = [len(c[1]) for c in culls]
    assert m.rays == 385 and scene.P == 600 and counts[0] > 2 * 64 and counts[1] > 64 and counts[0] != counts[1] and counts[2] == 0
    sd = scene.to_device(DEV)
    dev_poses = torch.from_numpy(poses).to(DEV)
    kept, plane, status = ops.lidar_cull(sd.prims, sd.kind, sd.ground, dev_poses, m.max_range, scene.P)
    assert status.cpu().tolist() == [[n, 0] for n in counts]
    bad = 0
    for f, (rec, ids, kinds, pl) in enumerate(culls):
        got = kept[f, :counts[f]].cpu().numpy()
        bad += mismatches(f"cull records of frame {f}", got[:, :15], rec)
        assert got[:, 15].view(np.int32).tolist() == (ids | (kinds.astype(np.int64) << 30)).tolist()
        bad += mismatches(f"ground plane of frame {f}", plane[f].cpu().numpy(), pl)
    cast = LS.cast_rays(sd, poses, m)
    bad_prim = mismatches("prim (3 x 385 rays, 600 primitives)", cast[1], want[1])
    bad += mismatches("range", cast[0], want[0]) + mismatches("cos_inc", cast[2], want[2])
    assert bad_prim == 0 and bad == 0
    p = want[1]
    assert (p[2][p[2] >= 0] == scene.P).all() and (p[2] == scene.P).any()       # the far frame sees the ground and nothing else
    assert len(np.unique(p[0])) > 10 and (p[0] == -1).any()


def test_overflow_of_max_kept_is_deferred_to_the_read_back(s600):
    LS, ops, augment = mods()
    scene, poses, _, culls = s600
    most = max(len(c[1]) for c in culls)
    sd = scene.to_device(DEV)
    cast = LS.cast_rays(sd, poses, C.MODEL_385, max_kept=most - 1)          # queued without complaint
    assert cast.status.cpu().tolist() == [[len(c[1]), int(len(c[1]) > most - 1)] for c in culls]
    with pytest.raises(ValueError, match="max_kept"):
        cast.check()
    LS.cast_rays(sd, poses, C.MODEL_385, max_kept=most).check()
    frames = LS.LidarSimulator(sd, C.MODEL_385, max_kept=most - 1).frames(poses)
    with pytest.raises(ValueError, match="max_kept"):
        augment.collate_frames(frames, padding_to=C.MODEL_385.rays)
    frames = LS.LidarSimulator(sd, C.MODEL_385, max_kept=most - 1).frames(poses)
    with pytest.raises(ValueError, match="max_kept"):
        frames[0].nbr_point


# ---------------------------------------------------------------------------------------------------------------- float64
def test_kernels_against_float64_one_kilometre_from_the_origin():
    LS, _, _ = mods()
    scene, poses, m = C.scene_far()
    assert m.rays == 8 * 192 and np.abs(poses[:, :2, 3]).min() > 950
    dirs = m.directions()
    rng, prim, _ = (t.cpu().numpy() for t in LS.cast_rays(scene.to_device(DEV), poses, m))
    worst, n_amb, n = 0.0, 0, 0
    for f, M in enumerate(poses):
        r64, p64, _ = RS.cast64(scene.params, scene.kind, scene.z0, M, dirs, m.min_range, m.max_range)
        amb = RS.ambiguous(scene.params, scene.kind, scene.z0, M, dirs, m.min_range, m.max_range, p64)
        ok = ~amb
        n_amb, n = n_amb + int(amb.sum()), n + len(amb)
        wrong = int((prim[f][ok] != p64[ok]).sum())
        err = float(np.abs(rng[f][ok & (prim[f] == p64)].astype(np.float64) - r64[ok & (prim[f] == p64)]).max())
        C.log(f"kernel vs float64, 1 km from the origin, frame {f}: {len(amb)} rays, {int(amb.sum())} ambiguous, {wrong} ids differ, "
              f"max |t - t64| = {err:.3e} m (bound {T_BOUND:.0e}), {(p64 >= 0).mean():.2f} of the rays return")
        assert wrong == 0 and (p64 >= 0).mean() > 0.3
        worst = max(worst, err)
    assert n_amb <= AMBIGUOUS_CAP * n and worst <= T_BOUND


# ---------------------------------------------------------------------------------------------------------------- rules
@pytest.mark.parametrize("case", C.rule_cases(), ids=lambda c: c.name.replace(" ", "_"))
def test_rule_cases_through_the_kernels(case):
    LS, _, _ = mods()
    m = LS.LidarModel([0.0], 1, case.min_range, case.max_range)
    dirs = torch.from_numpy(case.dirs).to(DEV)
    rng, prim, cos = LS.cast_rays(case.scene.to_device(DEV), case.pose[None], m, dirs=dirs)
    assert prim[0].cpu().tolist() == case.want_prim
    assert rng[0].cpu().tolist() == case.want_range and cos[0].cpu().tolist() == case.want_cos


# ---------------------------------------------------------------------------------------------------------------- emit
def test_emit_equals_the_restatement_and_feeds_collate_without_a_sync(s600):
    LS, ops, augment = mods()
    scene, poses, want, _ = s600
    m = C.MODEL_385.with_(drop_prob=0.3)
    sd = scene.to_device(DEV)
    _, _, _, albedo, class_id = scene.arrays()
    dirs = m.directions()
    g = np.random.default_rng(3)
    noise = (0.02 * g.standard_normal(want[0].shape)).astype(np.float32)
    u = g.random(want[0].shape, dtype=np.float32)
    cast = LS.cast_rays(sd, poses, m)
    for name, kw_np, kw in (("noise and drop", dict(noise=noise, u=u, drop_prob=0.3),
                             dict(noise=torch.from_numpy(noise).to(DEV), u=torch.from_numpy(u).to(DEV))), ("clean", {}, {})):
        frames, intensity, label = LS.emit_frames(*cast, m, poses, scene=sd, **kw)
        for f, pcd in enumerate(frames):
            per_frame = {k: v[f] if isinstance(v, np.ndarray) else v for k, v in kw_np.items()}
            xyz, idx, n, inten, lab = RS.emit(want[0][f], want[1][f], want[2][f], dirs, albedo, class_id, **per_frame)
            assert pcd._host_n is None and pcd.cap == m.rays
            assert int(pcd.count.item()) == n and bits(pcd.xyz) == bits(xyz) and bits(pcd.idx) == bits(idx), (name, f)
            assert bits(intensity[f]) == bits(inten) and bits(label[f]) == bits(lab), (name, f)
            assert np.array_equal(pcd.R.numpy(), poses[f, :3, :3].astype(np.float32))
            assert np.array_equal(pcd.T.numpy(), poses[f, :3, 3:].astype(np.float32))
            if not kw:        # drop_prob = 0, noise = None: every return, t * dir exactly
                hit = want[1][f] >= 0
                assert n == int(hit.sum()) and np.array_equal(xyz[:n], want[0][f][hit, None] * dirs[hit])
    assert 0 < int(frames[1].count.item()) < int(frames[0].count.item()) and int(frames[2].count.item()) > 0
    # the class layer: clean scans equal the functional layer; nothing synchronises until the batch is packed
    sim = LS.LidarSimulator(sd, C.MODEL_385)
    before = augment.host_syncs()
    out = sim.frames(poses)
    assert augment.host_syncs() == before
    pts, R, T, padding, _ = augment.collate_frames(out, padding_to=m.rays)
    assert augment.host_syncs() == before + 1
    assert pts.shape == (3, 3, m.rays) and R.shape == (3, 3, 3) and T.shape == (3, 3, 1)
    for f, pcd in enumerate(frames):
        n = pcd.nbr_point
        assert out[f].nbr_point == n and int((~padding[f]).sum()) == n
        assert bits(pts[f, :, :n].T.contiguous()) == bits(pcd.xyz[:n])


# ---------------------------------------------------------------------------------------------------------------- determinism
def test_three_launches_replay_from_a_graph_and_a_seeded_generator_repeats(s600):
    LS, ops, _ = mods()
    scene, poses, want, _ = s600
    m = C.MODEL_385
    sd = scene.to_device(DEV)
    dirs = torch.from_numpy(m.directions()).to(DEV)
    dev_poses = torch.from_numpy(poses).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    noise = torch.randn(3, m.rays, device=DEV, generator=g) * 0.02
    u = torch.rand(3, m.rays, device=DEV, generator=g)

    def run():
        kept, plane, status = ops.lidar_cull(sd.prims, sd.kind, sd.ground, dev_poses, m.max_range, scene.P)
        cast = ops.lidar_cast(kept, plane, status, scene.P, dirs, m.min_range, m.max_range)
        return cast + ops.lidar_emit(*cast, dirs, sd.albedo, sd.class_id, noise=noise, u=u, drop_prob=0.25)
    eager = [bits(t) for t in run()]
    assert eager[0] == bits(want[0]) and eager[1] == bits(want[1])
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):      # one stream; the host-to-device copies stayed outside
        captured = run()
    for _ in range(2):
        for t in captured:
            t.fill_(0) if t.dtype != torch.float32 else t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert [bits(t) for t in captured] == eager
    a, b = (LS.LidarSimulator(sd, m.with_(drop_prob=0.2), rng=torch.Generator(device=DEV).manual_seed(9)).frames(poses, True)
            for _ in range(2))
    for (fa, ia, la), (fb, ib, lb) in [(a, b)]:
        assert bits(ia) == bits(ib) and bits(la) == bits(lb)
        for x, y in zip(fa, fb):
            assert bits(x.xyz) == bits(y.xyz) and bits(x.idx) == bits(y.idx) and bits(x.count) == bits(y.count)
    clean = LS.LidarSimulator(sd, m).frames(poses)
    assert int(a[0][0].count.item()) < int(clean[0].count.item())           # the drop mask dropped something
    assert bits(a[0][0].xyz) != bits(clean[0].xyz)


# ---------------------------------------------------------------------------------------------------------------- the stack
def test_simulated_frames_register_through_icp():
    """two clean frames of a small street scene 1 m and 2 degrees apart, point-to-plane ICP from identity: the final errors
    against the exact relative pose are below the start errors (the figures go to the accuracy profile; no tighter bound is
    set because none has been measured)"""
    LS, _, augment = mods()
    from deeppointmap_amd import refine
    scene = LS.street_scene(7, blocks=(1, 1))
    m = LS.SMALL16
    assert m.rays == 16 * 512
    first = LS.circuit(scene, 2.0)[4]
    second = first @ C.pose(1.0, 0.0, 0.0, yaw=np.deg2rad(2.0))
    poses = np.stack([first, second])
    frames = LS.LidarSimulator(scene, m, device=DEV).frames(poses)
    pts, _, _, padding, _ = augment.collate_frames(frames, padding_to=m.rays)
    lengths = (~padding).sum(dim=1).to(torch.int32)
    truth = np.linalg.inv(first) @ second                  # frame 1 in frame 0
    one = lambda v: torch.tensor([v], dtype=torch.int32, device=DEV)
    res = refine.icp(pts.contiguous(), lengths, one(1), one(0), torch.eye(4, dtype=torch.float64)[None],
                     schedule=[(3.0, 20), (1.0, 30)], metric=refine.PLANE)
    pose = res.pose[0].cpu().numpy()
    t0, r0 = float(np.linalg.norm(truth[:3, 3])), rot_angle(np.eye(3), truth[:3, :3])
    t1, r1 = float(np.linalg.norm(pose[:3, 3] - truth[:3, 3])), rot_angle(pose[:3, :3], truth[:3, :3])
    C.log(f"ICP on two simulated frames ({lengths.tolist()} points): translation error {t0:.4f} -> {t1:.4f} m, rotation error "
          f"{np.rad2deg(r0):.4f} -> {np.rad2deg(r1):.4f} deg, fitness {float(res.fitness[0]):.3f}, status "
          f"{refine.STATUS_NAMES[int(res.status[0])]}")
    assert t1 < t0 and r1 < r0


# ---------------------------------------------------------------------------------------------------------------- full shape
def test_hdl64e_launch_is_sane_and_equals_the_restatement_on_a_subsample():
    LS, _, _ = mods()
    scene = LS.street_scene(3, blocks=(2, 2))
    m = LS.HDL64E
    poses = LS.circuit(scene, 30.0)[[1, 6]]
    sd = scene.to_device(DEV)
    cast = LS.cast_rays(sd, poses, m)
    frames, intensity, label = LS.emit_frames(*cast, m, poses, scene=sd, status=cast.status, max_kept=cast.max_kept)
    rng, prim, cos = (t.cpu().numpy() for t in cast)
    counts = [f.nbr_point for f in frames]
    assert np.isfinite(rng).all() and np.isfinite(cos).all() and (cos >= 0).all() and (cos <= 1 + 1e-6).all()
    assert all(m.rays // 2 < n <= m.rays for n in counts) and counts == (prim >= 0).sum(axis=1).tolist()
    assert rng[prim >= 0].min() >= m.min_range and rng.max() <= m.max_range
    assert all(torch.isfinite(f.points()).all() for f in frames) and torch.isfinite(intensity).all()
    assert set(np.unique(label.cpu().numpy())) <= {-1, 0, 1, 2, 3, 4}
    rays = np.arange(2048) * 64 + (np.arange(2048) * 37) % 64            # fixed, spread over every beam and column
    want = restated(scene, poses, m.directions(), m, rays=rays)
    bad = mismatches("HDL64E prim on 2 x 2048 sampled rays", prim[:, rays], want[1])
    bad += mismatches("HDL64E range", rng[:, rays], want[0]) + mismatches("HDL64E cos_inc", cos[:, rays], want[2])
    assert bad == 0
