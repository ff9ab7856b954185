"""GPU: the deskew transform (dpm_points_deskew in csrc/deskew.hip, augment.deskew / augment.Deskew) against this project's
float64 restatement (tests/lidar_sweep_restated.py: deskew64) and, end to end, against the exact scene.  The reference has
no counterpart: it assumes compensated scans.

The bound against float64 is 1 mm for points out to 120 m (one twentieth of the 2 cm range noise of the sensors modelled, the
simulator's own bound); the largest error seen goes to test_logs/deskew_errors.log (profiles/deskew_accuracy.md is a copy).
End to end every point of a deskewed clean frame lies within 3 mm of its scene: the 1 mm bounds of the cast, of the deskew
and of the evaluator.
"""
import ctypes

import numpy as np
import pytest
import torch

import lidar_sweep_cases as SC
import lidar_sweep_restated as SW

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 1e-3
A = 512
LOG = "deskew_errors.log"


def mods():
    from deeppointmap_amd import augment, lidar_sim, ops
    return lidar_sim, ops, augment


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def cloud(cap, seed):
    """cap rows out to 120 m (every eighth one beyond 100 m), idx = ray indices of a 16 x 512 sensor in any order"""
    g = np.random.default_rng(seed)
    d = g.standard_normal((cap, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.where(np.arange(cap) % 8 == 0, g.uniform(100.0, 120.0, cap), g.uniform(1.0, 100.0, cap))
    return (d * r[:, None]).astype(np.float32), g.integers(0, 16 * A, cap).astype(np.int32)


def frame(xyz, idx, count):
    from deeppointmap_amd import augment
    return augment.PointCloud.from_buffers(torch.from_numpy(xyz).to(DEV), torch.from_numpy(idx).to(DEV),
                                           torch.tensor([count], dtype=torch.int32, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- float64
@pytest.mark.parametrize("cap", [1, 255, 257, 4097])
def test_deskew_against_float64(cap):
    _, _, augment = mods()
    xyz, idx = cloud(cap, cap)
    worst = 0.0
    for count in sorted({0, cap - 1 - cap // 3}):
        for name, D in SC.MOTIONS.items():
            for s_ref in (0.0, 0.5, 1.0):
                pcd = augment.deskew(frame(xyz.copy(), idx, count), D, time="column", azimuth_steps=A, reference=s_ref)
                got = pcd.xyz.cpu().numpy()
                assert got[count:].tobytes() == xyz[count:].tobytes(), "rows at and past the count keep their bytes"
                assert int(pcd.count.item()) == count and bits(pcd.idx) == idx.tobytes() and pcd.sweep_motion is None
                want = SW.deskew64(xyz[:count], SW.column_fraction(idx[:count], A), D, s_ref)
                err = float(np.abs(got[:count].astype(np.float64) - want).max()) if count else 0.0
                worst = max(worst, err)
                assert err <= BOUND, (name, s_ref, count, err)
                ref = SW.motion64(D, s_ref)            # the frame's pose moves to P(s_ref); it started at the identity
                assert np.abs(pcd.R.numpy() - ref[:3, :3]).max() < 1e-6 and np.abs(pcd.T.numpy() - ref[:3, 3:]).max() < 1e-6
    SC.log(f"deskew vs float64, capacity {cap}, points out to 120 m, motions {list(SC.MOTIONS)}, s_ref 0 / 0.5 / 1: largest "
           f"error {worst:.3e} m (bound {BOUND:.0e})", LOG)


def test_identity_motion_returns_the_input_bytes():
    _, ops, augment = mods()
    xyz, idx = cloud(257, 5)
    xyz[3] = (-0.0, 0.0, -0.0)
    times = torch.rand(16 * A, device=DEV)
    for kw in (dict(time="column", azimuth_steps=A), dict(time="azimuth", azimuth_steps=A), dict(time="azimuth"),
               dict(time="times", times=times)):
        for s_ref in (0.0, 0.5, 1.0):
            pcd = augment.deskew(frame(xyz.copy(), idx, 200), np.eye(4), reference=s_ref, **kw)
            assert bits(pcd.xyz) == xyz.tobytes(), (kw, s_ref)


# ---------------------------------------------------------------------------------------------------------------- time modes
@pytest.fixture(scope="module")
def raw():
    """two clean SMALL16 frames of street_scene(2) with sweep motion, and how to make them again"""
    LS, _, _ = mods()
    scene, P0, P1, m = SC.street_sweep(frames=(7, 20))
    sim = LS.LidarSimulator(scene, m, device=DEV)
    return scene, P0, P1, m, (lambda: sim.frames(P0, poses_end=P1))


def test_column_mode_commutes_with_shuffle_and_voxel_sample(raw):
    _, _, augment = mods()
    scene, P0, P1, m, make = raw
    D = SW.delta64(P0[0], P1[0])
    first = augment.deskew(make()[0], D, time="column", azimuth_steps=m.azimuth_steps, reference=0.5)
    n = first.nbr_point
    row_of = torch.full((m.rays,), -1, dtype=torch.long, device=DEV)
    row_of[first.idx[:n].long()] = torch.arange(n, device=DEV)
    perm = torch.randperm(m.rays, generator=torch.Generator().manual_seed(3))
    for name, move in (("random_shuffle", lambda p: augment.random_shuffle(p, perm[perm < p.nbr_point].to(torch.int32))),
                       ("voxel_sample", lambda p: augment.voxel_sample(p, 0.5, retention="first"))):
        late = augment.deskew(move(make()[0]), D, time="column", azimuth_steps=m.azimuth_steps, reference=0.5)
        k = late.nbr_point
        assert 100 < k <= n and (name == "random_shuffle") == (k == n)
        rows = row_of[late.idx[:k].long()]
        assert (rows >= 0).all() and bits(late.xyz[:k]) == bits(first.xyz[rows]), name


def test_azimuth_mode_and_explicit_times_give_column_mode_bytes_on_a_raw_frame(raw):
    _, _, augment = mods()
    scene, P0, P1, m, make = raw
    D = SW.delta64(P0[1], P1[1])
    A_ = m.azimuth_steps
    column = augment.deskew(make()[1], D, time="column", azimuth_steps=A_, reference=1.0)
    azimuth = augment.deskew(make()[1], D, time="azimuth", azimuth_steps=A_, reference=1.0)
    times = torch.from_numpy((np.arange(m.rays) % A_).astype(np.float32) / np.float32(A_)).to(DEV)
    explicit = augment.deskew(make()[1], D, time="times", times=times, reference=1.0)
    untouched = make()[1]
    assert column.nbr_point > 4000 and bits(column.xyz) != bits(untouched.xyz)
    assert bits(azimuth.xyz) == bits(column.xyz) and bits(explicit.xyz) == bits(column.xyz)
    continuous = augment.deskew(make()[1], D, time="azimuth", reference=1.0)      # no columns given: the azimuth itself
    n = column.nbr_point
    assert float((continuous.xyz[:n] - column.xyz[:n]).abs().max()) < 1e-3
    # explicit times outside the table leave the row as it is
    short = augment.deskew(make()[1], D, time="times", times=times[:A_].contiguous(), reference=1.0)
    beyond = (untouched.idx[:n] >= A_)
    assert beyond.any() and bits(short.xyz[:n][beyond]) == bits(untouched.xyz[:n][beyond])
    assert bits(short.xyz[:n][~beyond]) == bits(column.xyz[:n][~beyond])


def test_bad_arguments_return_the_error_code_and_touch_nothing():
    from deeppointmap_amd import _lib
    _, ops, augment = mods()
    xyz, idx = cloud(64, 9)
    pcd = frame(xyz.copy(), idx, 64)
    D = (ctypes.c_double * 16)(*SC.CORNER.reshape(-1))
    Dp = ctypes.cast(D, ctypes.c_void_p)
    st = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    x, i, c = pcd.xyz.data_ptr(), pcd.idx.data_ptr(), pcd.count.data_ptr()
    for args in ((x, i, c, 64, 3, None, 0, A, Dp, 0.0), (x, i, c, 64, 0, None, 0, 0, Dp, 0.0), (x, None, c, 64, 0, None, 0, A, Dp, 0.0),
                 (x, i, c, 64, 2, None, 0, 0, Dp, 0.0), (x, i, c, 0, 0, None, 0, A, Dp, 0.0), (x, i, c, 64, 0, None, 0, A, None, 0.0),
                 (x, i, c, 64, 0, None, 0, A, Dp, -0.1)):
        assert lib.dpm_points_deskew(*args, st) == -1
    torch.cuda.synchronize()
    assert bits(pcd.xyz) == xyz.tobytes()
    with pytest.raises(ValueError):
        augment.deskew(pcd, SC.CORNER, time="column")
    with pytest.raises(ValueError):
        augment.deskew(pcd, SC.CORNER, time="sometimes", azimuth_steps=A)
    with pytest.raises(ValueError):
        augment.deskew(pcd, SC.CORNER, time="column", azimuth_steps=A, reference=2.0)
    with pytest.raises(ValueError, match="sweep_motion"):
        augment.Deskew("frame", azimuth_steps=A)(pcd)
    assert bits(pcd.xyz) == xyz.tobytes()


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_deskewed_frames_lie_on_their_scene_and_raw_frames_do_not(raw):
    LS, _, augment = mods()
    from deeppointmap_amd import evaluate
    scene, P0, P1, m, make = raw

    def off_the_scene(frames, poses):
        out = []
        for pcd, M in zip(frames, poses):
            p = pcd.points().cpu().numpy().astype(np.float64)
            world = torch.from_numpy(M[:3, :3] @ p.T + M[:3, 3:]).to(DEV)
            out.append(evaluate.scene_distance(world, scene)[0].cpu().numpy())
        return out
    raw_off = off_the_scene(make(), P0)
    for f, d in enumerate(raw_off):
        SC.log(f"end to end, frame {f}: raw under the start pose, {len(d)} points, max {d.max():.3f} m off the scene, "
               f"{100 * float((d > 0.01).mean()):.1f} % beyond 1 cm", LOG)
        assert len(d) > 4000 and (d > 0.01).mean() > 0.10
    for s_ref in (0.0, 0.5, 1.0):
        chain = augment.Compose([augment.Deskew("frame", time="column", azimuth_steps=m.azimuth_steps, reference=s_ref)])
        frames = augment.transform_frames(make(), chain)
        torch.cuda.synchronize()
        poses = [a @ SW.motion64(SW.delta64(a, b), s_ref) for a, b in zip(P0, P1)]
        for f, d in enumerate(off_the_scene(frames, poses)):
            SC.log(f"end to end, frame {f}, Deskew('frame') to s_ref = {s_ref}: max {d.max():.3e} m off the scene (bound 3e-03)", LOG)
            assert d.max() <= 3e-3
            assert np.abs(frames[f].R.numpy() - poses[f][:3, :3]).max() < 1e-6      # the frame's own pose moved along


def test_write_scene_writes_raw_clouds_by_default_and_compensated_ones_on_request(raw, tmp_path):
    LS, _, _ = mods()
    from deeppointmap_amd import evaluate
    scene, P0, P1, m, make = raw
    sim = LS.LidarSimulator(scene, m, device=DEV)
    files = LS.write_scene(tmp_path, "sim", "raw", sim, P0, poses_end=P1)
    fixed = LS.write_scene(tmp_path, "sim", "fixed", sim, P0, poses_end=P1, deskew=0.5)
    frames = make()
    for f in range(2):
        a, b = np.load(files[f]), np.load(fixed[f])
        assert sorted(a.files) == sorted(b.files) == ["ego_rotation", "ego_translation", "lidar_pcd"]
        n = frames[f].nbr_point
        assert a["lidar_pcd"][:, :3].tobytes() == frames[f].xyz[:n].cpu().numpy().tobytes()           # raw, under the start pose
        assert np.array_equal(a["ego_rotation"], P0[f, :3, :3]) and np.array_equal(a["ego_translation"], P0[f, :3, 3:])
        M = P0[f] @ SW.motion64(SW.delta64(P0[f], P1[f]), 0.5)
        assert np.abs(b["ego_rotation"] - M[:3, :3]).max() < 1e-12 and np.abs(b["ego_translation"] - M[:3, 3:]).max() < 1e-12
        assert np.array_equal(a["lidar_pcd"][:, 3], b["lidar_pcd"][:, 3])                              # the same intensities
        world = M[:3, :3] @ b["lidar_pcd"][:, :3].astype(np.float64).T + M[:3, 3:]
        assert float(evaluate.scene_distance(torch.from_numpy(world).to(DEV), scene)[0].max()) <= 3e-3
    with pytest.raises(ValueError, match="poses_end"):
        LS.write_scene(tmp_path, "sim", "bad", sim, P0, deskew=0.5)
