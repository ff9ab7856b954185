"""CPU: the LiDAR simulator's host side (scene, circuit, sensor, dataset writer), the numpy restatement's float32 form against
its independent float64 form, the hand-made rule cases, and the ops wrappers' argument checks.

The float32 bound: |t32 - t64| <= 1 mm on every unambiguous ray = one twentieth of the 2 cm range noise of the sensors that
are modelled; ids equal on every unambiguous ray; at most 1 % of a test's rays may be ambiguous (lidar_sim_restated.ambiguous).
"""
import math
import os
import random
import sys

import numpy as np
import pytest
import torch

import lidar_sim_cases as C
import lidar_sim_restated as RS
from conftest import GOLDEN, load_golden

T_BOUND = 1e-3
AMBIGUOUS_CAP = 0.01


def LS():
    from deeppointmap_amd import lidar_sim
    return lidar_sim


# ---------------------------------------------------------------------------------------------------------------- generators
def test_street_scene_and_circuit_are_stable_and_equal_the_fixture():
    sys.path.insert(0, GOLDEN)
    import make_golden_lidar_sim as G
    a, b, want = G.make(), G.make(), load_golden("lidar_sim_scene.npz")
    assert sorted(a) == sorted(want)
    for k in want:
        assert a[k].dtype == want[k].dtype and a[k].tobytes() == b[k].tobytes(), k
        assert a[k].tobytes() == want[k].tobytes(), k
    assert set(np.unique(a["class_id"])) == {1, 2, 3, 4} and set(np.unique(a["kind"])) == {0, 1}
    other = LS().street_scene(G.SEED + 1, blocks=G.BLOCKS)
    assert other.params.tobytes() != a["params"].tobytes()


def test_circuit_is_closed_level_free_and_evenly_spaced():
    ls = LS()
    scene = ls.street_scene(2, blocks=(2, 2))
    spacing = 2.0
    poses = ls.circuit(scene, spacing)
    F = len(poses)
    step = ls.circuit_length(scene) / F
    assert F == round(ls.circuit_length(scene) / spacing) and abs(step - spacing) <= spacing / F
    xy = poses[:, :3, 3]
    chord = np.linalg.norm(np.roll(xy, -1, axis=0) - xy, axis=1)      # the last pose's successor is the first: closed
    # a chord of an arc of length s at radius r is s (1 - (s / r)^2 / 24 + ...): within 0.5 % for s = 2, r = 6
    assert chord.max() <= step + 1e-9 and chord.min() >= step * (1 - (step / 6.0) ** 2 / 24 - 1e-6)
    R = poses[:, :3, :3]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-14 and np.allclose(np.linalg.det(R), 1.0)
    heading = np.arctan2(R[:, 1, 0], R[:, 0, 0])
    tangent = np.roll(xy, -1, axis=0) - np.roll(xy, 1, axis=0)
    dev = np.angle(np.exp(1j * (heading - np.arctan2(tangent[:, 1], tangent[:, 0]))))
    # heading along the tangent: the central difference is exact on a straight and, by symmetry, inside an arc; where the
    # two join it is off by at most step / (4 r) (half the turn of one step at radius r = 6)
    assert np.abs(dev).max() <= step / (4 * 6.0) and np.median(np.abs(dev)) < 1e-12
    pitch, roll = -np.arcsin(R[:, 2, 0]), np.arctan2(R[:, 2, 1], R[:, 2, 2])
    assert (np.abs(pitch) + np.abs(roll) > 1e-3).all() and np.abs(pitch).max() < 0.03 and np.abs(roll).max() < 0.03
    assert np.allclose(xy[:, 2], ls.SENSOR_HEIGHT)
    two = ls.circuit(scene, spacing, laps=2)
    assert len(two) == 2 * F and np.array_equal(two[:F], poses)
    d = np.linalg.norm(two[F:, :3, 3] - two[:F, :3, 3], axis=1)        # the second lap revisits every place 0.3 m further out
    assert np.allclose(d, 0.3)


def test_lidar_model_directions():
    ls = LS()
    m = ls.HDL64E
    assert (m.beams, m.azimuth_steps, m.rays, m.min_range, m.max_range, m.range_sigma) == (64, 2048, 131072, 0.9, 120.0, 0.02)
    assert m.elevations_deg[0] == 2.0 and abs(m.elevations_deg[-1] + 24.8) < 1e-12
    d = m.directions()
    assert d.dtype == np.float32 and d.shape == (m.rays, 3) and d.flags.c_contiguous
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-7
    r = 17 * m.azimuth_steps + 512                                      # ray = beam * steps + column; column 512 looks along +y
    e = math.radians(m.elevations_deg[17])
    assert np.allclose(d[r], [0.0, math.cos(e), math.sin(e)], atol=1e-7)
    assert ls.SMALL16.rays == 16 * 512
    with pytest.raises(ValueError):
        ls.LidarModel([0.0], 8, 2.0, 1.0)


# ---------------------------------------------------------------------------------------------------------------- float32 vs float64
def _compare(name, scene, poses, model):
    prims, kind, ground, _, _ = scene.arrays()
    dirs = model.directions()
    r32, p32, _ = RS.simulate32(prims, kind, ground, poses, dirs, model.min_range, model.max_range)
    worst, n_amb, n = 0.0, 0, 0
    for f, M in enumerate(poses):
        r64, p64, _ = RS.cast64(scene.params, scene.kind, scene.z0, M, dirs, model.min_range, model.max_range)
        amb = RS.ambiguous(scene.params, scene.kind, scene.z0, M, dirs, model.min_range, model.max_range, p64)
        ok = ~amb
        n_amb, n = n_amb + int(amb.sum()), n + len(amb)
        assert np.array_equal(p32[f][ok], p64[ok]), (name, f, int((p32[f][ok] != p64[ok]).sum()))
        worst = max(worst, float(np.abs(r32[f][ok].astype(np.float64) - r64[ok]).max()))
        assert (p64 >= 0).mean() > 0.3, "the scene returns too little to mean anything"
    C.log(f"restated float32 vs float64, {name}: {n} rays, {n_amb} ambiguous, max |t32 - t64| = {worst:.3e} m (bound {T_BOUND:.0e})")
    assert n_amb <= AMBIGUOUS_CAP * n
    assert worst <= T_BOUND


def test_float32_against_float64_random_scene():
    scene = C.random_scene(21, 500, 45.0)
    model = LS().LidarModel(np.linspace(10.0, -24.0, 16), 256, 0.9, 120.0)
    poses = np.stack([C.free_pose(scene, 0.0, 0.0, 1.8, yaw=0.3, pitch=0.04, roll=-0.03),
                      C.free_pose(scene, 120.0, 30.0, 2.0, yaw=3.0, pitch=-0.05, roll=0.02)])     # looks at it from 75 m off
    _compare("random scene of 500", scene, poses, model)


def test_float32_against_float64_street_scene_far_from_the_origin():
    ls = LS()
    scene = ls.street_scene(4, blocks=(3, 3), z0=0.0)
    poses = ls.circuit(scene, 25.0)[[0, 3, 7]]
    _compare("street scene 3 x 3, 120 m range", scene, poses, ls.LidarModel(np.linspace(2.0, -24.8, 16), 256, 0.9, 120.0))


# ---------------------------------------------------------------------------------------------------------------- rules
@pytest.mark.parametrize("case", C.rule_cases(), ids=lambda c: c.name.replace(" ", "_"))
def test_rule_cases_in_both_restatements(case):
    s = case.scene
    prims, kind, ground, _, _ = s.arrays()
    r32, p32, c32 = RS.simulate32(prims, kind, ground, case.pose[None], case.dirs, case.min_range, case.max_range)
    r64, p64, c64 = RS.cast64(s.params, s.kind, s.z0, case.pose, case.dirs, case.min_range, case.max_range)
    assert p32[0].tolist() == case.want_prim and p64.tolist() == case.want_prim
    assert r32[0].tolist() == case.want_range and r64.tolist() == case.want_range      # exact: the numbers are dyadic
    assert c32[0].tolist() == case.want_cos and c64.tolist() == case.want_cos


def test_emit_restatement_orders_and_fills():
    dirs = LS().LidarModel([0.0, -10.0], 4, 0.5, 50.0).directions()
    rng = np.array([2, 0, 3, 4, 0, 5, 6, 7], np.float32)
    prim = np.array([0, -1, 2, 1, -1, 0, 2, 1], np.int32)
    cos = np.full(8, 0.5, np.float32)
    u = np.array([0.9, 0.9, 0.1, 0.9, 0.9, 0.2, 0.9, 0.9], np.float32)
    albedo, cls = np.array([0.5, 1.0, 0.25], np.float32), np.array([1, 2, 0], np.int32)
    xyz, idx, n, inten, label = RS.emit(rng, prim, cos, dirs, albedo, cls, u=u, drop_prob=0.2)
    assert n == 5 and idx[:5].tolist() == [0, 3, 5, 6, 7] and not xyz[5:].any() and not idx[5:].any()   # u = 0.2 stays: u >= p
    assert np.array_equal(xyz[:5], rng[[0, 3, 5, 6, 7], None] * dirs[[0, 3, 5, 6, 7]])
    assert inten.tolist() == [0.25, 0, 0.125, 0.5, 0, 0.25, 0.125, 0.5] and label.tolist() == [1, -1, 0, 2, -1, 1, 0, 2]


# ---------------------------------------------------------------------------------------------------------------- writer
@pytest.mark.parametrize("fmt", ["npz", "bin"])
def test_write_scene_round_trip(tmp_path, fmt):
    from deeppointmap_amd import dataset, refine
    from deeppointmap_amd.config import Cfg
    ls = LS()
    scene = ls.street_scene(1, blocks=(1, 1))
    poses = ls.circuit(scene, 6.0, laps=1)
    F = len(poses)
    rng = np.random.default_rng(0)
    scans = [rng.standard_normal((20 + k, 4)).astype(np.float32) for k in range(F)]
    files = ls.write_scene(tmp_path, "SimCity", "00", scans, poses, agents=[F - 5, 5], fmt=fmt, refined_distance=15.0)
    assert [os.path.relpath(f, tmp_path) for f in files[:1] + files[-1:]] == \
        [os.path.join("SimCity", "00", "0", f"0.{fmt}"), os.path.join("SimCity", "00", "1", f"{F - 1}.{fmt}")]
    cfg = Cfg(ls.tree_config(tmp_path, {"SimCity": ["00"]}, fmt=fmt, distance=15.0))
    ds = dataset.SlamDatasets(cfg)
    assert len(ds) == F and ds.dataset_list[0].scene_list[0].pcd_range.tolist() == [0, F - 5, F]
    for k in range(F):
        assert ds.dataset_list[0].file_of(k) == files[k]
        rows, stride, R, T, _ = ds.dataset_list[0].read_raw(k)
        assert stride == 4 and rows.tobytes() == scans[k].tobytes()
        if fmt == "npz":
            assert R.dtype == np.float64 and np.array_equal(R, poses[k, :3, :3]) and np.array_equal(T, poses[k, :3, 3:])
    if fmt == "bin":
        assert np.array_equal(np.loadtxt(tmp_path / "SimCity" / "00" / "poses.txt").reshape(F, 3, 4), poses[:, :3, :])
    d = np.linalg.norm(poses[:, None, :3, 3].astype(np.float32) - poses[None, :, :3, 3].astype(np.float32), axis=-1)
    assert np.array_equal(ds.frame_distance[0][0].numpy(), d.astype(np.float16))
    table = refine.read_refined_table(tmp_path / "SimCity" / "00" / "refined_SE3.pkl")
    pairs = refine.candidate_pairs(poses[:, :3, 3], 15.0)
    assert sorted(table) == [tuple(p) for p in pairs.tolist()] and len(table) > F
    for (i, j), M in table.items():
        assert M.dtype == np.float64 and np.abs(M - np.linalg.inv(poses[i]) @ poses[j]).max() < 1e-12
    ds.registration()
    plan = ds.plan_registration(3, rng=random.Random(1))
    assert plan["frames"][0][3] == files[3] and len(plan["frames"]) == plan["S"] * plan["num_map"]
    assert all(f == str(tmp_path / "SimCity" / "00" / "refined_SE3.pkl") for f in plan["info"]["refined_SE3_file"])
    anchor = plan["info"]["dsf_index"][0][2]                             # every frame drawn for the first map has an exact entry
    for _, _, other in plan["info"]["dsf_index"][1:plan["S"]]:
        assert other != anchor and (min(anchor, other), max(anchor, other)) in table


def test_write_scene_refuses_bad_arguments(tmp_path):
    ls = LS()
    poses = np.tile(np.eye(4), (3, 1, 1))
    scans = [np.zeros((2, 4), np.float32)] * 3
    with pytest.raises(ValueError):
        ls.write_scene(tmp_path, "A", "00", scans, poses, fmt="pcd")
    with pytest.raises(ValueError):
        ls.write_scene(tmp_path, "A", "00", scans[:2], poses)
    with pytest.raises(ValueError):
        ls.write_scene(tmp_path, "A", "00", scans, poses, agents=[2, 2])
    with pytest.raises(ValueError):
        ls.write_scene(tmp_path, "A", "00", [np.zeros((2, 3), np.float32)] * 3, poses)
    assert len(ls.write_scene(tmp_path, "A", "00", scans, poses, agents=3)) == 3
    assert sorted(os.listdir(tmp_path / "A" / "00")) == ["0", "1", "2"]


# ---------------------------------------------------------------------------------------------------------------- wrappers
def test_entry_points_are_declared_and_built():
    from deeppointmap_amd import _lib
    from deeppointmap_amd.csrc import build
    assert "lidar_sim.hip" in build.SOURCES
    for name in ("dpm_lidar_cull", "dpm_lidar_cast", "dpm_lidar_emit"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    # the host-side refusals of the C entry points themselves need no GPU
    lib = _lib.load()
    assert lib.dpm_lidar_cull(None, None, 1, None, None, 1, 10.0, 1, None, None, None, None) == -1
    assert lib.dpm_lidar_cast(None, None, None, 1, 0, None, 1, 1, 0.0, 1.0, None, None, None, None) == -1
    assert lib.dpm_lidar_emit(None, None, None, None, 1, 1, None, None, 0.0, None, None, 0, None, None, None, None, None, None) == -1


def test_ops_wrappers_refuse_cpu_tensors_wrong_dtypes_and_wrong_shapes():
    from deeppointmap_amd import _lib, ops
    f64, f32_, i32 = torch.float64, torch.float32, torch.int32
    z = lambda *s, dtype=f32_: torch.zeros(*s, dtype=dtype)
    scene = (z(3, 10, dtype=f64), z(3, dtype=i32), z(2, dtype=f64))
    with pytest.raises(_lib.DpmError, match="no CPU fallback"):
        ops.lidar_cull(*scene, z(2, 4, 4, dtype=f64), 50.0, 8)
    with pytest.raises(TypeError):
        ops.lidar_cull(scene[0].float(), scene[1], scene[2], z(2, 4, 4, dtype=f64), 50.0, 8)
    with pytest.raises(TypeError):
        ops.lidar_cull(*scene, z(2, 4, 4), 50.0, 8)
    with pytest.raises(ValueError):
        ops.lidar_cull(z(3, 9, dtype=f64), scene[1], scene[2], z(2, 4, 4, dtype=f64), 50.0, 8)
    with pytest.raises(ValueError):
        ops.lidar_cull(scene[0], z(4, dtype=i32), scene[2], z(2, 4, 4, dtype=f64), 50.0, 8)
    with pytest.raises(ValueError):
        ops.lidar_cull(*scene, z(2, 3, 4, dtype=f64), 50.0, 8)
    with pytest.raises(ValueError):
        ops.lidar_cull(*scene, z(2, 4, 4, dtype=f64), 50.0, 0)
    cull = (z(2, 8, 16), z(2, 4), z(2, 2, dtype=i32))
    with pytest.raises(_lib.DpmError):
        ops.lidar_cast(*cull, 3, z(7, 3), 0.5, 50.0)
    with pytest.raises(TypeError):
        ops.lidar_cast(cull[0], cull[1], cull[2].long(), 3, z(7, 3), 0.5, 50.0)
    with pytest.raises(ValueError):
        ops.lidar_cast(z(2, 8, 15), cull[1], cull[2], 3, z(7, 3), 0.5, 50.0)
    with pytest.raises(ValueError):
        ops.lidar_cast(cull[0], z(3, 4), cull[2], 3, z(7, 3), 0.5, 50.0)
    with pytest.raises(ValueError):
        ops.lidar_cast(*cull, 3, z(7, 4), 0.5, 50.0)
    with pytest.raises(ValueError):
        ops.lidar_cast(*cull, 3, z(7, 3), 5.0, 5.0)
    cast = (z(2, 7), z(2, 7, dtype=i32), z(2, 7), z(7, 3), z(4), z(4, dtype=i32))
    with pytest.raises(_lib.DpmError):
        ops.lidar_emit(*cast)
    with pytest.raises(TypeError):
        ops.lidar_emit(cast[0], cast[1].float(), *cast[2:])
    with pytest.raises(TypeError):
        ops.lidar_emit(*cast, noise=z(2, 7, dtype=f64))
    with pytest.raises(ValueError):
        ops.lidar_emit(*cast, u=z(2, 8))
    with pytest.raises(ValueError):
        ops.lidar_emit(*cast[:3], z(8, 3), *cast[4:])
    with pytest.raises(ValueError):
        ops.lidar_emit(*cast[:5], z(5, dtype=i32))
    with pytest.raises(ValueError):
        ops.lidar_emit(*cast, drop_prob=1.5)
