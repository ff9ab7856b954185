"""CPU: the trajectory metrics of deeppointmap_amd/evaluate.py on constructed trajectories with known answers, the map
restatement's float32 form against its independent float64 form and against hand-made cases, ResultLogger.evaluate without
a map, and the argument refusals of the three C entry points (before any HIP call: they need no GPU).

The float32 bound is the simulator's: |dist32 - dist64| <= 1 mm; ids equal wherever the two nearest surfaces are more than
2 mm apart in float64; at most 1 % of a test's points may be excluded that way.
"""
import json
import math

import numpy as np
import pytest
import torch

import map_eval_cases as C
import map_eval_restated as RS


def EV():
    from deeppointmap_amd import evaluate
    return evaluate


# ---------------------------------------------------------------------------------------------------------------- helpers
def rigid(rng, angle=None, trans=10.0):
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(-math.pi, math.pi) if angle is None else angle
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * K @ K
    T[:3, 3] = rng.uniform(-trans, trans, 3)
    return T


def random_trajectory(rng, n=60):
    out, T = [], np.eye(4)
    for _ in range(n):
        T = T @ rigid(rng, angle=rng.uniform(-0.1, 0.1), trans=1.5)
        out.append(T)
    return np.stack(out)


def yaw_step(length, yaw=0.0):
    T = np.eye(4)
    c, s = math.cos(yaw), math.sin(yaw)
    T[:2, :2], T[0, 3] = [[c, -s], [s, c]], length
    return T


def chain(steps):
    out, T = [np.eye(4)], np.eye(4)
    for S in steps:
        T = T @ S
        out.append(T)
    return np.stack(out)


# ---------------------------------------------------------------------------------------------------------------- ATE
def test_ate_is_zero_for_a_rigidly_moved_copy_and_invariant_under_rigid_moves():
    ev, rng = EV(), np.random.default_rng(1)
    gt = random_trajectory(rng)
    a = ev.ate(rigid(rng) @ gt, gt)
    assert a["rmse"] <= 1e-9 and a["max"] <= 1e-9 and a["rot_max"] <= 1e-9 and a["n"] == len(gt)
    est = gt.copy()
    est[:, :3, 3] += 0.2 * rng.standard_normal((len(gt), 3))
    base = ev.ate(est, gt)
    assert 0.05 < base["rmse"] < 0.5
    for _ in range(3):
        moved = ev.ate(rigid(rng) @ est, gt)
        for k in ("rmse", "mean", "median", "max", "rot_mean", "rot_max"):
            assert abs(moved[k] - base[k]) <= 1e-9, k
    # without alignment the move shows
    assert ev.ate(rigid(rng) @ est, gt, mode="none")["rmse"] > 1.0
    # "first" makes the first pose exact
    M = rigid(rng)
    assert np.abs(ev.align_trajectory(M @ gt, gt, "first") @ (M @ gt) - gt).max() <= 1e-9


def test_ate_of_a_hand_made_residual_pattern():
    """positions on the corners of a square in the plane z = 0, residuals +-e along z with alternating signs: mean and
    cross-covariance are unchanged by them, so the least-squares fit is the identity and every error is exactly e"""
    ev = EV()
    e = 0.125
    gt = np.tile(np.eye(4), (8, 1, 1))
    gt[:, :3, 3] = [(x, y, 0.0) for x, y in ((1, 1), (-1, -1), (1, -1), (-1, 1), (2, 2), (-2, -2), (2, -2), (-2, 2))]
    est = gt.copy()
    est[:, 2, 3] = [e, e, -e, -e, e, e, -e, -e]
    assert np.abs(ev.align_trajectory(est, gt, "se3") - np.eye(4)).max() <= 1e-12
    a = ev.ate(est, gt)
    for k in ("rmse", "mean", "median", "max"):
        assert abs(a[k] - e) <= 1e-12, (k, a[k])
    assert a["rot_max"] <= 1e-12
    # one outlier: rmse, mean, median and max come apart as computed by hand (no alignment)
    est2 = gt.copy()
    est2[0, 0, 3] += 0.8
    a = ev.ate(est2, gt, mode="none")
    assert abs(a["rmse"] - 0.8 / math.sqrt(8)) <= 1e-12 and abs(a["mean"] - 0.1) <= 1e-12 and a["median"] == 0.0 and abs(a["max"] - 0.8) <= 1e-12
    # a reflection would fit mirrored positions better: the guard keeps a rotation
    mirrored = gt.copy()
    mirrored[:, 0, 3] *= -1
    mirrored[:4, 2, 3] += 0.01          # off the plane, so that the mirror image is no rotation of it
    S = ev.align_trajectory(mirrored, gt, "se3")
    assert abs(np.linalg.det(S[:3, :3]) - 1.0) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------- RPE
def test_rpe_of_a_constant_extra_step():
    ev = EV()
    d = np.array([0.03, -0.04, 0.12])                      # |d| = 0.13
    extra = np.eye(4)
    extra[:3, 3] = d
    gt = chain([yaw_step(1.0)] * 40)
    est = chain([yaw_step(1.0) @ extra] * 40)
    r = ev.rpe(est, gt, 1)
    for k in ("trans_rmse", "trans_mean", "trans_max"):
        assert abs(r[k] - 0.13) <= 1e-12, k
    assert r["rot_max"] <= 1e-12 and r["n"] == 40
    z = ev.rpe(gt, gt, 3)
    assert z["trans_max"] <= 1e-12 and z["n"] == 38
    assert ev.rpe(gt[:2], gt[:2], 5) is None


# ---------------------------------------------------------------------------------------------------------------- KITTI
def test_kitti_scaled_steps_give_the_scale_error_at_every_length():
    ev = EV()
    s = 1.04
    gt = chain([yaw_step(1.0)] * 450)
    est = chain([yaw_step(s)] * 450)
    k = ev.kitti_odometry_error(est, gt, lengths=(100, 200, 300, 400, 500, 600, 700, 800), step=10)
    assert [r["length"] for r in k["per_length"]] == [100.0, 200.0, 300.0, 400.0]       # 450 m of path: the rest is skipped
    for r in k["per_length"]:
        assert abs(r["t_err"] - (s - 1)) <= 1e-9 and r["r_err"] <= 1e-12
    assert [r["n"] for r in k["per_length"]] == [36, 26, 16, 6] and k["segments"] == 84
    assert abs(k["t_err"] - (s - 1)) <= 1e-9
    short = ev.kitti_odometry_error(chain([yaw_step(0.9)] * 450), gt)
    assert abs(short["t_err"] - 0.1) <= 1e-9
    assert ev.kitti_odometry_error(est[:50], gt[:50]) is None                           # 49 m: every length skipped


def test_kitti_constant_yaw_drift_gives_the_drift_per_metre():
    ev = EV()
    w = 2e-4                                               # rad per metre; 400 m of it stays far below pi
    gt = chain([yaw_step(1.0)] * 420)
    est = chain([yaw_step(1.0, yaw=w)] * 420)
    k = ev.kitti_odometry_error(est, gt, lengths=(100, 200, 400), step=10)
    assert len(k["per_length"]) == 3
    for r in k["per_length"]:
        assert abs(r["r_err"] - w) <= 1e-12, r
        assert r["t_err"] > 0
    assert abs(k["r_err"] - w) <= 1e-12


def test_trajectory_file_round_trip_and_command_line(tmp_path, capsys):
    from deeppointmap_amd.consumer import Rank0Consumer
    from deeppointmap_amd.system import ResultLogger
    ev, rng = EV(), np.random.default_rng(3)
    gt = random_trajectory(rng, 12)
    b = Rank0Consumer(None, "cpu")
    for i, T in enumerate(gt):
        b.type[i], b.poses[i] = "full", torch.from_numpy(T)
    ResultLogger(b, str(tmp_path)).save_trajectory("t")
    back = ev.load_kitti_trajectory(tmp_path / "t.allframes.txt")
    assert back.shape == (12, 4, 4) and np.abs(back - gt).max() <= 1e-9
    assert ev.main([str(tmp_path / "t.allframes.txt"), str(tmp_path / "t.keyframes.txt")]) == 0
    out = json.loads(capsys.readouterr().out)
    assert out["n"] == 12 and out["ate"]["rmse"] <= 1e-9 and out["rpe"]["trans_max"] <= 1e-9 and out["kitti"] is None


# ---------------------------------------------------------------------------------------------------------------- ResultLogger
def test_result_logger_evaluate_without_maps_writes_the_trajectory_section(tmp_path):
    from deeppointmap_amd.consumer import Rank0Consumer
    from deeppointmap_amd.system import ResultLogger
    ev = EV()
    b = Rank0Consumer(None, "cpu")                         # no result_maps: no clouds are retained
    for tok, kind in [(0, "full"), (2, "non-keyframe"), (1, "full"), (3, "full")]:
        b.type[tok] = kind
        b.poses[tok] = torch.eye(4)
        b.poses[tok][:3, 3] = torch.tensor([float(tok), 0.25 * tok * tok, 0.0])
    for tok in (0, 1, 2):                                  # scan 3 has no ground truth: it is left out
        b.gt[tok] = torch.eye(4)
        b.gt[tok][:3, 3] = torch.tensor([float(tok), 0.0, 0.0])
    rl = ResultLogger(b, str(tmp_path))
    out = rl.evaluate("m")
    assert out["map_to_map"] is None and out["map_accuracy"] is None and out["scans"] == 4
    est = np.stack([b.poses[t].double().numpy() for t in (0, 1, 2)])
    gt = np.stack([b.gt[t].double().numpy() for t in (0, 1, 2)])
    assert out["trajectory"] == ev.trajectory_metrics(est, gt) and out["trajectory"]["n"] == 3
    assert out["trajectory"]["ate"]["rmse"] > 0 and out["trajectory"]["kitti"] is None
    assert json.load(open(tmp_path / "m.json")) == json.loads(json.dumps(out))
    # no ground truth at all: no trajectory section either, and still no error
    b.gt.clear()
    assert rl.evaluate("n")["trajectory"] is None and json.load(open(tmp_path / "n.json"))["trajectory"] is None
    assert ResultLogger(b, None).evaluate()["scans"] == 4


# ---------------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("case", C.rule_cases(), ids=lambda c: c.name.replace(" ", "_").replace(",", "").replace(":", ""))
@pytest.mark.parametrize("origin", [(0.0, 0.0, 0.0), (2.0, -4.0, 1.0)], ids=["origin0", "dyadic_origin"])
def test_rule_cases_in_both_restatements(case, origin):
    s = case.scene
    rec = RS.records(s.params, s.kind, origin)
    d32, s32 = RS.scene_distance32(case.points, rec, None if s.z0 is None else s.z0 - origin[2], origin)
    assert d32.tolist() == case.want_dist and s32.tolist() == case.want_surf            # exact: the numbers are dyadic
    ok = np.isfinite(case.points).all(axis=0)
    d64, s64, _ = RS.scene_distance64(s.params, s.kind, s.z0, case.points[:, ok].astype(np.float64))
    want = np.asarray(case.want_dist)[ok]
    if np.isfinite(want).all():
        assert np.abs(d64 - want).max() <= 1e-12
        # a tie in float64 goes to the first row as well (argmin), the ground being the last row
        assert s64.tolist() == np.asarray(case.want_surf)[ok].tolist()
    else:
        assert np.isinf(d64).all() and (s64 == -1).all()


def test_records_equal_the_modules():
    ev = EV()
    scene = C.mixed_scene(65)
    origin = [1.25, -3.5, 2.0]
    assert ev.scene_records(scene, origin).tobytes() == RS.records(scene.params, scene.kind, origin).tobytes()
    assert ev.scene_records(C.mixed_scene(0), origin).shape == (0, 12)


def _float32_against_float64(name, scene, pts, cap=C.EXCLUDED_CAP):
    origin = C.bbox_centre(pts)
    rec = RS.records(scene.params, scene.kind, origin)
    d32, s32 = RS.scene_distance32(pts, rec, None if scene.z0 is None else scene.z0 - origin[2], origin)
    d64, s64, gap = RS.scene_distance64(scene.params, scene.kind, scene.z0, pts.astype(np.float64))
    err = float(np.abs(d32.astype(np.float64) - d64).max())
    clear = gap > C.GAP
    share = 1.0 - clear.mean()
    C.log(f"restated float32 vs float64, {name}: {pts.shape[1]} points, max |d32 - d64| = {err:.3e} m (bound {C.DIST_BOUND:.0e}), "
          f"{int((~clear).sum())} points ({100 * share:.3f} %) under the {C.GAP * 1e3:.0f} mm gap, "
          f"{int((s32 != s64)[clear].sum())} ids differ outside it")
    assert err <= C.DIST_BOUND
    assert cap is None or share <= cap
    assert np.array_equal(s32[clear], s64[clear])


def test_float32_against_float64_one_kilometre_from_the_origin():
    scene, pts = C.far_cloud()
    assert pts.shape[1] > 5000
    _float32_against_float64("scene_far, SMALL16, 2 cm noise", scene, pts)


def test_float32_against_float64_mixed_scene():
    """the scene of the bit-for-bit GPU test.  No cap on the excluded share here: its boxes stand ON the ground and its
    random points reach a metre below it, so every point under a box is an exact tie between floor and ground by construction"""
    scene = C.mixed_scene(130)
    _float32_against_float64("mixed scene of 130, random points", scene, C.mixed_points(scene, 1000)[:, :900], cap=None)


def test_statistics_restatement_on_a_hand_made_array():
    d = np.array([0.0, 0.5, 1.0, 2.0, np.inf, 0.25, np.nan], np.float32)
    surf = np.array([0, 1, 2, 0, 1, -1, 2], np.int32)
    cls = np.array([0, 1, 1], np.int32)
    t = RS.stats(d, [0.25, 1.0], 1.0, surf, cls, C=2)
    assert t[2].tolist() == [4, 3, 1.75, 1.3125, 1.0, 2, 4]                                # total: 0, .5, 1, .25 matched
    assert t[0].tolist() == [1, 1, 0.0, 0.0, 0.0, 1, 1] and t[1].tolist() == [2, 2, 1.5, 1.25, 1.0, 0, 2]
    row = EV().stats_row(t[2], [0.25, 1.0])
    assert row["n"] == 7 and row["matched"] == 4 and row["mean"] == 0.4375 and row["max"] == 1.0
    assert row["within"] == {"0.25": 2 / 7, "1": 4 / 7} and row["unmatched_share"] == 3 / 7
    assert EV().stats_row([0, 0, 0, 0, 0], [])["mean"] is None


# ---------------------------------------------------------------------------------------------------------------- wrappers
def test_entry_points_are_declared_built_and_refuse_bad_arguments_without_a_gpu():
    import ctypes
    from deeppointmap_amd import _lib
    from deeppointmap_amd.csrc import build
    assert "map_eval.hip" in build.SOURCES
    lib = _lib.load()
    for name in ("dpm_scene_distance", "dpm_cloud_nn", "dpm_cloud_nn_workspace_bytes", "dpm_distance_stats",
                 "dpm_distance_stats_workspace_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    x = 4096            # any non-NULL address: a refused call touches none of them
    thr = (ctypes.c_float * 9)(*([0.1] * 9))
    tp = ctypes.addressof(thr)
    # scene distance: negative sizes, a NULL output, records missing
    assert lib.dpm_scene_distance(x, -1, x, 1, 0.0, 1, 0.0, 0.0, 0.0, x, x, None) == -1
    assert lib.dpm_scene_distance(x, 8, x, -1, 0.0, 1, 0.0, 0.0, 0.0, x, x, None) == -1
    assert lib.dpm_scene_distance(x, 8, x, 1, 0.0, 1, 0.0, 0.0, 0.0, None, x, None) == -1
    assert lib.dpm_scene_distance(x, 8, x, 1, 0.0, 1, 0.0, 0.0, 0.0, x, None, None) == -1
    assert lib.dpm_scene_distance(x, 8, None, 1, 0.0, 1, 0.0, 0.0, 0.0, x, x, None) == -1
    assert lib.dpm_scene_distance(None, 8, x, 1, 0.0, 1, 0.0, 0.0, 0.0, x, x, None) == -1
    # neighbour search: negative sizes, a NULL output, no workspace, max_dist <= 0
    assert lib.dpm_cloud_nn(x, -1, x, 4, 0.5, 0.0, 0.0, 0.0, x, x, x, None) == -1
    assert lib.dpm_cloud_nn(x, 4, x, -1, 0.5, 0.0, 0.0, 0.0, x, x, x, None) == -1
    assert lib.dpm_cloud_nn(x, 4, x, 4, 0.5, 0.0, 0.0, 0.0, None, x, x, None) == -1
    assert lib.dpm_cloud_nn(x, 4, x, 4, 0.5, 0.0, 0.0, 0.0, x, None, x, None) == -1
    assert lib.dpm_cloud_nn(x, 4, x, 4, 0.5, 0.0, 0.0, 0.0, x, x, None, None) == -1
    assert lib.dpm_cloud_nn(x, 4, x, 4, 0.0, 0.0, 0.0, 0.0, x, x, x, None) == -1
    assert lib.dpm_cloud_nn(x, 4, x, 4, -1.0, 0.0, 0.0, 0.0, x, x, x, None) == -1
    assert lib.dpm_cloud_nn(x, 4, x, 4, float("nan"), 0.0, 0.0, 0.0, x, x, x, None) == -1
    assert lib.dpm_cloud_nn_workspace_bytes(-1, 4) == 0 and lib.dpm_cloud_nn_workspace_bytes(4, -1) == 0
    assert lib.dpm_cloud_nn_workspace_bytes(1, 0) > 0
    assert lib.dpm_cloud_nn_workspace_bytes(1, 1000) - lib.dpm_cloud_nn_workspace_bytes(1, 0) == 16000
    # statistics: T > 8, negative sizes, a NULL output, max_dist <= 0, classes without surf
    assert lib.dpm_distance_stats(x, 8, None, None, 0, 0, tp, 9, 1.0, x, x, None) == -1
    assert lib.dpm_distance_stats(x, -1, None, None, 0, 0, tp, 2, 1.0, x, x, None) == -1
    assert lib.dpm_distance_stats(x, 8, None, None, 0, 0, tp, -1, 1.0, x, x, None) == -1
    assert lib.dpm_distance_stats(x, 8, None, None, 0, -1, tp, 2, 1.0, x, x, None) == -1
    assert lib.dpm_distance_stats(x, 8, None, None, 0, 0, tp, 2, 1.0, None, x, None) == -1
    assert lib.dpm_distance_stats(x, 8, None, None, 0, 0, tp, 2, 1.0, x, None, None) == -1
    assert lib.dpm_distance_stats(x, 8, None, None, 0, 0, tp, 2, 0.0, x, x, None) == -1
    assert lib.dpm_distance_stats(x, 8, None, None, 0, 0, tp, 2, -2.0, x, x, None) == -1
    assert lib.dpm_distance_stats(x, 8, None, x, 3, 2, tp, 2, 1.0, x, x, None) == -1
    assert lib.dpm_distance_stats(x, 8, x, x, 3, 2, None, 2, 1.0, x, x, None) == -1
    assert lib.dpm_distance_stats_workspace_bytes(8, 0, 9) == 0 and lib.dpm_distance_stats_workspace_bytes(-1, 0, 1) == 0
    assert lib.dpm_distance_stats_workspace_bytes(4097, 5, 8) - lib.dpm_distance_stats_workspace_bytes(4096, 5, 8) == 8 * 6 * 13


def test_ops_wrappers_refuse_cpu_tensors_wrong_dtypes_and_wrong_shapes():
    from deeppointmap_amd import _lib, ops
    f32_, i32 = torch.float32, torch.int32
    z = lambda *s, dtype=f32_: torch.zeros(*s, dtype=dtype)
    o = (0.0, 0.0, 0.0)
    with pytest.raises(_lib.DpmError, match="no CPU fallback"):
        ops.scene_distance(z(3, 8), z(2, 12), 0.0, o)
    with pytest.raises(TypeError):
        ops.scene_distance(z(3, 8, dtype=torch.float64), z(2, 12), 0.0, o)
    with pytest.raises(ValueError):
        ops.scene_distance(z(8, 3), z(2, 12), 0.0, o)
    with pytest.raises(ValueError):
        ops.scene_distance(z(3, 8), z(2, 16), 0.0, o)
    with pytest.raises(ValueError):
        ops.scene_distance(z(3, 8), z(2, 12), 0.0, (0.0, 0.0))
    with pytest.raises(_lib.DpmError):
        ops.cloud_nn(z(3, 8), z(3, 9), 0.5, o)
    with pytest.raises(ValueError):
        ops.cloud_nn(z(3, 8), z(3, 9), 0.0, o)
    with pytest.raises(ValueError):
        ops.cloud_nn(z(3, 8), z(4, 9), 0.5, o)
    with pytest.raises(TypeError):
        ops.cloud_nn(z(3, 8), z(3, 9, dtype=torch.float64), 0.5, o)
    with pytest.raises(_lib.DpmError):
        ops.distance_stats(z(8), [0.1], 1.0)
    with pytest.raises(ValueError):
        ops.distance_stats(z(8), [0.1] * 9, 1.0)
    with pytest.raises(ValueError):
        ops.distance_stats(z(8), [0.1], 0.0)
    with pytest.raises(ValueError):
        ops.distance_stats(z(8), [0.1], 1.0, n_classes=2)
    with pytest.raises(TypeError):
        ops.distance_stats(z(8), [0.1], 1.0, surf=z(8), class_id=z(3, dtype=i32), n_classes=2)
    with pytest.raises(ValueError):
        ops.distance_stats(z(8), [0.1], 1.0, surf=z(7, dtype=i32), class_id=z(3, dtype=i32), n_classes=2)
