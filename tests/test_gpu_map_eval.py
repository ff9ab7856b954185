"""GPU: the map-evaluation kernels (csrc/map_eval.hip) against tests/map_eval_restated.py -- float32 bit for bit, float64
within the simulator's bound (1 mm; ids wherever the two nearest surfaces are more than 2 mm apart; at most 1 % of the points
excluded) --, the simulator against the evaluator (two independent code paths: every clean return lies on the surface its ray
hit), map_to_map against a brute-force evaluation, and ResultLogger.evaluate against the direct calls.

Every observed figure goes to test_logs/map_eval_errors.log (DESIGN.md 7h quotes it).
"""
import json
import math

import numpy as np
import pytest
import torch

import map_eval_cases as C
import map_eval_restated as RS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THR = (0.05, 0.1, 0.2, 0.5)
MAX_DIST = 1.0
VOXEL = 1.0             # voxel size of the maps of tests 6 and 7: a few thousand points, so that brute force takes a second


def EV():
    from deeppointmap_amd import evaluate
    return evaluate


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def kernel_scene_distance(scene, pts, origin):
    d, s = EV().scene_distance(up(pts), scene, origin)
    return d.cpu().numpy(), s.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("P", [0, 1, 64, 65, 130])
def test_scene_distance_equals_the_float32_restatement_bit_for_bit(P):
    scene = C.mixed_scene(P)
    for M in (1, 255, 257, 1000):
        pts = C.mixed_points(scene, M)
        origin = C.bbox_centre(pts)
        want_d, want_s = RS.scene_distance32(pts, RS.records(scene.params, scene.kind, origin), scene.z0 - origin[2], origin)
        got_d, got_s = kernel_scene_distance(scene, pts, origin)
        bad = int((got_d.view(np.uint32) != want_d.view(np.uint32)).sum()), int((got_s != want_s).sum())
        C.log(f"scene_distance vs float32 restatement, P={P} M={M}: {bad[0]} distances and {bad[1]} ids differ")
        assert bad == (0, 0)
        if M >= 255:
            assert np.isnan(pts).any() and (got_s == -1).sum() == 1 and np.isinf(got_d[got_s == -1]).all()
            assert (got_s == P).any()                                   # the ground is somebody's nearest surface


@pytest.mark.parametrize("case", C.rule_cases(), ids=lambda c: c.name.replace(" ", "_").replace(",", "").replace(":", ""))
def test_rule_cases_through_the_kernel(case):
    """the constructed ties (the lower index wins; the ground loses), the regions of a yawed box and of a cylinder, the
    empty scene and the NaN row, with their exact answers"""
    for origin in ((0.0, 0.0, 0.0), (2.0, -4.0, 1.0)):
        d, s = kernel_scene_distance(case.scene, case.points, origin)
        assert d.tolist() == case.want_dist and s.tolist() == case.want_surf, (origin, d, s)


def test_default_origin_is_the_bounding_box_centre_and_two_runs_give_identical_bytes():
    ev = EV()
    scene = C.mixed_scene(65)
    pts = C.mixed_points(scene, 1000)
    assert ev.bounding_box_centre(up(pts)) == C.bbox_centre(pts)
    a = ev.scene_distance(up(pts), scene)
    b = kernel_scene_distance(scene, pts, C.bbox_centre(pts))
    c = ev.scene_distance(up(pts), scene)
    assert same_bits(a[0].cpu().numpy(), b[0]) and same_bits(a[1].cpu().numpy(), b[1])
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


# ---------------------------------------------------------------------------------------------------------------- 2
def test_scene_distance_against_float64_one_kilometre_from_the_origin():
    scene, pts = C.far_cloud()
    got_d, got_s = kernel_scene_distance(scene, pts, C.bbox_centre(pts))
    d64, s64, gap = RS.scene_distance64(scene.params, scene.kind, scene.z0, pts.astype(np.float64))
    err = float(np.abs(got_d.astype(np.float64) - d64).max())
    clear = gap > C.GAP
    share = 1.0 - clear.mean()
    C.log(f"scene_distance vs float64, scene_far (1 km off), {pts.shape[1]} points: max |d - d64| = {err:.3e} m (bound "
          f"{C.DIST_BOUND:.0e}), {int((~clear).sum())} points ({100 * share:.3f} %) under the 2 mm gap, "
          f"{int((got_s != s64)[clear].sum())} ids differ outside it")
    assert err <= C.DIST_BOUND
    assert share <= C.EXCLUDED_CAP
    assert np.array_equal(got_s[clear], s64[clear])


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("case", C.nn_cases(), ids=lambda c: c.name.replace(" ", "_").replace("'", ""))
def test_cloud_nn_equals_an_exhaustive_float32_search_bit_for_bit(case):
    ev = EV()
    want_d, want_i = RS.cloud_nn32(case.query, case.target, case.max_dist, case.origin)
    q, t = up(case.query), up(case.target)
    d, i = ev.cloud_nn(q, t, case.max_dist, case.origin)
    d2, i2 = ev.cloud_nn(q, t, case.max_dist, case.origin)
    d, i = d.cpu().numpy(), i.cpu().numpy()
    bad = int((d.view(np.uint32) != want_d.view(np.uint32)).sum()), int((i != want_i).sum())
    C.log(f"cloud_nn vs exhaustive float32 search, {case.name} ({case.query.shape[1]} x {case.target.shape[1]}): "
          f"{bad[0]} distances and {bad[1]} indices differ, {int((i >= 0).sum())} matched")
    assert bad == (0, 0)
    assert same_bits(d2.cpu().numpy(), d) and same_bits(i2.cpu().numpy(), i)             # two calls: identical bytes
    if case.name == "ties and the boundary":
        assert i[255] == 7 and d[255] == 0.5 and i[256] == -1 and np.isinf(d[256])      # at max_dist: in; one ulp beyond: out
        assert (d[:100] == 0).all() and (i[:100] == np.arange(40, 140)).all()           # of two equal targets the lower index
    if case.name == "non-finite coordinates":
        assert (i[3:6] == -1).all() and not np.isin(i, [5, 6, 7]).any()
    if case.name == "all targets at one position":
        assert set(i.tolist()) <= {-1, 0} and (i == 0).any()
    if case.target.shape[1]:
        assert (i >= 0).any() and ((i < 0).any() or case.name == "one and one")
    else:
        assert (i == -1).all() and np.isinf(d).all()


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("M", [1, 4095, 4097, 20000])
@pytest.mark.parametrize("n_classes,T", [(0, 1), (5, 8), (0, 8), (5, 1)])
def test_distance_stats_counts_are_exact_and_sums_within_1e12_of_fsum(M, n_classes, T):
    ev = EV()
    rng = np.random.Generator(np.random.PCG64(100 * M + 10 * n_classes + T))
    d = (rng.random(M) ** 2 * 1.5).astype(np.float32)                    # some beyond max_dist = 1
    d[rng.random(M) < 0.05] = np.inf
    if M > 1:
        d[M // 2] = np.float32(1.0)                                      # exactly max_dist: matched
    surf = rng.integers(-1, 12, M).astype(np.int32)                      # -1 and 11: in no class
    class_id = np.array([0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 7], np.int32)     # class 7 of surface 10: beyond C
    thr = [0.05, 0.1, 0.2, 0.3, 0.5, 0.7, 1.0, 2.0][:T]
    want = RS.stats(d, thr, 1.0, surf, class_id, C=n_classes)
    kw = dict(surf=up(surf), class_id=up(class_id), n_classes=n_classes) if n_classes else {}
    a = ev.distance_stats(up(d), thr, 1.0, **kw)
    b = ev.distance_stats(up(d), thr, 1.0, **kw)
    got = a.cpu().numpy()
    assert got.shape == want.shape == (n_classes + 1, 5 + T) and got.dtype == np.float64
    assert same_bits(got, b.cpu().numpy())                               # two runs: identical bytes
    counts = [0, 1] + list(range(5, 5 + T))
    assert np.array_equal(got[:, counts], want[:, counts]) and np.array_equal(got[:, 4], want[:, 4])
    assert got[-1, 0] + got[-1, 1] == M
    rel = np.abs(got[:, 2:4] - want[:, 2:4]) / np.maximum(np.abs(want[:, 2:4]), 1e-300)
    C.log(f"distance_stats vs fsum, M={M} C={n_classes} T={T}: counts and max exact, sums within {float(rel.max()):.2e} relative")
    assert float(rel.max()) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------- 5-7
@pytest.fixture(scope="module")
def street():
    """clean SMALL16 scans of 8 poses of a street scene, through the simulator's kernels: per scan the sensor-frame points
    (n,3) float32, the primitive each ray hit, and the points in the world (float64 move, rounded to float32)"""
    from deeppointmap_amd import lidar_sim as LS
    scene, poses, shifted = C.street()
    dev = scene.to_device(DEV)
    with torch.cuda.device(DEV):
        cast = LS.cast_rays(dev, poses, LS.SMALL16)
        frames, _, _ = LS.emit_frames(*cast, LS.SMALL16, poses, scene=dev)
    scans, prims, world = [], [], []
    for f, pcd in enumerate(frames):
        n = pcd.nbr_point
        xyz, idx = pcd.xyz[:n].cpu().numpy(), pcd.idx[:n].long()
        scans.append(xyz)
        prims.append(cast[1][f][idx].cpu().numpy())
        world.append(C.world_points(xyz, poses[f]))
    return dict(scene=scene, poses=poses, shifted=shifted, scans=scans, prims=prims, world=world)


def test_every_simulated_return_lies_on_the_surface_its_ray_hit(street):
    ev = EV()
    scene = street["scene"]
    pts, prim = np.concatenate(street["world"], axis=1), np.concatenate(street["prims"])
    assert pts.shape[1] > 20000 and (prim >= 0).all()
    d, s = ev.scene_distance(up(pts), scene)
    dist, surf = d.cpu().numpy(), s.cpu().numpy()
    _, _, gap = RS.scene_distance64(scene.params, scene.kind, scene.z0, pts.astype(np.float64))
    clear = gap > C.GAP
    share = 1.0 - clear.mean()
    C.log(f"simulator -> evaluator, street scene {C.STREET_SEED}, 8 clean SMALL16 scans, {pts.shape[1]} returns: max distance to "
          f"the scene {float(dist.max()):.3e} m (bound 2e-03), {int((~clear).sum())} returns ({100 * share:.3f} %) under the 2 mm gap, "
          f"{int((surf != prim)[clear].sum())} ids differ from the ray's outside it")
    assert float(dist.max()) <= 2e-3              # the simulator's 1 mm against float64 plus this kernel's
    assert share <= C.EXCLUDED_CAP
    assert np.array_equal(surf[clear], prim[clear])
    # the per-class rows of map_accuracy against numpy on the kernel's own distances and ids
    from deeppointmap_amd import lidar_sim as LS
    acc = ev.map_accuracy(up(pts), scene, THR, MAX_DIST)
    class_id = np.concatenate([scene.class_id, [LS.GROUND]]).astype(np.int32)
    want = RS.stats(dist, THR, MAX_DIST, surf, class_id, C=5)
    assert list(acc["classes"]) == ["ground", "building", "vehicle", "pole", "trunk"]
    for row, got in zip(want, list(acc["classes"].values()) + [acc["total"]]):
        n = row[0] + row[1]
        assert got["n"] == n and got["matched"] == row[0] and n > 0
        assert got["max"] == row[4] and abs(got["mean"] - row[2] / row[0]) <= 1e-12 * row[2] / row[0]
        assert abs(got["rmse"] - math.sqrt(row[3] / row[0])) <= 1e-12 * math.sqrt(row[3] / row[0])
        assert list(got["within"].values()) == [row[5 + k] / n for k in range(len(THR))] and got["unmatched_share"] == row[1] / n
    assert acc["total"]["n"] == pts.shape[1] and acc["total"]["within"]["0.05"] == 1.0


def _maps(street, poses):
    from deeppointmap_amd.globalmap import voxel_map
    clouds = [up(s.T) for s in street["scans"]]
    return voxel_map(clouds, torch.from_numpy(poses).float(), VOXEL, device=DEV)[0]


def test_map_to_map_equals_a_brute_force_evaluation(street):
    ev = EV()
    ref, est = _maps(street, street["poses"]), _maps(street, street["shifted"])
    origin = ev.bounding_box_centre(est, ref)
    m = ev.map_to_map(est, ref, THR, MAX_DIST, origin=origin)
    e, r = est.cpu().numpy(), ref.cpu().numpy()
    d_acc, _ = RS.cloud_nn32(e, r, MAX_DIST, origin, block=256)
    d_cmp, _ = RS.cloud_nn32(r, e, MAX_DIST, origin, block=256)
    for key, d, row in (("precision", d_acc, m["accuracy"]), ("recall", d_cmp, m["completeness"])):
        t = RS.stats(d, THR, MAX_DIST)[0]
        assert row["n"] == len(d) and row["matched"] == t[0]
        for k, thr in enumerate(THR):
            assert m[key][f"{thr:g}"] == t[5 + k] / len(d) == row["within"][f"{thr:g}"]
        assert abs(row["mean"] - t[2] / t[0]) <= 1e-12 * t[2] / t[0]
    p, q = m["precision"]["0.1"], m["recall"]["0.1"]
    C.log(f"map_to_map, every second pose {C.SHIFT} m off, {VOXEL} m voxel maps of {e.shape[1]} / {r.shape[1]} points: precision "
          f"{p:.4f} recall {q:.4f} at 0.1 m, chamfer {m['chamfer']:.4f} m")
    assert 0 < p < 1 and 0 < q < 1 and m["fscore"]["0.1"] == 2 * p * q / (p + q)
    assert m["chamfer"] == m["accuracy"]["mean"] + m["completeness"]["mean"]
    same = ev.map_to_map(ref, ref.clone(), THR, MAX_DIST)
    assert same["precision"]["0.1"] == 1.0 and same["recall"]["0.1"] == 1.0 and same["chamfer"] == 0.0 and same["fscore"]["0.05"] == 1.0


def test_result_logger_evaluate_with_maps_equals_the_direct_calls(street, tmp_path):
    from deeppointmap_amd.consumer import Rank0Consumer
    from deeppointmap_amd.system import ResultLogger
    ev = EV()
    b = Rank0Consumer(None, DEV, slam_args=dict(result_maps=True))
    for f, scan in enumerate(street["scans"]):
        b.type[f] = "full" if f % 2 == 0 else "non-keyframe"
        b.poses[f] = torch.from_numpy(street["shifted"][f]).float()
        b.gt[f] = torch.from_numpy(street["poses"][f]).float()
        b.map_clouds[f] = up(scan.T)
    out = ResultLogger(b, str(tmp_path)).evaluate("metrics", scene=street["scene"], voxel_size=VOXEL, thresholds=THR, max_dist=MAX_DIST)
    disk = json.load(open(tmp_path / "metrics.json"))
    assert disk == json.loads(json.dumps(out)) and all(disk[k] is not None for k in ("trajectory", "map_to_map", "map_accuracy"))
    est, gt = np.stack([b.poses[f].double().numpy() for f in range(8)]), np.stack([b.gt[f].double().numpy() for f in range(8)])
    assert out["trajectory"] == ev.trajectory_metrics(est, gt)
    assert 0.0 < out["trajectory"]["ate"]["rmse"] < C.SHIFT and out["trajectory"]["rpe"]["n"] == 7
    pred, ref = _maps(street, street["shifted"]), _maps(street, street["poses"])
    m = ev.map_to_map(pred, ref, THR, MAX_DIST)
    a = ev.map_accuracy(pred, street["scene"], THR, MAX_DIST)
    assert {k: v for k, v in out["map_to_map"].items() if k != "scans"} == m and out["map_to_map"]["scans"] == 8
    assert {k: v for k, v in out["map_accuracy"].items() if k != "scans"} == a and out["map_accuracy"]["scans"] == 8
    assert a["total"]["within"]["0.5"] >= a["total"]["within"]["0.05"] and 0.0 < a["total"]["within"]["0.05"] < 1.0
