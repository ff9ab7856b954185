"""CPU: the restatement of the scan-to-TSDF registration (tests/tsdf_register_restated.py) against known answers, before any
kernel is compared with it.

  known answer   three tilted wall patches fused once in the plane form with true normals (voxel 0.5 m, truncation 1.5 m); 1100
                 of their returns started 0.3 m and 2 degrees off come back within the project's pose bar (1e-4 m, 1e-4 in
                 || R - R_true ||_F) in float64, at the origin and with the map origin 1 km away; in float32 within 1e-4 m at
                 the origin and 1e-3 m 1 km out.  The field of the plane form is exactly linear in a band fed by one plane.
  mutants        the four mutants of the restatement differ from the rule on these inputs: the cell anchored at the voxel's
                 floor, the gradient not divided by v and J's rotation part negated miss the known answer; a missing corner read
                 as 0 changes rows at a patch border, and only there.
  two forms      float32 against float64 `sample`: d within 1 mm wherever both have a value, grad within 1e-3 away from the cell
                 faces, the ambiguous rows under 1 %.
  one patch      a plane alone constrains three of six freedoms: SINGULAR, the pose's bytes those of the start.
  tracker        the box room in float64: the plane form's final error is logged with the ray form's beside it.
Every figure goes to test_logs/tsdf_register_errors.log.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_register_restated as TR  # noqa: E402
import tsdf_restated as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
FAR = (1000.0, -500.0, 20.0)


def log(line):
    print(line)
    try:
        os.makedirs(os.path.join(ROOT, "test_logs"), exist_ok=True)
        with open(os.path.join(ROOT, "test_logs", "tsdf_register_errors.log"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


_CASES = {}


def case(origin=(0.0, 0.0, 0.0), which=(0, 1, 2), distance="plane"):
    """the scene, its fused restatement and the exported field, made once and left unchanged"""
    key = (tuple(origin), tuple(which), distance)
    if key not in _CASES:
        c = TR.patches_case(origin, which)
        c.map = TR.fuse_case(c, distance)
        c.exported = c.map.export()
        c.unit = 256 if distance == "plane" else 1
        c.tau = 3 * c.voxel
        _CASES[key] = c
    return _CASES[key]


def run(c, dtype, **kw):
    fld = R.field(c.exported, c.unit, F32 if dtype == F32 else np.float64)
    return TR.register(fld, c.voxel, c.src, c.origin, c.start, [(c.tau, 40)], dtype=dtype, **kw)


# --------------------------------------------------------------------------------------------------------------- known answer
@pytest.mark.parametrize("origin,dtype,bound_t", [((0.0, 0.0, 0.0), np.float64, 1e-4), (FAR, np.float64, 1e-4),
                                                  ((0.0, 0.0, 0.0), F32, 1e-4), (FAR, F32, 1e-3)])
def test_three_patches_come_back(origin, dtype, bound_t):
    c = case(origin)
    r = run(c, dtype)
    dt, dr = TR.pose_error(r["pose"], c.pose)
    d0, r0 = TR.pose_error(c.start, c.pose)
    log(f"host: three patches, plane form, {np.dtype(dtype).name}, map origin {tuple(origin)}: start {d0:.3f} m / {r0:.3e}, status "
        f"{r['status']}, iterations {r['iterations']}, translation error {dt:.3e} m, |R - R_true|_F {dr:.3e}, fitness {r['fitness']:.3f}, "
        f"rmse {r['rmse']:.3e}")
    assert 0.25 < d0 < 0.4 and r["status"] == TR.CONVERGED and r["fitness"] > 0.8
    assert dt <= bound_t and dr <= 1e-4, (dt, dr)


def test_the_ray_form_is_not_held_to_the_truth():
    """the ray form's field is not a distance off the ray's axis: the same input stalls millimetres from the truth (logged)"""
    c = case(distance="ray")
    r = run(c, np.float64)
    dt, dr = TR.pose_error(r["pose"], c.pose)
    log(f"host: three patches, RAY form, float64: status {r['status']}, iterations {r['iterations']}, translation error {dt:.3e} m, "
        f"|R - R_true|_F {dr:.3e}, fitness {r['fitness']:.3f} (logged, no bar)")
    assert r["status"] in (TR.CONVERGED, TR.MAX_ITER) and dt < 0.3


# -------------------------------------------------------------------------------------------------------------------- mutants
@pytest.mark.parametrize("mutant", [dict(anchor_floor=True), dict(divide=False), dict(negate_rot=True)])
def test_mutants_miss_the_known_answer(mutant):
    c = case()
    r = run(c, np.float64, **mutant)
    dt, dr = TR.pose_error(r["pose"], c.pose)
    log(f"host: mutant {mutant}: status {r['status']}, translation error {dt:.3e} m, |R - R_true|_F {dr:.3e}")
    assert r["status"] != TR.CONVERGED or dt > 1e-4 or dr > 1e-4


def test_a_missing_corner_read_as_zero_changes_rows_at_a_patch_border():
    c = case()
    fld = R.field(c.exported, c.unit, F32)
    true = TR.sample(fld, c.voxel, c.xyz, c.pose, c.origin, F32)
    bad = TR.sample(fld, c.voxel, c.xyz, c.pose, c.origin, F32, corners7=True)
    changed = true.flag != bad.flag
    log(f"host: mutant corners7: {int(changed.sum())} of {len(c.xyz)} rows change, all with 7 corners: {bool((true.corners[changed] == 7).all())}; "
        f"largest |d| among them {float(np.abs(bad.d[changed]).max()):.3e} m on points that lie on the surface")
    assert changed.any() and (true.corners[changed] == 7).all() and (true.flag[changed] == 0).all()
    same = ~changed
    assert bad.d[same].tobytes() == true.d[same].tobytes() and bad.grad[same].tobytes() == true.grad[same].tobytes()
    S0 = TR.system(true, c.tau, 0.5, 0.0, F32)[0]
    S1 = TR.system(bad, c.tau, 0.5, 0.0, F32)[0]
    assert S1[27] > S0[27] and S1[28] > S0[28]


# ------------------------------------------------------------------------------------------------------------------ two forms
@pytest.mark.parametrize("origin", [(0.0, 0.0, 0.0), FAR])
def test_float32_sample_against_float64(origin):
    c = case(origin)
    rng = np.random.default_rng(3)
    pts = np.concatenate([c.xyz, c.xyz + rng.normal(0, 0.4, c.xyz.shape).astype(F32)])     # on the surface, and round it
    s32 = TR.sample(R.field(c.exported, c.unit, F32), c.voxel, pts, c.start, c.origin, F32)
    s64 = TR.sample(R.field(c.exported, c.unit, np.float64), c.voxel, pts, c.start, c.origin, np.float64)
    dd, dg, doubt = TR.compare_samples(s32, s64, c.voxel)
    log(f"host: sample float32 against float64, map origin {tuple(origin)}: {int((s32.flag == 1).sum())} of {len(pts)} rows have a value, "
        f"max |d32 - d64| {dd:.3e} m, max |grad32 - grad64| {dg:.3e}, ambiguous share {doubt:.2e}")
    assert (s32.flag == 1).sum() > len(pts) // 2
    assert dd <= 1e-3 and dg <= 1e-3 and doubt < 0.01


def test_the_field_is_linear_where_one_plane_feeds_it():
    """the known answer rests on this: on the returns themselves, under the true pose, d = 0 and |grad| = 1 to rounding"""
    c = case()
    s = TR.sample(R.field(c.exported, c.unit, np.float64), c.voxel, c.xyz, c.pose, c.origin, np.float64)
    has = s.flag == 1
    inner = has & (np.abs(np.sqrt(s.n2) - 1) < 1e-3)
    log(f"host: on the fused returns under the true pose: {int(has.sum())} of {len(has)} have a value, {int(inner.sum())} with |grad| within 1e-3 "
        f"of 1; among those max |d| {float(np.abs(s.d[inner]).max()):.3e} m")
    assert inner.sum() > 0.7 * len(has) and np.abs(s.d[inner]).max() < 1e-5


# ------------------------------------------------------------------------------------------------------------------ one patch
@pytest.mark.parametrize("dtype", [np.float64, F32])
def test_one_patch_alone_is_singular(dtype):
    c = case(which=(0,))
    r = run(c, dtype)
    log(f"host: one patch alone, {np.dtype(dtype).name}: status {r['status']}, iterations {r['iterations']}, fitness {r['fitness']:.3f}")
    assert r["status"] == TR.SINGULAR and r["iterations"] == 0 and r["pose"].tobytes() == c.start.tobytes()


# -------------------------------------------------------------------------------------------------------------------- tracker
BOX_KW = dict(voxel=0.25, register_every=3)
_BOX = {}


def box_tracker(distance, dtype=np.float64):
    """the box-room run of the restatement's tracker, made once per form -> (poses, statuses, fitnesses, lost, true poses)"""
    if (distance, dtype) not in _BOX:
        xyz, nrm, poses = TR.box_room()
        out = TR.tracker(xyz, nrm if distance == "plane" else None, poses[0], distance=distance, dtype=dtype, **BOX_KW)
        _BOX[(distance, dtype)] = out[:4] + (poses,)
    return _BOX[(distance, dtype)]


def test_box_room_tracker_in_float64():
    final = {}
    for distance in ("plane", "ray"):
        poses, statuses, fits, lost, true = box_tracker(distance)
        err = np.linalg.norm(poses[:, :3, 3] - true[:, :3, 3], axis=1)
        final[distance] = float(err[-1])
        log(f"host: box-room tracker, {distance} form, float64: statuses {statuses}, lost {lost}, fitness {min(fits):.3f}..{max(fits):.3f}, "
            f"translation error per frame (mm) {np.round(err * 1e3, 2).tolist()}")
        assert lost == 0 and all(s in (TR.CONVERGED, TR.MAX_ITER) for s in statuses)
    log(f"host: box-room tracker, final translation error: plane form {final['plane'] * 1e3:.2f} mm, ray form {final['ray'] * 1e3:.2f} mm")
    assert final["plane"] < 0.05
