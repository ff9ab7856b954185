"""CPU: the adaptive gate of deeppointmap_amd/odometry.py on hand-made cases, the numpy restatement of the voxel planes and
the plane rows (tests/lidar_plane_restated.py) on exact cases and against itself, the sliding case that is the reason for
point-to-plane rows, the scenes of the GPU tests (which must meet the GPU tests' premises in the restatement alone), and
the argument refusals of the two new C entry points (before any HIP call: they need no GPU)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restated as I  # noqa: E402
import lidar_odometry_restated as L  # noqa: E402
import lidar_plane_restated as PR  # noqa: E402

EYE = np.eye(4)
DTYPES = [np.float32, np.float64]


def exported(pts, voxel=1.0, s=3, dtype=np.float32):
    m = L.Map(voxel, s, dtype=dtype, max_range=1e4)
    m.insert(np.asarray(pts, np.float32), np.arange(len(pts)), EYE, 0)
    return m.export()


# -------------------------------------------------------------------------------------------------------------- adaptive gate
def test_adaptive_sigma_on_hand_made_lists():
    from deeppointmap_amd.odometry import adaptive_sigma
    assert adaptive_sigma([], 2.0) == 2.0
    assert adaptive_sigma([3.0, 4.0], 2.0) == np.sqrt(12.5)
    assert adaptive_sigma([0.3], 2.0) == 0.3
    # at or below min_motion a deviation does not count: the sensor stood still, and the threshold would collapse
    assert adaptive_sigma([0.05, 0.1], 2.0, min_motion=0.1) == 2.0
    assert adaptive_sigma([0.05, 0.1, 3.0, 4.0], 2.0, min_motion=0.1) == np.sqrt(12.5)
    assert adaptive_sigma([0.6, 0.8], 1.0) == PR.sigma_of([0.6, 0.8], 1.0, 0.0)


def test_gate_is_three_sigma_clipped_at_the_voxel_and_the_scale_a_third():
    from deeppointmap_amd.odometry import LidarOdometry, adaptive_stage
    assert adaptive_stage(0.2, 1.0, 30) == ((3.0 * 0.2, 30), 0.2 / 3.0)
    assert adaptive_stage(0.5, 1.0, 7) == ((1.0, 7), 0.5 / 3.0)                        # 1.5 is clipped
    assert adaptive_stage(5.0, 0.7, 7) == ((float(np.float32(0.7)), 7), 5.0 / 3.0)     # the fp32 voxel the search checks against
    odo = LidarOdometry(voxel_size=1.0, schedule=((1.0, 5), (0.5, 9)), kernel_scale=0.25, max_range=50.0)
    assert odo.gate() == ([(1.0, 5), (0.5, 9)], 0.25), "without adaptive: the schedule and the scale as given"
    odo = LidarOdometry(voxel_size=1.0, schedule=((1.0, 5), (0.5, 9)), kernel_scale=0.25, max_range=50.0, adaptive=(2.0, 0.1))
    assert odo.gate() == ([(1.0, 9)], 2.0 / 3.0), "sigma0, one stage, max_iter of the last stage"
    odo.deviations = [0.05, 0.12, 0.16]
    sigma = np.sqrt((0.12 ** 2 + 0.16 ** 2) / 2)
    assert odo.gate() == ([(3.0 * sigma, 9)], sigma / 3.0)
    with pytest.raises(ValueError):
        LidarOdometry(adaptive=(0.0, 0.1))
    with pytest.raises(ValueError):
        LidarOdometry(metric="hybrid")


def test_deviation_of_a_pure_translation_and_a_pure_rotation():
    from deeppointmap_amd.odometry import prediction_deviation
    pred = I.se3([0.1, -0.2, 0.3], [5.0, -3.0, 1.0])
    assert prediction_deviation(pred, pred, 80.0) < 1e-12
    shift = pred @ I.se3([0, 0, 0], [0.3, -0.4, 0.0])
    assert abs(prediction_deviation(pred, shift, 80.0) - 0.5) < 1e-14
    turn = pred @ I.se3([0, 0, np.radians(2.0)], [0, 0, 0])
    want = 2 * 80.0 * np.sin(np.radians(1.0))        # the chord a point at max_range moves along
    assert abs(prediction_deviation(pred, turn, 80.0) - want) < 1e-12
    both = pred @ I.se3([0, np.radians(2.0), 0], [0.3, -0.4, 0.0])
    assert abs(prediction_deviation(pred, both, 80.0) - (0.5 + want)) < 1e-12
    assert abs(PR.deviation(pred, both, 80.0) - prediction_deviation(pred, both, 80.0)) < 1e-12


# ------------------------------------------------------------------------------------------------------ planes on exact cases
@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_axis_plane_lattices_give_the_axis_exactly(axis, s):
    ex = exported(PR.plane_lattice(axis, 0.25, centre=(-0.5, 0.25, 1.0)), s=s)
    want = np.zeros(3, np.float32)
    want[axis] = 1
    mirror, free = PR.planes(ex, 1.0, 1.5, np.float32), PR.planes(ex, 1.0, 1.5, np.float64)
    assert np.array_equal(mirror.counts, free.counts) and len(mirror.keys) == 9 and mirror.counts.max() >= 6
    defined = mirror.w >= 0
    assert defined.sum() >= 4 and np.array_equal(defined, free.w >= 0)
    for i in np.nonzero(defined)[0]:
        assert mirror.normal[i].tobytes() == want.tobytes() and mirror.w[i].tobytes() == np.float32(0).tobytes()
    # numpy's eigh is not held to bits: within rounding of the same
    assert PR.angle(free.normal[defined], np.broadcast_to(want, (int(defined.sum()), 3))).max() < 1e-7
    assert np.abs(free.w[defined]).max() < 1e-12
    # every voxel that is not defined says so in one way
    assert (mirror.normal[~defined] == 0).all() and (mirror.w[~defined] == -1).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_fewer_than_three_points_or_a_line_have_no_plane(dtype):
    P = PR.planes(exported([[0.5, 0.5, 0.5], [10.5, 0.5, 0.5], [10.5, 0.6, 0.9]], s=3), 1.0, 1.5, dtype)
    assert list(P.counts) == [1, 2] and (P.w == -1).all() and (P.normal == 0).all()
    # three points on a line: the middle eigenvalue is zero as well
    P = PR.planes(exported([[0.25, 0.5, 0.5], [0.5, 0.5, 0.5], [0.75, 0.5, 0.5]], s=3), 1.0, 1.5, np.float32)
    assert list(P.counts) == [3] and P.w[0] == -1


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_line_rounded_to_float32_has_no_plane(dtype):
    """nine points of a straight line 50 m out: the float32 rounding leaves l1 / l2 near 1e-12, not 0, and the eigenvector of
    l0 is that rounding's; the same line with 2 mm of thickness is a (thin) plane"""
    ex = exported(PR.wall_line())
    P = PR.planes(ex, 1.0, 1.5, dtype)
    assert P.counts.max() >= 5 and (P.w == -1).all() and (P.normal == 0).all()
    thick = PR.wall_line().astype(np.float64)
    thick[::2, 2] += 0.002
    P = PR.planes(exported(thick), 1.0, 1.5, dtype)
    assert (P.w[P.counts >= 5] >= 0).all() and (P.counts >= 5).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_membership_at_the_balls_surface_and_over_voxel_faces(dtype):
    # voxel (0,0,0) has its centre at .5.  (-1, .5, .5) on the far face of a neighbour and (1.5, 1.5, 1) lie exactly 1.5 away:
    # members.  (1.5, 1.5, 1.125) and (.5, -.5, -.75) lie in neighbours but farther: not.  (2, .5, .5) is 1.5 away as well, but
    # a point ON the far face towards + belongs to the voxel after the neighbour, which is not among the 27: not a member.
    pts = [[0.5, 0.5, 0.5], [-1.0, 0.5, 0.5], [1.5, 1.5, 1.0], [1.5, 1.5, 1.125], [0.5, -0.5, -0.75], [2.0, 0.5, 0.5]]
    P = PR.planes(exported(pts, s=3), 1.0, 1.5, dtype)
    at = int(np.searchsorted(P.keys, L.pack_key([0, 0, 0])))
    assert P.counts[at] == 3
    P = PR.planes(exported(pts, s=3), 1.0, 1.25, dtype)
    assert P.counts[int(np.searchsorted(P.keys, L.pack_key([0, 0, 0])))] == 1


def test_sign_rule_largest_component_positive_first_axis_among_equals():
    lam = np.array([[0.0, 1.0, 2.0]])
    for v, want in (([0.6, 0.0, -0.8], [-0.6, 0.0, 0.8]), ([0.8, -0.6, 0.0], [0.8, -0.6, 0.0]), ([-1.0, 1.0, 0.0], [1.0, -1.0, 0.0]),
                    ([0.0, -1.0, 1.0], [0.0, 1.0, -1.0]), ([0.0, 0.0, -1.0], [0.0, 0.0, 1.0])):
        vec = np.zeros((1, 3, 3))
        vec[0, :, 0] = v
        normal, w, _ = PR.finish(lam[:1], vec, np.array([9]))
        unit = (np.array(want) / np.linalg.norm(want)).astype(np.float32)
        assert normal[0].tobytes() == unit.tobytes() and w[0] == 0, (v, normal)
    # a tilted lattice plane x = y: the normal is (1, -1, 0) / sqrt 2 with x positive, in both forms
    a = (np.arange(9) - 4) * 0.25
    u, v = [g.ravel() for g in np.meshgrid(a, a, indexing="ij")]
    ex = exported(np.stack([u, u, v], axis=1) + 0.5)
    for dtype in DTYPES:
        P = PR.planes(ex, 1.0, 1.5, dtype)
        ok = P.w >= 0
        assert ok.sum() >= 3 and (P.normal[ok, 0] > 0.707).all() and (P.normal[ok, 1] < -0.707).all()


def test_jacobi_is_an_eigendecomposition():
    rng = np.random.default_rng(1)
    B = rng.normal(size=(50, 3, 3))
    A = B @ B.transpose(0, 2, 1)
    lam, V = PR.jacobi(A)
    assert np.abs(V @ (lam[:, :, None] * V.transpose(0, 2, 1)) - A).max() < 1e-12
    assert np.abs(np.sort(lam, axis=1) - np.linalg.eigvalsh(A)).max() < 1e-12


# --------------------------------------------------------------------------------------------------------- the GPU tests' scenes
@pytest.mark.parametrize("s", [1, 2, 3])
def test_normals_scene_meets_the_gpu_tests_premises(s):
    """both forms count alike, and the voxels left out of the angle check for a small gap are at most 2 % of those with >= 5
    points: shown here on the restatement alone"""
    ex = exported(PR.normals_scene(), s=s)
    mirror, free = PR.planes(ex, 1.0, 1.5, np.float32), PR.planes(ex, 1.0, 1.5, np.float64)
    assert np.array_equal(mirror.counts, free.counts) and len(free.keys) > 500
    big = free.counts >= 5
    low = big & (free.gap < 1e-3)
    assert low.sum() <= 0.02 * big.sum()
    check = big & ~low
    assert PR.angle(mirror.normal[check], free.normal[check]).max() < 1e-6 and np.abs(mirror.w - free.w)[check].max() < 1e-5
    assert PR.gate(free.counts, free.w).sum() > 300 and (~PR.gate(free.counts, free.w)).sum() > 50


def test_plane_rows_are_icp_restateds_and_ungated_matches_drop_out():
    rng = np.random.default_rng(2)
    ex = exported(PR.normals_scene())
    P = PR.planes(ex, 1.0, 1.5, np.float64)
    normals, ok = PR.per_row(ex, P)
    assert normals.shape == (len(ex[0]), 3) and 0 < ok.sum() < len(ok)
    q = ex[3][rng.choice(len(ex[0]), 400, replace=False)].astype(np.float64) + rng.normal(0, 0.02, (400, 3))
    win = L.search_fast(q, ex, 1.0, 3, 1.0, np.float64)
    S, J, e, w, used = PR.system(q, win, ex[3], normals, ok, 0.1, np.float64)
    assert S[27] == (used >= 0).sum() == ((win >= 0) & ok[np.maximum(win, 0)]).sum() < (win >= 0).sum()
    J2, e2 = I.rows(q, used, ex[3], normals, I.PLANE, np.float64)
    assert np.array_equal(J, J2) and np.array_equal(e, e2)
    k = 0.01
    assert np.allclose(w, (k / (k + e * e)) ** 2) and S[28] == (e * e).sum()
    assert np.allclose(S[21:27], (w[:, None] * J * e[:, None]).sum(axis=0))
    assert (PR.system_floor(J, e, w, 0.1, 1e-6) >= I.system_floor(J, e, 1e-6) * w.min() - 1e-18).all()


# ------------------------------------------------------------------------------------------------------------ the sliding case
def test_sliding_case_plane_rows_find_the_motion_point_rows_do_not():
    """Ground rings and two perpendicular walls, 16 x 256 rays; frame 1 is 0.5 m and 1 degree on and starts from the pose of
    frame 0; max_dist = voxel = 1 m, kernel scale 0.1 (lidar_plane_restated.sliding_scene: walls at x = 12 and y = 9, beams
    from +8 to -22 degrees, 1.8 m over the ground).  Observed in float64: plane rows 5.6e-4 m, point rows 0.495 m (0.403 m
    unweighted)."""
    r_plane, plane = PR.sliding_case("plane")
    r_point, point = PR.sliding_case("point")
    print(f"sliding case, float64 restatement: plane rows {plane:.3e} m, point rows {point:.3e} m")
    assert r_plane["status"] == L.CONVERGED and r_point["status"] in (L.CONVERGED, L.MAX_ITER)
    assert plane <= 5e-3
    assert point >= 20 * plane


def test_register_with_metric_point_is_the_point_registration():
    f0, f1, P0, P1 = PR.sliding_scene(beams=8, columns=64)
    ex = exported(f0)
    a = PR.register(f1, ex, 1.0, 3, np.zeros(3), EYE, [(1.0, 3)], 0.1, metric="point")
    b = L.register(f1, ex, 1.0, 3, np.zeros(3), EYE, [(1.0, 3)], 0.1)
    assert a["pose"].tobytes() == b["pose"].tobytes() and a["status"] == b["status"]


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_new_entry_points_refuse_bad_arguments_before_any_hip_call():
    from deeppointmap_amd import _lib
    lib = _lib.load()
    for name in ("dpm_local_map_planes", "dpm_local_map_register_planes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    EINVAL = -1
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) & ~255   # never dereferenced: every call below is refused first
    o = (ctypes.c_double * 3)(0, 0, 0)
    oa = ctypes.addressof(o)
    base = dict(map=p, cap_vox=64, s=3, half=0, voxel=1.0, origin=oa, radius=1.5, planes=p, counts=p, stream=None)
    order = ("map", "cap_vox", "s", "half", "voxel", "origin", "radius", "planes", "counts", "stream")
    pl = lambda **k: lib.dpm_local_map_planes(*[{**base, **k}[n] for n in order])
    for k in (dict(map=None), dict(cap_vox=48), dict(s=0), dict(half=2), dict(voxel=0.0), dict(origin=None), dict(radius=0.0),
              dict(radius=1.5000001), dict(radius=float("nan")), dict(planes=None), dict(planes=p + 4), dict(counts=None)):
        assert pl(**k) == EINVAL, k
    dist, iters = (ctypes.c_double * 1)(1.0), (ctypes.c_int32 * 1)(5)
    order = ("map", "cap_vox", "s", "half", "voxel", "origin", "planes", "counts", "min_points", "max_ratio", "xyz", "count", "cap",
             "init", "dist", "iters", "n", "ks", "tr", "tt", "pose", "fit", "rmse", "it", "st", "dk", "ds", "dsys", "ws", "stream")
    base = dict(map=p, cap_vox=64, s=3, half=0, voxel=1.0, origin=oa, planes=p, counts=p, min_points=5, max_ratio=0.1, xyz=p, count=p,
                cap=8, init=p, dist=ctypes.addressof(dist), iters=ctypes.addressof(iters), n=1, ks=0.0, tr=1e-7, tt=1e-6,
                pose=p + 512, fit=p, rmse=p, it=p, st=p, dk=None, ds=None, dsys=None, ws=p, stream=None)
    reg = lambda **k: lib.dpm_local_map_register_planes(*[{**base, **k}[n] for n in order])
    far = (ctypes.c_double * 1)(1.5)
    for k in (dict(planes=None), dict(planes=p + 8), dict(counts=None), dict(min_points=-1), dict(max_ratio=-0.1),
              dict(max_ratio=float("nan")), dict(map=None), dict(xyz=None), dict(cap=0), dict(pose=p), dict(ws=None),
              dict(dist=ctypes.addressof(far)), dict(n=17)):
        assert reg(**k) == EINVAL, k


def test_python_layer_refuses_before_the_gpu():
    from deeppointmap_amd import odometry
    with pytest.raises(ValueError):
        odometry.LocalMap(voxel_size=1.0, plane_radius=1.6)
    with pytest.raises(ValueError):
        odometry.LocalMap(plane_radius=0.0)
    m = odometry.LocalMap(voxel_size=2.0)
    assert m.plane_radius == 3.0
    empty = m.export_planes()
    assert [len(a) for a in empty] == [0, 0, 0, 0] and empty[2].shape == (0, 3)
