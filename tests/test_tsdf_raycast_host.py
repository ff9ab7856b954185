"""CPU: the ray-cast's restatement (tests/tsdf_raycast_restated.py), the inputs of the GPU tests (tests/tsdf_raycast_cases.py)
and the refusals.

  header      include/dpm_hip.h declares the three entry points, the binding table holds them, the library exports them.
  refusals    TsdfMap.raycast / render, ops.tsdf_cast_args and the C entry points refuse bad arguments before any HIP call.
  mutants     the five mutants of cast32 each differ from the true form on the inputs the GPU tests use, and miss the known
              answers where those apply: those inputs can tell a kernel that got the rule wrong.
  inputs      what the constructed cases must show shows: HIT / MISS round max_range, MISS through the 7-corner cell between the
              two signs, BACK from inside the band, MISS everywhere on an empty table and for K = 1.
  float64     cast32 against the independent cast64: flags equal and ranges within 1 mm on the unambiguous rays, also with the
              origin 1 km out; the ambiguous share of each input stays under 1 %.
  answers     the tilted plane, the sphere, the wall seen through and the three patches on the restatement, with the bounds
              the GPU test uses.
Everything observed goes to test_logs/tsdf_raycast.log.
"""
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restated as I  # noqa: E402
import tsdf_cases as C  # noqa: E402
import tsdf_plane_restated as PR  # noqa: E402
import tsdf_raycast_cases as RC  # noqa: E402
import tsdf_raycast_restated as T  # noqa: E402
import tsdf_register_restated as RR  # noqa: E402
import tsdf_restated as R  # noqa: E402
import test_tsdf_plane_host as H  # noqa: E402
from test_tsdf_host import valid  # noqa: E402
from tsdf_raycast_cases import log  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
ENTRY_POINTS = ("dpm_tsdf_blocks_bytes", "dpm_tsdf_blocks", "dpm_tsdf_raycast")
MUTANTS = ("across_gap", "sign_ge", "back_as_hit", "map_normal", "accumulate_t")
RANGE_BOUND = 1e-3        # metres, float32 against float64: the bound of the other TSDF tests
AMBIGUOUS_CAP = 0.01
PLANE_BOUND = 1e-4        # metres from the plane: test_tsdf_plane_host.PLANE_BOUND
MISS_CAP = 0.01


@functools.lru_cache(maxsize=None)
def exported(name):
    """the float32 restatement's sorted export of a cast case's map, fused once"""
    return RC.export_restated(RC.cast_cases()[name])


@functools.lru_cache(maxsize=None)
def true_cast(name):
    return RC.restated(RC.cast_cases()[name], exported(name))


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------- header
def test_the_header_declares_the_three_entry_points():
    from deeppointmap_amd import _lib
    text = open(os.path.join(ROOT, "include", "dpm_hip.h")).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\b(size_t|int) " + name + r"\(", text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert [lib.dpm_tsdf_blocks_bytes(n) for n in (0, 1, 2, 3, 64, 1 << 24, 1 << 25, -4)] == [0, 0, 272, 0, 256 + 8 * 64, 256 + 8 * (1 << 24), 0, 0]
    assert not [n for n in _lib.SIGNATURES if n.startswith("dpm_tsdf") and n.endswith("_workspace_bytes")]


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_raycast_refuses_bad_arguments_before_any_hip_call():
    from deeppointmap_amd import ops
    from deeppointmap_amd.lidar_sim import SMALL16
    from deeppointmap_amd.tsdf import TsdfMap, TsdfTracker
    m = TsdfMap()
    assert m.max_blocks == m.max_voxels // 2 and TsdfMap(max_voxels=2).max_blocks == 2 and TsdfMap(max_blocks=64).max_blocks == 64
    for bad in (0, 1, 3, 1000, 1 << 25):
        with pytest.raises(ValueError):
            TsdfMap(max_blocks=bad)
    dirs = np.zeros((4, 3), F32)
    for kw in (dict(step=0.0), dict(step=-0.1), dict(step=float("nan")), dict(min_range=-1.0), dict(min_range=5.0, max_range=4.0),
               dict(max_range=float("inf")), dict(min_range=0.0, max_range=65537 * 0.1, step=0.1), dict(min_count=0), dict(min_count=-1)):
        with pytest.raises(ValueError):
            m.raycast(np.eye(4), dirs, **kw)
    for poses, rays in ((np.eye(3), dirs), (np.zeros((2, 3, 4)), dirs), (np.eye(4), np.zeros((4, 2), F32)), (np.eye(4), np.zeros(3, F32)),
                        (np.eye(4), np.zeros((4, 3), np.float64))):
        with pytest.raises(ValueError):
            m.raycast(poses, rays)
    with pytest.raises(ValueError):
        m.render(np.eye(3), SMALL16)
    with pytest.raises(ValueError):
        m.blocks()                                       # no table yet
    with pytest.raises(ValueError):
        TsdfTracker().predicted(SMALL16)                 # no frame yet
    assert ops.tsdf_cast_args(0.9, 120.0, 0.1) == (0.9, 120.0, 0.1)
    assert ops.tsdf_cast_args(0.0, 65535 * 0.25, 0.25)[1] == 65535 * 0.25         # K = 65536 is the most
    with pytest.raises(ValueError):
        ops.tsdf_cast_args(0.0, 65536 * 0.25, 0.25)
    assert m.table is None and m.check() is m            # nothing was allocated


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    import ctypes
    from deeppointmap_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) & ~255   # never dereferenced: every call below is refused first, or is a no-op
    o = (ctypes.c_double * 3)(0, 0, 0)
    bad_o = (ctypes.c_double * 3)(0, float("nan"), 0)

    def refusals(fn, names, good, bad):
        call = lambda **k: fn(*[{**good, **k}[n] for n in names])
        for k in bad:
            assert call(**k) == -1, (fn.__name__, k)
        return call
    bad_map = [dict(map=None), dict(map=p + 8), dict(cap_vox=65), dict(cap_vox=1), dict(cap_vox=1 << 25)]
    bad_set = [dict(blocks=p + 8), dict(cap_blocks=65), dict(cap_blocks=1), dict(cap_blocks=1 << 25)]
    refusals(lib.dpm_tsdf_blocks, ("map", "cap_vox", "min_count", "blocks", "cap_blocks", "stream"),
             dict(map=p, cap_vox=64, min_count=1, blocks=p, cap_blocks=64, stream=None),
             bad_map + bad_set + [dict(blocks=None), dict(min_count=0)])
    names = ("map", "cap_vox", "voxel", "origin", "blocks", "cap_blocks", "poses", "F", "dirs", "R", "lo", "hi", "h", "min_count", "range",
             "normals", "flag", "stream")
    good = dict(map=p, cap_vox=64, voxel=0.2, origin=ctypes.addressof(o), blocks=p, cap_blocks=64, poses=p, F=2, dirs=p, R=8, lo=0.5, hi=10.0,
                h=0.1, min_count=1, range=p, normals=p, flag=p, stream=None)
    call = refusals(lib.dpm_tsdf_raycast, names, good, bad_map + bad_set + [
        dict(voxel=0.0), dict(voxel=float("nan")), dict(origin=None), dict(origin=ctypes.addressof(bad_o)), dict(h=0.0), dict(h=-0.1),
        dict(h=float("nan")), dict(lo=-0.5), dict(lo=11.0), dict(hi=float("inf")), dict(hi=float("nan")), dict(lo=0.0, hi=6553.6, h=0.1),
        dict(h=1e-60), dict(min_count=0), dict(F=-1), dict(F=65536), dict(R=-1), dict(poses=None), dict(dirs=None), dict(range=None),
        dict(normals=None), dict(flag=None)])
    assert call(R=0, dirs=None, range=None, normals=None, flag=None) == 0 and call(F=0, poses=None) == 0      # no-ops
    assert call(lo=0.0, hi=6553.5, h=0.1, R=0) == 0                                                           # K = 65536 is taken


# ------------------------------------------------------------------------------------------------------------------- mutants
def test_every_mutant_differs_on_the_inputs_of_the_gpu_tests():
    """which input tells which mutant: the 7-corner cell across_gap, the layer of exact zeros sign_ge (a zero between a positive and a
    negative sample gives the same bytes under either rule; a ray that STARTS on a zero does not), the BACK rays back_as_hit, any
    HIT under a turned pose map_normal, the steps that are no binary fractions accumulate_t"""
    tells = {m: [] for m in MUTANTS}
    for name in ("poses3", "plane", "lattice", "seven", "zero", "far"):
        c = RC.cast_cases()[name]
        want = true_cast(name)
        for m in MUTANTS:
            if not same(want, RC.restated(c, exported(name), **{m: True})):
                tells[m].append(name)
    log(f"host raycast mutants told apart by: {tells}")
    assert all(tells[m] for m in MUTANTS), tells
    assert "seven" in tells["across_gap"] and "lattice" in tells["back_as_hit"] and "poses3" in tells["accumulate_t"]
    assert "zero" in tells["sign_ge"] and "poses3" in tells["map_normal"]


# -------------------------------------------------------------------------------------------------------------------- inputs
def test_the_constructed_cases_show_what_they_were_built_for():
    cases = RC.cast_cases()
    assert true_cast("between_miss")[2].tolist() == [[T.MISS]] and true_cast("between_hit")[2].tolist() == [[T.HIT]]
    assert abs(float(true_cast("between_hit")[0][0, 0]) - 7.375) < 0.05
    assert not true_cast("empty")[2].any() and not true_cast("one_sample")[2].any() and not true_cast("rays0")[2].size
    assert T.samples(4.0, 4.0, 0.1) == 1
    # the 7-corner cell: MISS under the rule, HIT when a crossing is accepted across the valueless samples; between the positive
    # and the negative valued sample lie four samples with exactly 7 of their 8 corners; one cell further, a HIT at 1.1 m
    c, want = cases["seven"], true_cast("seven")
    gap = RC.restated(c, exported("seven"), across_gap=True)
    assert want[2][0, 1] == T.MISS and gap[2][0, 1] == T.HIT and want[2][1, 1] == T.HIT and abs(float(want[0][1, 1]) - 1.1) < 1e-6
    t = (np.arange(T.samples(c.lo, c.hi, c.step)) * F32(c.step)).astype(F32)
    s = RR.sample(R.field(exported("seven")), c.map.voxel, c.dirs[1][None, :] * t[:, None], c.poses[0], c.map.origin, F32)
    assert s.corners.tolist() == [8, 8, 8, 8, 7, 7, 7, 7, 8, 8, 4] and (s.d[:4] > 0).all() and (s.d[8:10] < 0).all()
    # the lattice: BACK from inside the negative band and from behind the wall, MISS looking away from behind it, HIT from in front
    flag = true_cast("lattice")[2]
    assert flag[5, 0] == T.BACK and flag[7, 0] == T.BACK and flag[7, 1] == T.MISS and (flag[:5, 1] == T.HIT).all()
    assert (flag[:, 6:] == T.MISS).all()                                     # the zero and the NaN direction
    assert (flag[:5, 2:6] == T.MISS).all()                                   # along the wall, in front of it: nothing there
    rng, _, flag = true_cast("zero")                                         # starts ON the zero: no crossing; the zero at 2 m: a HIT there
    assert flag[0, 1] == T.MISS and flag[1, 1] == T.HIT and rng[1, 1] == F32(2.0) and flag[0, 0] == T.BACK
    out = true_cast("outside")[2]
    assert (out == T.MISS).sum() > 0
    for name in ("poses3", "plane", "far", "poses3_min2", "plane_min2"):
        f = true_cast(name)[2]
        log(f"host raycast {name}: HIT {int((f == 1).sum())}, BACK {int((f == 2).sum())}, MISS {int((f == 0).sum())} of {f.size}")
        assert (f == T.HIT).mean() > 0.3 and (f == T.MISS).sum() > 0
        assert (f[:, [5, 9, 11]] == T.MISS).all()


# ------------------------------------------------------------------------------------------------------------------- float64
@pytest.mark.parametrize("name", ["poses3", "plane", "far", "poses3_min2"])
def test_float32_agrees_with_the_independent_float64_form(name):
    c = RC.cast_cases()[name]
    differ, dr, dn, share = T.compare(true_cast(name), RC.restated(c, exported(name), np.float64))
    log(f"host raycast {name}: float32 against float64: {differ} flags differ, range within {dr:.3e} m (bound {RANGE_BOUND:.0e}), "
        f"normal within {dn:.3e}, ambiguous share {share:.4f} (cap {AMBIGUOUS_CAP})")
    assert differ == 0 and dr <= RANGE_BOUND and share < AMBIGUOUS_CAP


# ------------------------------------------------------------------------------------------------------------------- answers
def tilted_report(what, tilt, cc, rng, flag):
    """the tilted plane's assertions, shared with the GPU test: rng, flag (R,)"""
    hit = flag == T.HIT
    err = np.abs(rng.astype(np.float64) - cc.analytic) * np.abs(cc.u_dot_n)
    log(f"{what} raycast tilted plane {tilt}: {int(hit.sum())} HIT of {len(flag)} rays ({int(cc.required.sum())} required), distance of the "
        f"HIT points from the plane at most {err[hit].max():.3e} m (bound {PLANE_BOUND:.0e})")
    assert cc.required.sum() > 100 and hit[cc.required].all(), (tilt, int((~hit & cc.required).sum()))
    assert err[hit].max() <= PLANE_BOUND, (tilt, err[hit].max())


@pytest.mark.parametrize("tilt", H.TILTS)
def test_tilted_plane_known_answer(tilt):
    cc = RC.tilted_cast(tilt)
    rng, _, flag = RC.restated(cc, H.fuse_plane(cc.map).export())
    tilted_report("host", tilt, cc, rng[0], flag[0])


@functools.lru_cache(maxsize=None)
def sphere_yardstick(which):
    """-> (the cast case, cast32's result, cast64's result, the float64 form's own worst range and normal error against the
    analytic sphere) on the float32 restatement's table"""
    cc = RC.sphere_cast(RC.SPHERE_STARTS[which])
    exp = RC.fuse_restated(cc).export()
    c32, c64 = RC.restated(cc, exp), RC.restated(cc, exp, np.float64)
    ended = c64.flag[0] == T.HIT
    e_r = float(np.abs(c64.range[0] - cc.analytic)[ended].max())
    e_n = float(np.abs(c64.normals[0] - cc.analytic_normals)[ended].max())
    return cc, c32, c64, e_r, e_n


def sphere_report(what, which, rng, nrm, flag):
    """the sphere's assertions, shared with the GPU test: rng (R,), nrm (R,3), flag (R,) of the form under test.  Against the
    analytic sphere it may be twice as far off as the float64 form is; from the float64 form it stays within max(3 |r32 - r64|,
    1e-4 m) (normals: 1e-4), r32 the float32 restatement."""
    cc, c32, c64, e_r, e_n = sphere_yardstick(which)
    miss = float((flag != T.HIT).mean())
    hit = (flag == T.HIT) & (c64.flag[0] == T.HIT)
    r, n = rng.astype(np.float64), nrm.astype(np.float64)
    err_r, err_n = np.abs(r - cc.analytic)[hit].max(), np.abs(n - cc.analytic_normals)[hit].max()
    d32r = np.abs(c32[0][0].astype(np.float64) - c64.range[0])
    d32n = np.abs(c32[1][0].astype(np.float64) - c64.normals[0]).max(axis=1)
    dr, dn = np.abs(r - c64.range[0]), np.abs(n - c64.normals[0]).max(axis=1)
    log(f"{what} raycast sphere from {RC.SPHERE_STARTS[which]}: not HIT {miss:.4f} of {len(flag)} rays (cap {MISS_CAP}); range off the "
        f"sphere by at most {err_r * 1e3:.2f} mm (float64 form {e_r * 1e3:.2f} mm, bound twice that), normal by {err_n:.3e} (float64 "
        f"form {e_n:.3e}); from the float64 form: range {dr[hit].max():.3e} m, normal {dn[hit].max():.3e}")
    assert miss <= MISS_CAP
    assert err_r <= 2 * e_r and err_n <= 2 * e_n
    assert (dr[hit] <= np.maximum(3 * d32r[hit], 1e-4)).all() and (dn[hit] <= np.maximum(3 * d32n[hit], 1e-4)).all()


@pytest.mark.parametrize("which", [0, 1])
def test_sphere_known_answer(which):
    cc, c32, c64, e_r, e_n = sphere_yardstick(which)
    assert float((c64.flag[0] != T.HIT).mean()) <= MISS_CAP               # the restatement alone stays within the share
    sphere_report("host", which, c32[0][0], c32[1][0], c32[2][0])


def walls_seen_report(what, cc, before, after):
    """(range, flag) (R,) before and after the carve: the front wall, then the wall behind it; the plane form's field is linear
    in the band of one plane, so the bar is the tilted plane's"""
    c = cc.map
    x0 = c.frames[0][2][0, 3]
    for (rng, flag), wall, when in ((before, c.walls[0], "before"), (after, c.walls[1], "after")):
        err = np.abs(rng.astype(np.float64) * cc.ux - (wall - x0))
        log(f"{what} raycast wall seen through, {when} the carve: {int((flag == T.HIT).sum())} HIT of {len(flag)}, x of the hit within "
            f"{err.max():.3e} m of the wall at {wall - x0:g} m (bound {PLANE_BOUND:.0e})")
        assert (flag == T.HIT).all() and err.max() <= PLANE_BOUND, (when, flag.tolist(), err.max())


def test_wall_seen_through_known_answer():
    cc = RC.walls_cast()
    m = H.fuse_plane(cc.map)
    before = RC.restated(cc, m.export())
    PR.carve(m, *valid(cc.map.frames[1]), 512, cc.map.truncation + cc.map.voxel)
    after = RC.restated(cc, m.export())
    walls_seen_report("host", cc, (before[0][0], before[2][0]), (after[0][0], after[2][0]))


def patches_poses(c):
    """the three patches (origin at the world's zero) -> (a rendering pose that did not fuse them, the start 0.35 m / 2 degrees off it)"""
    pose = I.perturbed(c.pose, seed=3, trans=0.2, deg=3.0)
    return pose, I.perturbed(pose, seed=4, trans=0.35, deg=2.0)


def test_three_patches_render_then_register_known_answer():
    c = RR.patches_case()
    model = RC.render_model()
    pose, start = patches_poses(c)
    fld = R.field(RR.fuse_case(c).export(), PR.WEIGHT_ONE // 256)
    rng, _, flag = T.cast32(fld, c.voxel, c.origin, pose[None], model.directions(), model.min_range, model.max_range, c.voxel / 2)
    hit = flag[0] == T.HIT
    xyz = (model.directions() * rng[0][:, None])[hit]
    r = RR.register(fld, c.voxel, xyz, c.origin, start, ((3 * c.voxel, 30),), dtype=F32)
    dt, dr = RR.pose_error(r["pose"], pose)
    log(f"host raycast three patches: {int(hit.sum())} HIT of {hit.size} rendered rays; registered from 0.35 m / 2 degrees off: status "
        f"{r['status']}, {r['iterations']} iterations, back to the rendering pose within {dt:.3e} m and {dr:.3e} (bounds 1e-4)")
    assert hit.sum() > 300 and r["status"] == RR.CONVERGED and dt <= 1e-4 and dr <= 1e-4
