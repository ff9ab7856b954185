"""CPU: the plane-distance fusion and the free-space carving of the TSDF map: their restatement (tests/tsdf_plane_restated.py),
the inputs of tests/test_gpu_tsdf_plane.py (built here from tests/tsdf_cases.py, with normals) and the host side of
deeppointmap_amd/tsdf.py.

  mutants     no orientation flip, the weight not applied to the sum, u instead of m, a carve that claims slots: each changes
              the table on the inputs the GPU tests use.
  float64     the float32 field lies within 1 mm of the independent float64 field on the unambiguous voxels, after fusion and
              after a carve, also 1 km from the world's zero; the ambiguous share of every input used for that stays under 1 %,
              found with the float64 form alone.
  slanted     known answer: one plane 6 m from an off-lattice sensor, exact normals, tilted by 0, 0.5, 1.0 and 1.2 rad: every
              surface record within 1e-4 m of the plane (a plane's distance field is linear, so interpolating its crossing is
              exact and only rounding is left); the same input through the along-ray form is more than 10 mm off on average.
  carve       known answer: a wall at 5 m, then a wall at 10 m seen through where it stood; carving with the second frame at
              weight 2 leaves no surface record of the first wall in front of the sensor, the second wall's records keep their
              bytes and the key set its size.
  refusals    TsdfMap and the C entry points refuse bad arguments before any HIP call.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_cases as C  # noqa: E402
import tsdf_plane_restated as PR  # noqa: E402
import tsdf_restated as R  # noqa: E402
from test_tsdf_host import CAP, FIELD_BOUND, log, same, valid  # noqa: E402

F32 = np.float32
PLANE_BOUND = 1e-4       # metres: the slanted plane's surface records (observed 2.1e-6)
RAY_FLOOR = 10e-3        # metres: the along-ray form's mean error on the same input (observed 36 to 43 mm)
TILTS = (0.0, 0.5, 1.0, 1.2)


# --------------------------------------------------------------------------------------------------------------------- inputs
def unit_normals(n, seed):
    """random unit normals of either orientation, float32"""
    g = np.random.default_rng(seed).normal(size=(n, 3))
    return (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(F32)


def with_normals(c, seed=0, spoil=()):
    """a case of tsdf_cases with c.normals = one (cap,3) array per frame; spoil: rows of the first frame that get a NaN and a
    zero normal in turn"""
    c.normals = [unit_normals(len(f[0]), 7919 * seed + i) for i, f in enumerate(c.frames)]
    for j, row in enumerate(spoil):
        c.normals[0][row] = np.nan if j % 2 == 0 else 0.0
    c.cos_min = 0.0
    return c


def counted():
    """count < cap: NaN rows and NaN / zero normals below the count, valid rows with valid normals past it"""
    return with_normals(C.counted(), 1, spoil=(5, 6, 120, 198))


def wall():
    """tsdf_cases.wall with the wall's own normal (pointing away from the sensors), so that cells have their 8 corners"""
    c = C.wall()
    n_w = np.array([1.0, -0.3, 0.2]) / np.linalg.norm([1.0, -0.3, 0.2])
    c.normals = [np.tile((pose[:3, :3].T @ n_w).astype(F32), (len(xyz), 1)) for xyz, _, pose in c.frames]
    c.cos_min = 0.0
    return c


def cos_met(cos_min=0.5):
    """an exact pose and returns on the x axis, so that u = (1, 0, 0) exactly and a = |n_x|: 0.5 meets cos_min = 0.5 exactly,
    the float below it does not; from the other side the same; a normal with a = 0 and one with 256 a = 0.5 (rounds to 0)"""
    below = np.nextafter(F32(0.5), F32(0))
    nx = np.array([0.5, below, -0.5, -below, 0.0, 0.5 / 256, 1.0, 1.5 / 256], F32)
    normals = np.stack([nx, np.sqrt(1 - nx.astype(np.float64) ** 2).astype(F32), np.zeros(len(nx), F32)], axis=1)
    xyz = np.stack([np.arange(len(nx)) * 0.75 + 2.0, np.zeros(len(nx)), np.zeros(len(nx))], axis=1).astype(F32)
    c = C._case([(xyz, len(xyz), np.eye(4))])
    c.normals, c.cos_min = [normals], cos_min
    return c


def plane_cases():
    out = {f"cap{cap}": with_normals(C.general(cap), cap) for cap in C.CAPS}
    out.update(counted=counted(), two_frames=with_normals(C.two_frames(), 4), wall=wall(), cos_met=cos_met(),
               short=with_normals(C.short(), 5), outside=with_normals(C.outside(), 6))
    return out


def list_case(F, P):
    """tsdf_cases.list_case with a normals store (capacity,P,3): NaN and zero normals among them"""
    c = C.list_case(F, P)
    cap = c.store.shape[0]
    c.normal_store = unit_normals(cap * P, 31 * F + P).reshape(cap, P, 3)
    for r in range(cap):
        c.normal_store[r, (r + 2) % P] = np.nan if r % 2 else 0.0
    c.normals = [np.ascontiguousarray(c.normal_store[r, :len(f[0])]) for f, r in
                 zip(c.frames, [r for r in c.rows if 0 <= r < cap])]
    c.cos_min = 0.0
    return c


def fuse_plane(c, order=None, rows=None, sign=1.0, **mutant):
    m = PR.FusedPlane(c.voxel, c.origin, c.truncation, c.step, c.min_range, c.max_range, cos_min=c.cos_min, **mutant)
    for f in (range(len(c.frames)) if order is None else order):
        xyz, _ = valid(c.frames[f])
        nrm = c.normals[f][:len(xyz)] * F32(sign)
        m.integrate(xyz if rows is None else xyz[rows], c.frames[f][2], nrm if rows is None else nrm[rows])
    return m


def fuse_plane64(c):
    m = PR.Fused64(c.voxel, c.origin, c.truncation, c.step, c.min_range, c.max_range, c.cos_min)
    for f, nrm in zip(c.frames, c.normals):
        xyz, pose = valid(f)
        m.integrate(xyz, pose, nrm[:len(xyz)])
    return m


def carve_all(m, c, weight, margin=None, **kw):
    """every frame of the case carved into m; margin None: truncation + voxel, TsdfMap's default"""
    for f in c.frames:
        xyz, pose = valid(f)
        PR.carve(m, xyz, pose, weight, c.truncation + c.voxel if margin is None else margin, **kw)
    return m


# ----------------------------------------------------------------------------------------------------- the two known answers
def slanted(tilt):
    """one plane with normal (cos tilt, 0, sin tilt), 6 m from the world's zero, seen by 256 x 48 rays from an off-lattice
    sensor: the rays that meet it within 40 m.  voxel 0.25, truncation 0.75, step 0.125; exact normals"""
    n_w = np.array([np.cos(tilt), 0.0, np.sin(tilt)])
    az = np.linspace(-np.pi, np.pi, 256, endpoint=False) + 0.0123
    el = np.linspace(-0.4, 0.4, 48) + 0.0031
    A, E = np.meshgrid(az, el)
    dirs = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)
    den = dirs @ n_w
    hit = den > 1e-3
    t = 6.0 / den[hit]
    xyz = (dirs[hit] * t[:, None])[t < 40.0].astype(F32)
    pose = np.eye(4)
    pose[:3, 3] = [0.013, 0.021, 0.007]
    c = C._case([(xyz, len(xyz), pose)], voxel=0.25, truncation=0.75, step=0.125, min_range=0.0, max_range=100.0, cap_vox=1 << 17)
    c.normals, c.cos_min = [np.tile(n_w.astype(F32), (len(xyz), 1))], 0.0
    c.plane = (n_w, 6.0 + n_w @ pose[:3, 3])          # n . x = d in world coordinates (the origin is the world's zero)
    return c


def plane_errors(c, xyz_map):
    """distances of surface positions (M,3) in the map frame from the case's plane"""
    n_w, d = c.plane
    return np.abs((np.asarray(xyz_map, np.float64) + c.origin) @ n_w - d)


def slanted_report(what, tilt, c, plane_xyz, ray_xyz):
    """the slanted plane's assertions, shared with the GPU test"""
    ep, er = plane_errors(c, plane_xyz), plane_errors(c, ray_xyz)
    log(f"{what} slanted plane tilt {tilt}: {len(c.frames[0][0])} rays; plane distance: {len(ep)} records, max {ep.max():.3e} m, mean "
        f"{ep.mean():.3e} m (bound {PLANE_BOUND:.0e}); along-ray: {len(er)} records, mean {er.mean() * 1e3:.1f} mm, max "
        f"{er.max() * 1e3:.1f} mm (floor of the mean {RAY_FLOOR * 1e3:.0f} mm)")
    assert len(ep) > 500 and ep.max() <= PLANE_BOUND, (tilt, len(ep), ep.max())
    assert er.mean() > RAY_FLOOR, (tilt, er.mean())


def two_walls():
    """a wall at x = 5 m (frame 0), then a wall at x = 10 m seen through where it stood (frame 1): 96 x 48 rays within +-0.4
    rad from an off-lattice sensor, voxel 0.25, exact normals"""
    a = np.linspace(-0.4, 0.4, 96) + 0.0011
    e = np.linspace(-0.4, 0.4, 48) + 0.0007
    A, E = np.meshgrid(a, e)
    dirs = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)
    pose = np.eye(4)
    pose[:3, 3] = [0.013, 0.021, 0.007]
    frames = [((dirs * (x / dirs[:, :1])).astype(F32), len(dirs), pose) for x in (5.0, 10.0)]
    c = C._case(frames, voxel=0.25, truncation=0.75, step=0.125, min_range=0.0, max_range=100.0, cap_vox=1 << 17)
    c.normals, c.cos_min = [np.tile(np.array([-1, 0, 0], F32), (len(dirs), 1))] * 2, 0.0
    c.walls = (5.0 + pose[0, 3], 10.0 + pose[0, 3])     # world x of the two walls
    return c


def walls_report(what, c, before, after, keys_before, keys_after):
    """before / after: surface records (keys, axes, xyz (M,3) map frame, normals) round a carve with frame 1 at weight 2"""
    def near(s, wall):
        x = s[2].astype(np.float64) + c.origin
        return np.abs(x[:, 0] - wall) < 1.0, (np.abs(x[:, 1]) < 1.5) & (np.abs(x[:, 2]) < 1.5)
    (a0, mid0), (a1, mid1) = near(before, c.walls[0]), near(after, c.walls[0])
    b0, b1 = near(before, c.walls[1])[0], near(after, c.walls[1])[0]
    log(f"{what} carve: records of the wall at 5 m in front of the sensor {int((a0 & mid0).sum())} -> {int((a1 & mid1).sum())} "
        f"(anywhere {int(a0.sum())} -> {int(a1.sum())}); of the wall at 10 m {int(b0.sum())} -> {int(b1.sum())}; keys {keys_before} -> {keys_after}")
    assert (a0 & mid0).sum() > 100 and (a1 & mid1).sum() == 0
    assert b0.sum() > 100 and all(x[b0].tobytes() == y[b1].tobytes() for x, y in zip(before, after))
    assert keys_before == keys_after


def surface_of(m, voxel, min_count):
    return R.surface(R.field(m.export(), min_count), voxel)


@pytest.mark.parametrize("tilt", TILTS)
def test_slanted_plane_known_answer(tilt):
    c = slanted(tilt)
    plane = surface_of(fuse_plane(c), c.voxel, 1)                  # every voxel that holds a sample, whatever its weight
    ray = R.Fused(c.voxel, c.origin, c.truncation, c.step, c.min_range, c.max_range).integrate(*valid(c.frames[0]))
    slanted_report("host", tilt, c, plane[2], surface_of(ray, c.voxel, 1)[2])


def test_carve_known_answer():
    c = two_walls()
    m = fuse_plane(c)
    before, n0 = surface_of(m, c.voxel, PR.WEIGHT_ONE), len(m.sum)
    one = carve_all(fuse_plane(c), SimpleNamespace(frames=c.frames[1:], truncation=c.truncation, voxel=c.voxel), PR.WEIGHT_ONE)
    left = surface_of(one, c.voxel, PR.WEIGHT_ONE)
    x = left[2].astype(np.float64) + c.origin
    log(f"host carve at weight 1: {int(((np.abs(x[:, 0] - c.walls[0]) < 1.0) & (np.abs(x[:, 1]) < 1.5) & (np.abs(x[:, 2]) < 1.5)).sum())} "
        "records of the wall at 5 m remain in front of the sensor (why weight 2 is the test)")
    PR.carve(m, *valid(c.frames[1]), 2 * PR.WEIGHT_ONE, c.truncation + c.voxel)
    walls_report("host", c, before, surface_of(m, c.voxel, PR.WEIGHT_ONE), n0, len(m.sum))


# -------------------------------------------------------------------------------------------------------------------- mutants
def gpu_inputs():
    cases = plane_cases()
    cases.update({f"list{F}x{P}": list_case(F, P) for F, P in C.LIST_SHAPES if F})
    return cases


def test_the_gpu_cases_can_tell_the_mutants_from_the_true_form():
    cases = gpu_inputs()
    for name, mutant in (("no orientation flip", dict(flip=False)), ("the weight not applied to the sum", dict(weigh_sum=False)),
                         ("u instead of m", dict(use_m=False))):
        differs = [k for k, c in cases.items() if not same(fuse_plane(c, **mutant), fuse_plane(c))]
        log(f"host plane mutant '{name}': differs from the true form on {len(differs)} of {len(cases)} input sets")
        assert {"cap257", "two_frames", "counted", "list17x257"} <= set(differs), (name, differs)
    assert not same(fuse_plane(cases["wall"], weigh_sum=False), fuse_plane(cases["wall"]))
    differs = [k for k in ("two_frames", "wall", "cap257") if not same(carve_all(fuse_plane(cases[k]), cases[k], 256, claims=True),
                                                                       carve_all(fuse_plane(cases[k]), cases[k], 256))]
    log(f"host carve mutant 'claims slots': differs on {differs}")
    assert differs == ["two_frames", "wall", "cap257"]
    for k in ("two_frames", "wall"):                                   # and the true carve does reach voxels the map holds
        assert not same(carve_all(fuse_plane(cases[k]), cases[k], 256), fuse_plane(cases[k])), k


def test_the_constructed_cases_hold_what_they_are_for():
    cases = plane_cases()
    m = fuse_plane(cases["cos_met"])
    # rows 0 and 2 (a = 0.5, either side) and row 6 (a = 1) pass cos_min = 0.5; the float below, a = 0, 256 a = 0.5 and 1.5 do not
    assert m.unusable == 5 and set(m.count.values()) <= {128, 256, 384} and len(m.sum) > 0
    loose = cos_met(0.0)
    assert fuse_plane(loose).unusable == 2                            # a = 0 and 256 a = 0.5, which rounds to even: 0
    # the four spoiled normals on top of the random ones with 256 a < 0.5; NaN rows fail the range gate first
    assert fuse_plane(cases["counted"]).unusable == fuse_plane(with_normals(C.counted(), 1)).unusable + 4
    assert same(fuse_plane(cases["two_frames"], sign=-1.0), fuse_plane(cases["two_frames"]))
    assert fuse_plane(cases["short"]).unusable >= 1                   # the return at range 0 has no direction
    assert fuse_plane(cases["outside"]).outside > 0
    assert len(fuse_plane(cases["cap0"]).sum) == 0 and len(fuse_plane(cases["cap1"]).sum) > 0


def test_the_table_is_the_same_for_permuted_rows_frames_in_any_order_and_carves_in_any_order():
    c = plane_cases()["two_frames"]
    want = fuse_plane(c)
    assert same(fuse_plane(c, order=[1, 0]), want)
    one = plane_cases()["cap257"]
    assert same(fuse_plane(one, rows=np.random.default_rng(0).permutation(257)), fuse_plane(one))
    a = carve_all(fuse_plane(c), c, 256)
    b = carve_all(fuse_plane(c), SimpleNamespace(frames=c.frames[::-1], truncation=c.truncation, voxel=c.voxel), 256)
    assert same(a, b) and same(carve_all(carve_all(fuse_plane(c), c, 256), c, 256), carve_all(fuse_plane(c), c, 512))
    lst = list_case(17, 257)
    by_list = PR.FusedPlane(lst.voxel, lst.origin, lst.truncation, lst.step, lst.min_range, lst.max_range)
    by_list.integrate_frames(lst.store, lst.lengths, lst.rows, lst.poses, lst.normal_store)
    assert same(by_list, fuse_plane(lst)) and by_list.unusable == fuse_plane(lst).unusable > 0


# -------------------------------------------------------------------------------------------------------------------- float64
def moved(c, far):
    """the case with its poses and the map's origin moved by `far`"""
    c.origin = np.asarray(far, np.float64)
    c.frames = [(x, n, np.vstack([np.hstack([p[:3, :3], (p[:3, 3] + far)[:, None]]), [0, 0, 0, 1]])) for x, n, p in c.frames]
    return c


@pytest.mark.parametrize("name", ["cap257", "two_frames", "counted", "list17x257", "two_frames_far", "two_frames_carved",
                                  "two_frames_far_carved", "ray_two_frames_carved"])
def test_float32_field_against_float64_and_the_ambiguity_cap(name):
    """The inputs are the sparse ones, a few rows a voxel at most: a row in a thousand has 256 a within 5e-4 of a half-integer and
    makes every voxel it touches ambiguous, so a dense input cannot stay under the cap whatever the kernel does -- the float64
    form alone calls 1.84 % of the dense wall's voxels ambiguous, which is why the wall is not among them (it is compared byte for
    byte with the float32 form, where the rounding of a weight is exact).  Observed: max |dD| 9.1e-7 m, shares up to 0.49 %."""
    far = np.array([1000.0, -1000.0, 1000.0])
    base = name.replace("_carved", "").replace("_far", "").replace("ray_", "")
    c = list_case(17, 257) if base == "list17x257" else plane_cases()[base]
    if "_far" in name:
        c = moved(c, far)
    if name.startswith("ray_"):
        m32 = R.Fused(c.voxel, c.origin, c.truncation, c.step, c.min_range, c.max_range)
        m64 = PR.Fused64(c.voxel, c.origin, c.truncation, c.step, c.min_range, c.max_range)
        for f in c.frames:
            m32.integrate(*valid(f)), m64.integrate_ray(*valid(f))
        weight = 1
    else:
        m32, m64, weight = fuse_plane(c), fuse_plane64(c), 256
    if "_carved" in name:
        carve_all(m32, c, weight)
        for f in c.frames:
            m64.carve(*valid(f), weight, c.truncation + c.voxel)
    err, lonely, share = R.compare_fields(R.field(m32.export()), m64.result())
    log(f"host plane {name}: float32 field against float64 on unambiguous voxels: max |dD| {err:.3e} m (bound {FIELD_BOUND:.0e}), "
        f"{lonely} voxels in one form only, ambiguous share {share:.4%} (cap {CAP:.0%})")
    assert share <= CAP, share
    assert lonely == 0 and err <= FIELD_BOUND, (err, lonely)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_tsdf_map_refuses_bad_plane_and_carve_arguments_before_any_hip_call():
    import torch
    from deeppointmap_amd.tsdf import TsdfMap
    assert (TsdfMap().distance, TsdfMap().unit, TsdfMap(distance="plane").unit) == ("ray", 1, 256)
    for kw in (dict(distance="normal"), dict(cos_min=-0.1), dict(cos_min=1.5), dict(cos_min=float("nan"))):
        with pytest.raises(ValueError):
            TsdfMap(**kw)
    ray, plane = TsdfMap(), TsdfMap(distance="plane", cos_min=0.2)
    xyz, store, lengths = torch.zeros(4, 3), torch.zeros(2, 3, 4), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="normals"):
        ray.integrate(xyz, np.eye(4), normals=torch.zeros(4, 3))
    with pytest.raises(ValueError, match="normals"):
        ray.integrate(xyz, np.eye(4), normals=1.0)
    with pytest.raises(ValueError, match="normals"):
        plane.integrate(xyz, np.eye(4))
    with pytest.raises(ValueError):
        plane.integrate(xyz, np.eye(4), normals=torch.zeros(3, 3))
    with pytest.raises(ValueError, match="normals"):
        plane.integrate_frames(store, lengths, [0], np.eye(4)[None])
    with pytest.raises(ValueError, match="normals"):
        ray.integrate_frames(store, lengths, [0], np.eye(4)[None], normals=torch.zeros(2, 4, 3))
    for kw in (dict(weight=0), dict(weight=-1.0), dict(weight=65536), dict(margin=-0.5), dict(margin=float("nan"))):
        with pytest.raises(ValueError):
            ray.carve(xyz, np.eye(4), **kw)
        with pytest.raises(ValueError):
            ray.carve_frames(store, lengths, [0], np.eye(4)[None], **kw)
    with pytest.raises(ValueError):
        plane.carve(xyz, np.eye(4), weight=256)                      # 256 full-weight samples are 65536 count units
    with pytest.raises(ValueError):
        ray.carve_frames(store, lengths, [2], np.eye(4)[None])
    with pytest.raises(ValueError, match="max_range / step"):
        TsdfMap(step=1e-3, truncation=0.6, max_range=100.0).carve(xyz, np.eye(4))
    assert ray.carve(xyz, np.eye(4)) is ray and ray.table is None     # an empty map: nothing to carve, nothing allocated
    assert plane._min_count(1) == 256 and plane._min_count(0.001) == 1 and ray._min_count(3) == 3 and plane._min_count(2.5) == 640
    for bad in (0, -1):
        for fn in (plane.field, plane.surface, plane.mesh):
            with pytest.raises(ValueError):
                fn(min_count=bad)
    assert plane.unusable() == 0 and plane.table is None


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    import ctypes
    from deeppointmap_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) & ~255   # never dereferenced: every call below is refused first, or is a no-op
    o = (ctypes.c_double * 3)(0, 0, 0)

    def refusals(fn, names, good, bad):
        call = lambda **k: fn(*[{**good, **k}[n] for n in names])
        for k in bad:
            assert call(**k) == -1, (fn.__name__, k)
        return call
    rays = dict(lo=0.0, hi=10.0, tau=0.6, h=0.1)
    bad_rays = [dict(lo=-1.0), dict(lo=11.0), dict(hi=float("inf")), dict(tau=0.0), dict(tau=64.0001), dict(h=0.0), dict(h=float("nan")),
                dict(tau=41.0, h=0.01)]
    bad_map = [dict(map=None), dict(map=p + 8), dict(cap_vox=65), dict(voxel=0.0), dict(origin=None)]
    bad_cos = [dict(cos=-1e-9), dict(cos=1.0001), dict(cos=float("nan"))]
    bad_carve = [dict(w=0), dict(w=-3), dict(w=65536), dict(margin=-1e-9), dict(margin=float("nan")), dict(margin=float("inf")),
                 dict(hi=10.0, h=1e-4), dict(hi=6553.7, h=0.1)]
    frame = dict(map=p, cap_vox=64, voxel=0.2, origin=ctypes.addressof(o), xyz=p, normals=p, count=p, cap=8, pose=p, stream=None,
                 cos=0.5, w=1, margin=0.8, **rays)
    lst = dict(map=p, cap_vox=64, voxel=0.2, origin=ctypes.addressof(o), store=p, normals=p, lengths=p, capacity=4, P=8, frames=p,
               poses=p, F=2, stream=None, cos=0.5, w=1, margin=0.8, **rays)
    bad_frame = [dict(xyz=None), dict(count=None), dict(pose=None), dict(cap=-1)]
    bad_list = [dict(store=None), dict(lengths=None), dict(frames=None), dict(poses=None), dict(capacity=0), dict(P=0), dict(F=-1),
                dict(F=65536)]
    call = refusals(lib.dpm_tsdf_integrate_planes, ("map", "cap_vox", "voxel", "origin", "xyz", "normals", "count", "cap", "pose", "lo",
                                                   "hi", "tau", "h", "cos", "stream"),
                    frame, bad_map + bad_rays + bad_cos + bad_frame + [dict(normals=None)])
    assert call(cap=0) == 0 and call(cap=0, cos=0.0) == 0 and call(cap=0, cos=1.0) == 0
    call = refusals(lib.dpm_tsdf_integrate_planes_frames,
                    ("map", "cap_vox", "voxel", "origin", "store", "normals", "lengths", "capacity", "P", "frames", "poses", "F", "lo", "hi",
                     "tau", "h", "cos", "stream"), lst, bad_map + bad_rays + bad_cos + bad_list + [dict(normals=None)])
    assert call(F=0, store=None, normals=None, lengths=None, frames=None, poses=None) == 0
    call = refusals(lib.dpm_tsdf_carve, ("map", "cap_vox", "voxel", "origin", "xyz", "count", "cap", "pose", "lo", "hi", "tau", "h", "w",
                                        "margin", "stream"), frame, bad_map + bad_rays + bad_carve + bad_frame)
    assert call(cap=0) == 0 and call(cap=0, w=65535, margin=0.0) == 0 and call(cap=0, hi=6553.6, h=0.1) == 0
    call = refusals(lib.dpm_tsdf_carve_frames, ("map", "cap_vox", "voxel", "origin", "store", "lengths", "capacity", "P", "frames", "poses",
                                               "F", "lo", "hi", "tau", "h", "w", "margin", "stream"),
                    lst, bad_map + bad_rays + bad_carve + bad_list)
    assert call(F=0, store=None, lengths=None, frames=None, poses=None) == 0


def test_surface_map_takes_distance_and_carve():
    from deeppointmap_amd.loop_closure import GeometricSlam
    slam = GeometricSlam(loop=dict(capacity=8, points_per_frame=8, metric="point"))
    m = slam.surface_map(0.5, distance="plane", carve=1.0, truncation=1.0, cos_min=0.1)
    assert (m.distance, m.unit, m.cos_min, m.table) == ("plane", 256, 0.1, None)
    assert slam.surface_map(0.5).distance == "ray"
    with pytest.raises(ValueError):
        slam.surface_map(0.5, carve=-1.0)
    with pytest.raises(ValueError):
        slam.surface_map(0.5, distance="other")
