"""CPU: the TSDF surface map's restatement (tests/tsdf_restated.py), the inputs of the GPU tests (tests/tsdf_cases.py) and the
host side of deeppointmap_amd/tsdf.py.

  order       the float32 table is identical for permuted rows and for frames in any order.
  float64     the float32 field lies within 1 mm (the project's geometric bound) of the independent float64
              field on the unambiguous voxels, also 1 km from the world's zero with the origin there; the ambiguous share of
              every input stays under 1 %, found with the float64 form alone.
  sphere      a sphere seen from its centre: every voxel whose centre lies within sqrt(3) v of it is present, every surface
              point and mesh vertex lies within 3 v^2 / (8 (rho - tau)) of it, the mesh is closed, consistently wound, has
              Euler characteristic 2 and its normals point to the sensor.
  mutants     omitting the skip of a repeated key, the clamp, or rounding to nearest changes the table on the GPU tests' inputs.
  refusals    TsdfMap and the C entry points refuse bad arguments before any HIP call.
  ply         write_ply round-trips through a small reader.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lidar_odometry_restated as L  # noqa: E402
import tsdf_cases as C  # noqa: E402
import tsdf_restated as R  # noqa: E402

from conftest import ROOT  # noqa: E402

CAP = 0.01          # the ambiguous share allowed (the simulator's cap): a condition on the inputs
FIELD_BOUND = 1e-3  # metres


def log(line):
    print(line)
    try:
        os.makedirs(os.path.join(ROOT, "test_logs"), exist_ok=True)
        with open(os.path.join(ROOT, "test_logs", "tsdf.log"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def valid(frame):
    xyz, count, pose = frame
    return (xyz if count is None else xyz[:count]), pose


def fuse(c, order=None, rows=None, **mutant):
    m = R.Fused(c.voxel, c.origin, c.truncation, c.step, c.min_range, c.max_range, **mutant)
    for f in (range(len(c.frames)) if order is None else order):
        xyz, pose = valid(c.frames[f])
        m.integrate(xyz if rows is None else xyz[rows], pose)
    return m


def fuse64(c):
    return R.fused64([valid(f) for f in c.frames], c.voxel, c.origin, c.truncation, c.step, c.min_range, c.max_range)


def same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a.export(), b.export()))


@pytest.fixture(scope="module")
def sphere():
    c = C.sphere()
    m = fuse(c)
    return c, m, R.field(m.export())


# ---------------------------------------------------------------------------------------------------------------------- order
def test_the_table_is_the_same_for_permuted_rows_and_frames_in_any_order():
    c = C.two_frames()
    want = fuse(c)
    assert len(want.sum) > 1000
    assert same(fuse(c, order=[1, 0]), want)
    one = C.general(257)
    assert same(fuse(one, rows=np.random.default_rng(0).permutation(257)), fuse(one))
    lst = C.list_case(17, 257)
    by_list = R.Fused(lst.voxel, lst.origin, lst.truncation, lst.step, lst.min_range, lst.max_range)
    by_list.integrate_frames(lst.store, lst.lengths, lst.rows, lst.poses)
    assert same(by_list, fuse(lst)) and same(by_list, fuse(lst, order=range(len(lst.frames) - 1, -1, -1)))
    assert len(lst.frames) == 16                       # one entry names a row outside the store


# -------------------------------------------------------------------------------------------------------------------- float64
def field_case(name, c):
    err, lonely, share = R.compare_fields(R.field(fuse(c).export()), fuse64(c))
    log(f"host {name}: float32 field against float64 on unambiguous voxels: max |dD| {err:.3e} m (bound {FIELD_BOUND:.0e}), "
        f"{lonely} voxels in one form only, ambiguous share {share:.4%} (cap {CAP:.0%})")
    return err, lonely, share


@pytest.mark.parametrize("name", ["cap257", "two_frames", "counted", "wall", "list17x257", "sphere", "sphere_far", "general_far"])
def test_float32_field_against_float64_and_the_ambiguity_cap(name):
    far = np.array([1000.0, -1000.0, 1000.0])
    if name == "sphere":
        c = C.sphere()
    elif name == "sphere_far":
        c = C.sphere(far)
    elif name == "general_far":
        c = C.two_frames()
        c.origin = far
        c.frames = [(x, n, np.vstack([np.hstack([p[:3, :3], (p[:3, 3] + far)[:, None]]), [0, 0, 0, 1]])) for x, n, p in c.frames]
    elif name == "list17x257":
        c = C.list_case(17, 257)
    else:
        c = C.single_frame_cases()[name]
    err, lonely, share = field_case(name, c)
    assert share <= CAP, share
    assert lonely == 0 and err <= FIELD_BOUND, (err, lonely)


def test_constructed_cases_are_ambiguous_on_purpose():
    """lattice points and axis rays sit ON voxel faces, and the short returns' ranges are multiples of the step, so that a sample
    has t = 0 exactly: the float64 form calls many of their voxels ambiguous, and they are checked against the float32 form
    only -- where these decisions are exact"""
    for name in ("lattice", "face_rays", "short"):
        share = R.compare_fields(R.field(fuse(C.single_frame_cases()[name]).export()), fuse64(C.single_frame_cases()[name]))[2]
        assert share > CAP, (name, share)


# --------------------------------------------------------------------------------------------------------------------- sphere
def sphere_report(what, c, fld, surf, vertices, faces):
    """the sphere's assertions, shared with the GPU test -> the log line"""
    s = C.SPHERE
    keys, D = fld
    centre = c.frames[0][2][:3, 3] - c.origin          # of the sphere (the sensor), in the map frame
    # completeness: every lattice voxel whose centre lies within sqrt(3) v of the sphere
    lim = int(np.ceil((s.rho + 2 * s.voxel) / s.voxel)) + 1
    g = np.stack(np.meshgrid(*[np.arange(-lim, lim)] * 3, indexing="ij"), -1).reshape(-1, 3)
    d = np.abs(np.linalg.norm((g + 0.5) * s.voxel - centre, axis=1) - s.rho)
    need = L.pack_key(g[d <= np.sqrt(3) * s.voxel])
    missing = int((~np.isin(need, keys)).sum())
    e_surf = np.abs(np.linalg.norm(surf[2].astype(np.float64) - centre, axis=1) - s.rho)
    e_mesh = np.abs(np.linalg.norm(vertices.astype(np.float64) - centre, axis=1) - s.rho)
    topo = R.topology(faces)
    volume = R.signed_volume(vertices.astype(np.float64) - centre, faces)
    nrm = surf[3].astype(np.float64)
    inward = -(surf[2].astype(np.float64) - centre) / np.linalg.norm(surf[2].astype(np.float64) - centre, axis=1, keepdims=True)
    cosine = (nrm * inward).sum(axis=1)
    log(f"{what} sphere rho {s.rho} v {s.voxel} tau {s.truncation}: {len(keys)} voxels, {len(need)} needed, {missing} missing; "
        f"{len(e_surf)} crossings max {e_surf.max() * 1e3:.2f} mm mean {e_surf.mean() * 1e3:.2f} mm; {topo['V']} vertices max "
        f"{e_mesh.max() * 1e3:.2f} mm (bound {s.bound * 1e3:.2f} mm); E {topo['E']} F {topo['F']} euler {topo['euler']} closed "
        f"{topo['closed']} oriented {topo['oriented']}; volume {volume:.3f} (sphere {-4 / 3 * np.pi * s.rho ** 3:.3f}); normals . inward "
        f"min {cosine.min():.4f}")
    assert missing == 0
    assert len(e_surf) > 1000 and e_surf.max() <= s.bound and e_mesh.max() <= s.bound
    assert topo["closed"] and topo["oriented"] and topo["euler"] == 2
    # Free space is inside: the faces' normals point to the centre, so the volume comes out NEGATIVE.  Its size: the vertices lie
    # within `bound` (10.4 mm) of the sphere and a chord of at most sqrt(3) v sags by 3 v^2 / (8 rho) = 7.8 mm, so the mesh lies
    # within 18.2 mm of it: 3 x 18.2 mm / rho = 1.8 % of the volume; 3 % is asserted.
    assert abs(volume + 4 / 3 * np.pi * s.rho ** 3) < 0.03 * 4 / 3 * np.pi * s.rho ** 3
    # The normals point to free space, the centre.  What is checked is the direction, not an accuracy: a field 10.4 mm wrong at
    # both ends of a difference over 2 v turns the gradient by 0.04 rad at most, far from the 0.45 rad that cos > 0.9 allows.
    assert cosine.min() > 0.9


def test_sphere_seen_from_its_centre(sphere):
    """Known answer.  The bound 3 v^2 / (8 (rho - tau)), 10.4 mm: s is the distance along the ray, from a centre up to
    sqrt(3)/2 v off that ray; the true distance to the sphere differs from it by d^2 / (2 R) at most, R >= rho - tau the
    distance from the sensor, d <= sqrt(3)/2 v.  Logged to test_logs/tsdf.log; a float64 prototype gave 3.2 mm."""
    from deeppointmap_amd import tsdf
    c, m, fld = sphere
    assert np.array_equal(fld[1], tsdf.field_values(m.export()[1], m.export()[2]))
    surf = R.surface(fld, c.voxel)
    vertices, faces = tsdf.weld(*R.mesh(fld, c.voxel))
    sphere_report("host", c, fld, surf, vertices, faces)


def test_min_count_leaves_thin_voxels_out(sphere):
    c, m, _ = sphere
    keys, sums, counts = m.export()
    assert counts.max() > counts.min()
    some = R.field((keys, sums, counts), min_count=int(np.median(counts)) + 1)
    assert 0 < len(some[0]) < len(keys)
    assert len(R.surface(some, c.voxel)[0]) <= len(R.surface(R.field(m.export()), c.voxel)[0])


# -------------------------------------------------------------------------------------------------------------------- mutants
def test_the_gpu_cases_can_tell_the_mutants_from_the_true_form():
    cases = C.single_frame_cases()
    cases.update({f"list{F}x{P}": C.list_case(F, P) for F, P in C.LIST_SHAPES if F})
    cases["sphere"] = C.sphere()
    for name, mutant in (("no skip of a repeated key", dict(skip=False)), ("no clamp", dict(clamp=False)),
                         ("truncation instead of rintf", dict(rint=False))):
        differs = [k for k, c in cases.items() if not same(fuse(c, **mutant), fuse(c))]
        log(f"host mutant '{name}': differs from the true form on {len(differs)} of {len(cases)} input sets")
        assert {"cap257", "two_frames", "wall", "list17x257", "sphere"} <= set(differs), (name, differs)


def test_the_constructed_cases_hold_what_they_are_for():
    cases = C.single_frame_cases()
    assert fuse(cases["outside"]).outside > 0 and len(fuse(cases["outside"]).sum) > 0
    short = fuse(cases["short"])
    assert short.outside > 0                                   # the return at range 0
    one = C._case([(np.array([[0.5, 0, 0]], np.float32), 1, np.eye(4))], min_range=0.0)
    assert R.steps(one.truncation, one.step) == 6 and sum(fuse(one, skip=False).count.values()) == 8    # t = 0.5 + 0.25 k > 0: k >= -1
    gates = C._case([(C.PLANTED, len(C.PLANTED), np.eye(4))])
    both = fuse(gates)
    only = C._case([(C.PLANTED[:2], 2, np.eye(4))])
    assert same(both, fuse(only)) and len(both.sum) > 0          # exactly the two rows ON the gates pass
    assert len(fuse(C.too_small()).sum) > C.too_small().cap_vox
    assert len(fuse(cases["cap0"]).sum) == 0 and len(fuse(cases["cap1"]).sum) > 0


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_tsdf_map_refuses_bad_arguments_before_any_hip_call():
    import torch
    from deeppointmap_amd.tsdf import TsdfMap
    m = TsdfMap()
    assert (m.voxel_size, m.truncation, m.step, m.max_voxels) == (0.2, 3 * 0.2, 0.1, 1 << 22)
    for kw in (dict(voxel_size=0.0), dict(voxel_size=-1.0), dict(max_voxels=1000), dict(max_voxels=1), dict(max_voxels=1 << 25),
               dict(truncation=0.0), dict(truncation=64.5), dict(step=0.0), dict(step=-0.1), dict(truncation=10.0, step=1e-3),
               dict(min_range=-1.0), dict(min_range=5.0, max_range=4.0), dict(voxel_size=float("nan"))):
        with pytest.raises(ValueError):
            TsdfMap(**kw)
    assert TsdfMap(truncation=64.0, step=1.0).truncation == 64.0
    for bad in (0, -1):
        for fn in (m.field, m.surface, m.mesh):
            with pytest.raises(ValueError):
                fn(min_count=bad)
    with pytest.raises(ValueError):
        m.integrate(torch.zeros(4, 2), np.eye(4))
    with pytest.raises(ValueError):
        m.integrate(torch.zeros(4, 3), np.eye(4), length=5)
    with pytest.raises(ValueError):
        m.integrate(torch.zeros(4, 3), np.eye(3))
    with pytest.raises(ValueError):
        m.integrate_frames(torch.zeros(2, 3, 4), torch.zeros(2, dtype=torch.int32), [2], np.eye(4)[None])
    with pytest.raises(ValueError):
        m.integrate_frames(torch.zeros(2, 3, 4), torch.zeros(2, dtype=torch.int32), [0, 1], np.eye(4)[None])
    assert m.table is None and m.overflow() == 0 and m.check() is m              # nothing was allocated
    assert [a.shape for a in m.export()] == [(0,), (0,), (0,)] and m.mesh()[1].shape == (0, 3)
    assert m.surface().xyz.shape == (3, 0)


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    import ctypes
    from deeppointmap_amd import _lib
    lib = _lib.load()
    assert [lib.dpm_tsdf_bytes(n) for n in (0, 1, 2, 3, 64, 1 << 24, 1 << 25, -4)] == [0, 0, 296, 0, 256 + 20 * 64, 256 + 20 * (1 << 24), 0, 0]
    assert not [n for n in _lib.SIGNATURES if n.startswith("dpm_tsdf") and n.endswith("_workspace_bytes")]
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) & ~255   # never dereferenced: every call below is refused first, or is a no-op
    o = (ctypes.c_double * 3)(0, 0, 0)
    bad_o = (ctypes.c_double * 3)(0, float("nan"), 0)

    def refusals(fn, names, good, bad):
        call = lambda **k: fn(*[{**good, **k}[n] for n in names])
        for k in bad:
            assert call(**k) == -1, (fn.__name__, k)
        return call
    rays = dict(lo=0.0, hi=10.0, tau=0.6, h=0.1)
    bad_rays = [dict(lo=-1.0), dict(lo=11.0), dict(hi=float("inf")), dict(tau=0.0), dict(tau=-1.0), dict(tau=64.0001),
                dict(tau=float("nan")), dict(h=0.0), dict(h=-0.1), dict(h=float("nan")), dict(tau=41.0, h=0.01), dict(h=1e-60)]
    bad_map = [dict(map=None), dict(map=p + 8), dict(cap_vox=65), dict(cap_vox=1), dict(cap_vox=1 << 25)]
    bad_geo = [dict(voxel=0.0), dict(voxel=float("nan")), dict(voxel=1e-60), dict(origin=None), dict(origin=ctypes.addressof(bad_o))]
    refusals(lib.dpm_tsdf_init, ("map", "cap_vox", "stream"), dict(map=p, cap_vox=64, stream=None), bad_map)
    names = ("map", "cap_vox", "voxel", "origin", "xyz", "count", "cap", "pose", "lo", "hi", "tau", "h", "stream")
    good = dict(map=p, cap_vox=64, voxel=0.2, origin=ctypes.addressof(o), xyz=p, count=p, cap=8, pose=p, stream=None, **rays)
    call = refusals(lib.dpm_tsdf_integrate, names, good,
                    bad_map + bad_geo + bad_rays + [dict(xyz=None), dict(count=None), dict(pose=None), dict(cap=-1)])
    assert call(cap=0) == 0                                                     # an empty frame is a no-op
    names = ("map", "cap_vox", "voxel", "origin", "store", "lengths", "capacity", "P", "frames", "poses", "F", "lo", "hi", "tau", "h",
             "stream")
    good = dict(map=p, cap_vox=64, voxel=0.2, origin=ctypes.addressof(o), store=p, lengths=p, capacity=4, P=8, frames=p, poses=p, F=2,
                stream=None, **rays)
    call = refusals(lib.dpm_tsdf_integrate_frames, names, good,
                    bad_map + bad_geo + bad_rays + [dict(store=None), dict(lengths=None), dict(frames=None), dict(poses=None),
                                                    dict(capacity=0), dict(P=0), dict(F=-1), dict(F=65536)])
    assert call(F=0, store=None, lengths=None, frames=None, poses=None) == 0     # an empty list is a no-op
    refusals(lib.dpm_tsdf_export, ("map", "cap_vox", "keys", "sums", "counts", "count", "max_out", "stream"),
             dict(map=p, cap_vox=64, keys=p, sums=p, counts=p, count=p, max_out=4, stream=None),
             bad_map + [dict(count=None), dict(max_out=-1), dict(keys=None), dict(sums=None), dict(counts=None)])
    refusals(lib.dpm_tsdf_surface, ("map", "cap_vox", "voxel", "min_count", "keys", "axes", "xyz", "normals", "count", "max_out", "stream"),
             dict(map=p, cap_vox=64, voxel=0.2, min_count=1, keys=p, axes=p, xyz=p, normals=p, count=p, max_out=4, stream=None),
             bad_map + bad_geo[:3] + [dict(min_count=0), dict(count=None), dict(max_out=-1), dict(keys=None), dict(axes=None),
                                      dict(xyz=None), dict(normals=None)])
    refusals(lib.dpm_tsdf_mesh, ("map", "cap_vox", "voxel", "min_count", "vkeys", "vdirs", "xyz", "count", "max_out", "stream"),
             dict(map=p, cap_vox=64, voxel=0.2, min_count=1, vkeys=p, vdirs=p, xyz=p, count=p, max_out=4, stream=None),
             bad_map + bad_geo[:3] + [dict(min_count=0), dict(count=None), dict(max_out=-1), dict(vkeys=None), dict(vdirs=None),
                                      dict(xyz=None)])


def test_surface_map_leaves_failed_frames_out():
    from deeppointmap_amd.loop_closure import GeometricSlam
    from deeppointmap_amd.odometry import CONVERGED, MAX_ITER, NO_MATCH, OdometryStep
    slam = GeometricSlam(loop=dict(capacity=8, points_per_frame=8))
    assert slam.surface_rows() == [] and slam.surface_map(0.5, truncation=1.0).table is None
    slam._corrected = [np.eye(4)] * 4
    slam.odometry.steps = [OdometryStep(np.eye(4), 1.0, 0.0, 1, s) for s in (CONVERGED, NO_MATCH, MAX_ITER, CONVERGED)]
    assert slam.surface_rows() == [0, 2, 3]


# ------------------------------------------------------------------------------------------------------------------------ ply
def read_ply(path):
    with open(path, "rb") as f:
        assert f.readline() == b"ply\n" and f.readline() == b"format binary_little_endian 1.0\n"
        counts, props, line = {}, {}, f.readline().decode().split()
        while line != ["end_header"]:
            if line[0] == "element":
                element = line[1]
                counts[element], props[element] = int(line[2]), []
            elif line[0] == "property":
                props[element].append(line[1:])
            line = f.readline().decode().split()
        assert all(p[0] == "float" for p in props["vertex"])
        v = np.frombuffer(f.read(4 * len(props["vertex"]) * counts["vertex"]), "<f4").reshape(counts["vertex"], len(props["vertex"]))
        faces = None
        if "face" in counts:
            assert props["face"] == [["list", "uchar", "int", "vertex_indices"]]
            rec = np.frombuffer(f.read(13 * counts["face"]), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
            assert (rec["n"] == 3).all()
            faces = rec["v"]
        assert f.read() == b""
    return [p[1] for p in props["vertex"]], v, faces


def test_write_ply_round_trips(tmp_path, sphere):
    from deeppointmap_amd import tsdf
    c, m, fld = sphere
    vertices, faces = tsdf.weld(*R.mesh(fld, c.voxel))
    path = str(tmp_path / "mesh.ply")
    tsdf.TsdfMap.write_ply(path, vertices, faces)
    names, v, f = read_ply(path)
    assert names == ["x", "y", "z"] and v.tobytes() == vertices.tobytes() and np.array_equal(f, faces)
    keys, axes, xyz, normals = R.surface(fld, c.voxel)
    tsdf.write_ply(path, xyz, normals=normals)
    names, v, f = read_ply(path)
    assert names == ["x", "y", "z", "nx", "ny", "nz"] and f is None
    assert v[:, :3].tobytes() == xyz.tobytes() and v[:, 3:].tobytes() == normals.tobytes()
    tsdf.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert read_ply(path)[1].shape == (0, 3)
    with pytest.raises(ValueError):
        tsdf.write_ply(path, vertices, faces + len(vertices))
    with pytest.raises(ValueError):
        tsdf.write_ply(path, vertices, normals=normals[:3])
