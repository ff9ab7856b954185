"""GPU: the TSDF surface map (csrc/tsdf_map.hip, deeppointmap_amd/tsdf.py) against its float32 restatement
(tests/tsdf_restated.py), byte for byte, on the inputs of tests/tsdf_cases.py -- tests/test_tsdf_host.py shows on the CPU that
these inputs tell the restatement's three mutants from the true form and stay under the ambiguity cap.

  export        the sorted export and header word 1 for cap 0, 1, 63, 64, 65, 257, count < cap, NaN rows, both range gates at
                equality, lattice points on voxel faces, rays inside face planes, returns nearer than the truncation, keys
                outside the 21 bits; a table too small raises.
  order         permuted rows, two frames in either order, a second run, one replay of a captured graph: the same bytes.
  frames        integrate_frames equals the per-frame calls for F in 0, 1, 3, 17 x P in 1, 255, 256, 257 (lengths 0, above P,
                negative; a row outside the store).
  extraction    field, surface records and mesh triangles equal the restatement's after sorting; max_out below the count.
  sphere        the known answer of test_tsdf_host.py on the GPU, and the float64 field within 1 mm.
  slam          GeometricSlam.surface_map equals integrate_frames called by hand.
Everything observed goes to test_logs/tsdf.log.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_cases as C  # noqa: E402
import tsdf_restated as R  # noqa: E402
from test_tsdf_host import CAP, FIELD_BOUND, fuse, fuse64, log, sphere_report  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("keys", "sums", "counts")


def gpu_map(c, cap_vox=None):
    from deeppointmap_amd.tsdf import TsdfMap
    return TsdfMap(c.voxel, c.truncation, c.step, c.cap_vox if cap_vox is None else cap_vox, c.min_range, c.max_range,
                   origin=c.origin, device=DEV)


def gpu_fuse(c, m=None, order=None, rows=None):
    m = gpu_map(c) if m is None else m
    for f in (range(len(c.frames)) if order is None else order):
        xyz, count, pose = c.frames[f]
        xyz = xyz if rows is None else xyz[rows]
        m.integrate(torch.from_numpy(np.ascontiguousarray(xyz)).to(DEV), pose, length=count)
    return m


def header(m):
    return m.table[:8].view(torch.int32).cpu().numpy().tolist()     # [overflow, outside]


def same_export(g, r, what):
    a, b = g.export(), r.export()
    for x, y, name in zip(a, b, NAMES):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name, x.dtype, y.dtype, x.shape, y.shape)
        assert x.tobytes() == y.tobytes(), (what, name)
    return a


def bytes_of(m):
    return [a.tobytes() for a in m.export()]


# --------------------------------------------------------------------------------------------------------------------- export
@pytest.mark.parametrize("name", sorted(C.single_frame_cases()))
def test_the_sorted_export_is_the_restatement_byte_for_byte(name):
    c = C.single_frame_cases()[name]
    want = fuse(c)
    got = gpu_fuse(c)
    keys = same_export(got, want, name)[0]
    assert header(got) == [0, want.outside], (name, header(got), want.outside)
    assert got.check() is got and got.outside() == want.outside
    log(f"gpu export '{name}': {len(keys)} voxels, {sum(want.count.values())} samples, {want.outside} outside the keys: identical bytes")
    if name == "outside":
        assert want.outside > 0 and len(keys) > 0
    if name == "cap0":
        assert len(keys) == 0


def test_a_table_too_small_overflows_and_check_raises():
    c = C.too_small()
    want = fuse(c)
    assert len(want.sum) > c.cap_vox
    got = gpu_fuse(c)
    n = got.overflow()
    log(f"gpu overflow: {len(want.sum)} voxels offered to {c.cap_vox} slots: {n} samples found none")
    assert n > 0
    with pytest.raises(ValueError, match="full"):
        got.check()
    assert len(got.export()[0]) == c.cap_vox                   # every slot was taken, and nothing was written beyond them


# ---------------------------------------------------------------------------------------------------------------------- order
def test_the_same_bytes_in_any_order_twice_and_from_a_captured_graph():
    from deeppointmap_amd import ops
    c = C.two_frames()
    want = fuse(c)
    ref = [a.tobytes() for a in want.export()]
    perm = np.random.default_rng(1).permutation(257)
    for what, m in (("in order", gpu_fuse(c)), ("again", gpu_fuse(c)), ("frames swapped", gpu_fuse(c, order=[1, 0])),
                    ("rows permuted", gpu_fuse(c, rows=perm))):
        assert bytes_of(m) == ref, what
    from deeppointmap_amd.augment import PointCloud
    as_frames = gpu_map(c)
    for xyz, n, pose in c.frames:
        as_frames.integrate(PointCloud(xyz[:n], capacity=n + 7), pose)          # a frame with room past its length
    assert bytes_of(as_frames) == ref, "as augment.PointCloud frames"
    with pytest.raises(ValueError):
        as_frames.integrate(PointCloud(c.frames[0][0]), c.frames[0][2], length=3)
    # one replay of a captured graph: clear + both frames, on tensors that are on the device already
    g = gpu_map(c)
    g._ready(torch.device(DEV))
    dev = [(torch.from_numpy(x).to(DEV), torch.full((1,), n, dtype=torch.int32).to(DEV), torch.from_numpy(p).to(DEV)) for x, n, p in c.frames]

    def work():
        ops.tsdf_clear(g.table, g.max_voxels)
        for x, n, p in dev:
            g.integrate(x, p, length=n)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        work()
    g.table.zero_()                 # not a map any more: the replay has to make it one
    graph.replay()
    torch.cuda.synchronize()
    assert bytes_of(g) == ref, "replayed from a captured graph"
    log(f"gpu order: {len(want.sum)} voxels: identical bytes in order, again, frames swapped, rows permuted, replayed from a graph")


# --------------------------------------------------------------------------------------------------------------------- frames
def on_device(c):
    return (torch.from_numpy(c.store).to(DEV), torch.from_numpy(c.lengths).to(DEV), torch.from_numpy(c.rows).to(DEV),
            torch.from_numpy(np.ascontiguousarray(c.poses)).to(DEV))


@pytest.mark.parametrize("F,P", C.LIST_SHAPES)
def test_integrate_frames_equals_the_per_frame_calls(F, P):
    c = C.list_case(F, P)
    store, lengths, rows, poses = on_device(c)
    by_list = gpu_map(c).integrate_frames(store, lengths, rows, poses)         # the rows on the device: one may lie outside the store
    per_frame = gpu_map(c)
    per_frame._ready(torch.device(DEV))
    for f, r in enumerate(c.rows):
        if 0 <= r < store.shape[0]:
            per_frame.integrate(store[r].t().contiguous(), c.poses[f], length=lengths[r:r + 1].clamp(0, P))
    want = fuse(c)
    same_export(by_list, want, "the list")
    same_export(per_frame, want, "per frame")
    assert header(by_list) == header(per_frame) == [0, want.outside]
    if F == 0:
        assert by_list.table is None or len(by_list.export()[0]) == 0
    if F >= 3:
        assert len(c.frames) == F - 1                                            # one entry named a row outside the store
    log(f"gpu frames F {F} P {P}: {len(want.sum)} voxels: the list, the per-frame calls and the restatement agree byte for byte")


# ----------------------------------------------------------------------------------------------------------------- extraction
def gpu_surface(m, min_count=1):
    s = m.surface(min_count)
    return (s.keys.cpu().numpy(), s.axes.cpu().numpy(), np.ascontiguousarray(s.xyz_map.t().cpu().numpy()),
            np.ascontiguousarray(s.normals.t().cpu().numpy()))


def gpu_triangles(m, min_count=1):
    from deeppointmap_amd import ops
    return R.sort_triangles(*[t.cpu().numpy() for t in ops.tsdf_mesh(m.table, m.max_voxels, m.voxel_size, min_count)[1:]])


@pytest.mark.parametrize("name,min_count", [("two_frames", 1), ("wall", 1), ("wall", 2), ("lattice", 1), ("sphere", 1), ("sphere", 3)])
def test_field_surface_and_mesh_are_the_restatement_byte_for_byte(name, min_count):
    from deeppointmap_amd import tsdf
    c = C.sphere() if name == "sphere" else C.single_frame_cases()[name]
    want = fuse(c)
    got = gpu_fuse(c)
    fld = R.field(want.export(), min_count)
    gk, gD = got.field(min_count)
    assert gk.tobytes() == fld[0].tobytes() and gD.dtype == np.float32 and gD.tobytes() == fld[1].tobytes()
    ws, gs = R.surface(fld, c.voxel), gpu_surface(got, min_count)
    for x, y, what in zip(gs, ws, ("keys", "axes", "positions", "normals")):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (name, "surface", what)
    wt, gt = R.sort_triangles(*R.mesh(fld, c.voxel)), gpu_triangles(got, min_count)
    for x, y, what in zip(gt, wt, ("vertex keys", "vertex directions", "positions")):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (name, "mesh", what)
    vertices, faces = got.mesh(min_count)
    wv, wf = tsdf.weld(*wt)
    assert vertices.tobytes() == wv.tobytes() and faces.tobytes() == wf.tobytes() and faces.dtype == np.int32
    log(f"gpu extraction '{name}' min_count {min_count}: {len(gk)} qualified voxels, {len(gs[0])} surface records, {len(gt[0])} triangles, "
        f"{len(vertices)} welded vertices: identical bytes")
    assert len(gs[0]) > 0 and (len(gt[0]) > 0 or name == "two_frames")    # 257 scattered rays leave no cell with its 8 corners


def test_max_out_below_the_count_reports_the_count_and_writes_nothing_beyond():
    from deeppointmap_amd import _lib, ops
    c = C.wall()
    m = gpu_fuse(c)
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    totals = (ops.tsdf_export(m.table, m.max_voxels, 0), ops.tsdf_surface(m.table, m.max_voxels, c.voxel, 1, 0),
              ops.tsdf_mesh(m.table, m.max_voxels, c.voxel, 1, 0))
    assert totals[0] == len(fuse(c).sum) and all(t > 8 for t in totals)
    for fn, total in zip((ops.tsdf_export, ops.tsdf_surface, ops.tsdf_mesh), totals):
        args = (m.table, m.max_voxels) + (() if fn is ops.tsdf_export else (c.voxel, 1))
        n, *out = fn(*args, total // 2)
        assert n == total and all(len(t) == total // 2 for t in out)
        assert fn(*args, total + 5)[0] == total and len(fn(*args, total + 5)[1]) == total
    # straight at the entry points, the outputs filled first: rows at and past max_out keep their bytes
    cut = totals[0] // 2
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    keys, sums = torch.full((totals[0],), -7, dtype=torch.int64, device=DEV), torch.full((totals[0],), -7, dtype=torch.int64, device=DEV)
    counts = torch.full((totals[0],), -7, dtype=torch.int32, device=DEV)
    _lib.check(lib.dpm_tsdf_export(m.table.data_ptr(), m.max_voxels, keys.data_ptr(), sums.data_ptr(), counts.data_ptr(),
                                   count.data_ptr(), cut, st), "dpm_tsdf_export")
    assert int(count.item()) == totals[0] and bool((keys[cut:] == -7).all() & (sums[cut:] == -7).all() & (counts[cut:] == -7).all())
    assert bool((keys[:cut] >= 0).all() & (counts[:cut] > 0).all())
    cut = totals[1] // 2
    count.zero_()
    keys, axes = torch.full((totals[1],), -7, dtype=torch.int64, device=DEV), torch.full((totals[1],), -7, dtype=torch.int32, device=DEV)
    xyz, nrm = torch.full((totals[1], 3), -7.0, device=DEV), torch.full((totals[1], 3), -7.0, device=DEV)
    _lib.check(lib.dpm_tsdf_surface(m.table.data_ptr(), m.max_voxels, c.voxel, 1, keys.data_ptr(), axes.data_ptr(), xyz.data_ptr(),
                                    nrm.data_ptr(), count.data_ptr(), cut, st), "dpm_tsdf_surface")
    assert int(count.item()) == totals[1]
    assert bool((keys[cut:] == -7).all() & (axes[cut:] == -7).all() & (xyz[cut:] == -7).all() & (nrm[cut:] == -7).all())
    assert bool((axes[:cut] >= 0).all())
    cut = totals[2] // 2
    count.zero_()
    vk, vd = torch.full((totals[2], 3), -7, dtype=torch.int64, device=DEV), torch.full((totals[2], 3), -7, dtype=torch.int32, device=DEV)
    xyz = torch.full((totals[2], 3, 3), -7.0, device=DEV)
    _lib.check(lib.dpm_tsdf_mesh(m.table.data_ptr(), m.max_voxels, c.voxel, 1, vk.data_ptr(), vd.data_ptr(), xyz.data_ptr(),
                                 count.data_ptr(), cut, st), "dpm_tsdf_mesh")
    assert int(count.item()) == totals[2]
    assert bool((vk[cut:] == -7).all() & (vd[cut:] == -7).all() & (xyz[cut:] == -7).all()) and bool((vd[:cut] >= 0).all())
    log(f"gpu max_out: counts {totals} reported with half the room, nothing written past it")


def test_fusion_makes_no_host_synchronisation_and_an_extraction_one():
    from deeppointmap_amd import augment
    c, lst = C.two_frames(), C.list_case(17, 257)
    m, ml = gpu_map(c), gpu_map(lst)
    m._ready(torch.device(DEV)), ml._ready(torch.device(DEV))
    dev = [(torch.from_numpy(x).to(DEV), torch.full((1,), n, dtype=torch.int32).to(DEV), torch.from_numpy(p).to(DEV)) for x, n, p in c.frames]
    store, lengths, rows, poses = on_device(lst)
    torch.cuda.synchronize()
    before = augment.host_syncs()
    torch.cuda.set_sync_debug_mode("error")      # any synchronising torch call raises
    try:
        for x, n, p in dev:
            m.integrate(x, p, length=n)
        ml.integrate_frames(store, lengths, rows, poses)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert augment.host_syncs() == before
    for fn in (m.export, m.field, m.surface, m.mesh, m.overflow, m.check):
        n = augment.host_syncs()
        fn()
        assert augment.host_syncs() == n + 1, fn.__name__
    same_export(m, fuse(c), "after the guarded calls")
    same_export(ml, fuse(lst), "after the guarded list call")


# --------------------------------------------------------------------------------------------------------------------- sphere
@pytest.mark.parametrize("far", [None, (1000.0, -1000.0, 1000.0)])
def test_sphere_seen_from_its_centre_on_the_gpu(far):
    """Observed on an MI355X (test_logs/tsdf.log), at the world's zero and 1 km out alike: 13213 voxels, none of the 6312 needed
    missing; 2728 crossings at most 3.20 mm and 8148 mesh vertices at most 6.18 mm from the sphere (bound 10.42 mm); euler 2,
    closed, oriented; field against float64 1.3e-7 m with 0.58 % of the voxels ambiguous."""
    c = C.sphere(far)
    m = gpu_fuse(c).check()
    fld = m.field()
    s = m.surface()
    assert np.array_equal(s.origin, c.origin)
    surf = (s.keys.cpu().numpy(), s.axes.cpu().numpy(), s.xyz_map.t().cpu().numpy(), s.normals.t().cpu().numpy())
    world = s.xyz_map.double().cpu().numpy() + c.origin[:, None]
    assert np.array_equal(s.xyz.cpu().numpy(), world.astype(np.float32))         # world coordinates, rounded once
    vertices, faces = m.mesh()
    sphere_report("gpu" if far is None else "gpu, 1 km out,", c, fld, surf, vertices, faces)
    err, lonely, share = R.compare_fields(fld, fuse64(c))
    log(f"gpu sphere{'' if far is None else ' 1 km out'}: field against float64 on unambiguous voxels: max |dD| {err:.3e} m (bound "
        f"{FIELD_BOUND:.0e}), {lonely} voxels in one form only, ambiguous share {share:.4%}")
    assert share <= CAP and lonely == 0 and err <= FIELD_BOUND


# ----------------------------------------------------------------------------------------------------------------------- slam
def test_geometric_slam_surface_map_is_integrate_frames_by_hand():
    """12 simulated frames along a street, a loop edge taken at frame 9 so that the corrected poses differ from the odometry's"""
    from deeppointmap_amd import augment
    from deeppointmap_amd import lidar_sim as LS
    from deeppointmap_amd.loop_closure import GeometricSlam, LoopEdge
    from deeppointmap_amd.tsdf import TsdfMap
    n, at = 12, 9
    scene = LS.street_scene(2, blocks=(1, 1))
    model = LS.LidarModel(np.linspace(10.0, -20.0, 16), 256, 0.9, 80.0, range_sigma=0.0, drop_prob=0.0)
    truth = LS.circuit(scene, spacing=1.0)[:n]
    frames = LS.LidarSimulator(scene, model, device=DEV).frames(truth)
    slam = GeometricSlam(odometry=dict(max_range=model.max_range, first_pose=truth[0], initial_motion=LS.sweep_delta(truth[0], truth[1]),
                                       sample_map=0.25, sample_register=0.75, metric="plane"),
                         loop=dict(capacity=n, points_per_frame=model.rays, sc=dict(max_range=model.max_range, z_offset=LS.SENSOR_HEIGHT)))
    lc = slam.loop_closer
    real_add = lc.add

    def add(pcd, pose):
        out = real_add(pcd, pose)
        if len(lc.poses) - 1 == at:
            edge = LoopEdge(at, 0, np.linalg.inv(truth[0]) @ truth[at], 1.0, 0.0, 0.0, 0)
            lc._take([edge])
            out = out + [edge]
        return out
    lc.add = add
    for f in frames:
        slam.step(f)
    rows = slam.surface_rows()
    assert rows == list(range(n))                                 # every registration succeeded
    assert np.abs(slam.poses - np.stack(slam.odometry.poses)).max() > 0     # the correction moved something
    kw = dict(truncation=0.9, max_voxels=1 << 20, max_range=model.max_range, min_range=0.9)
    before = augment.host_syncs()
    got = slam.surface_map(0.3, **kw)
    assert augment.host_syncs() == before and isinstance(got, TsdfMap) and got.voxel_size == 0.3
    by_hand = TsdfMap(0.3, **kw).integrate_frames(lc.store, lc.lengths, rows, slam.poses[rows])
    a, b = got.check().export(), by_hand.check().export()
    assert len(a[0]) > 10000 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    raw = TsdfMap(0.3, **kw).integrate_frames(lc.store, lc.lengths, rows, np.stack(slam.odometry.poses)[rows]).export()
    assert raw[0].tobytes() != a[0].tobytes() or raw[1].tobytes() != a[1].tobytes()
    surf = got.surface(min_count=2)
    log(f"gpu slam: {n} frames, {len(a[0])} voxels, {surf.xyz.shape[1]} surface points with min_count 2; surface_map equals "
        f"integrate_frames by hand under the corrected poses and differs from the odometry's poses")
