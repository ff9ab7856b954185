"""GPU: the plane-distance fusion and the free-space carving of the TSDF map (csrc/tsdf_map.hip, deeppointmap_amd/tsdf.py;
DESIGN §7l) against their float32 restatement (tests/tsdf_plane_restated.py), byte for byte, on the inputs of
tests/test_tsdf_plane_host.py -- which shows on the CPU that these inputs tell the restatement's mutants from the true form.

  export        the sorted export and header words 1 and 2 for cap 0, 1, 63, 64, 65, 257, count < cap with NaN rows and NaN /
                zero normals, cos_min exactly met, returns nearer than the truncation, keys outside the 21 bits.
  order         normals of either sign, permuted rows, two frames in either order, a second run, one replay of a captured graph.
  frames        the list forms (integrate and carve) equal the per-frame calls for F in 0, 1, 3, 17 x P in 1, 255, 256, 257.
  carve         on a ray map and on a plane map; twice against once at weight 2; an empty table stays empty; max_range / step
                too large is refused.
  extraction    surface records and mesh triangles of a plane map equal the restatement's after sorting.
  answers       the slanted plane and the two walls of test_tsdf_plane_host.py on the GPU, with the same bounds.
  slam          GeometricSlam.surface_map: the defaults equal a ray-form integrate_frames by hand; distance="plane" with carve
                equals the calls by hand and `unusable()` is read.
Everything observed goes to test_logs/tsdf.log.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_cases as C  # noqa: E402
import tsdf_plane_restated as PR  # noqa: E402
import tsdf_restated as R  # noqa: E402
import test_tsdf_plane_host as H  # noqa: E402
from test_tsdf_host import fuse, log, valid  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("keys", "sums", "counts")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_map(c, distance="plane"):
    from deeppointmap_amd.tsdf import TsdfMap
    kw = dict(cos_min=c.cos_min) if distance == "plane" else {}
    return TsdfMap(c.voxel, c.truncation, c.step, c.cap_vox, c.min_range, c.max_range, origin=c.origin, device=DEV, distance=distance, **kw)


def gpu_fuse(c, m=None, order=None, rows=None, sign=1.0):
    m = gpu_map(c) if m is None else m
    for f in (range(len(c.frames)) if order is None else order):
        xyz, count, pose = c.frames[f]
        count = len(xyz) if count is None else count
        nrm = c.normals[f] * np.float32(sign)
        if len(nrm) < len(xyz):                                      # rows past the count have no normal of their own
            nrm = np.concatenate([nrm, np.zeros((len(xyz) - len(nrm), 3), np.float32)])
        if rows is not None:
            xyz, nrm = xyz[rows], nrm[rows]
        m.integrate(dev(xyz), pose, length=count, normals=dev(nrm))
    return m


def gpu_carve(m, c, weight, frames=None):
    for xyz, count, pose in (c.frames if frames is None else frames):
        m.carve(dev(xyz), pose, length=len(xyz) if count is None else count, weight=weight)
    return m


def header(m):
    return m.table[:12].view(torch.int32).cpu().numpy().tolist()     # [overflow, outside, unusable]


def same_export(g, r, what):
    a, b = g.export(), r.export()
    for x, y, name in zip(a, b, NAMES):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name, x.dtype, y.dtype, x.shape, y.shape)
        assert x.tobytes() == y.tobytes(), (what, name)
    return a


def bytes_of(m):
    return [a.tobytes() for a in m.export()]


# --------------------------------------------------------------------------------------------------------------------- export
@pytest.mark.parametrize("name", sorted(H.plane_cases()))
def test_the_sorted_export_is_the_restatement_byte_for_byte(name):
    c = H.plane_cases()[name]
    want = H.fuse_plane(c)
    got = gpu_fuse(c)
    keys = same_export(got, want, name)[0]
    assert header(got) == [0, want.outside, want.unusable], (name, header(got), want.outside, want.unusable)
    assert got.check() is got and got.outside() == want.outside and got.unusable() == want.unusable
    log(f"gpu plane export '{name}': {len(keys)} voxels, weight {sum(want.count.values())}, {want.outside} samples outside the keys, "
        f"{want.unusable} rows unusable: identical bytes")
    if name == "cap0":
        assert len(keys) == 0
    if name == "cos_met":
        assert want.unusable == 5 and len(keys) > 0


def test_the_same_bytes_for_either_sign_in_any_order_twice_and_from_a_captured_graph():
    from deeppointmap_amd import ops
    c = H.plane_cases()["two_frames"]
    want = H.fuse_plane(c)
    ref = [a.tobytes() for a in want.export()]
    perm = np.random.default_rng(1).permutation(257)
    for what, m in (("in order", gpu_fuse(c)), ("again", gpu_fuse(c)), ("frames swapped", gpu_fuse(c, order=[1, 0])),
                    ("rows permuted", gpu_fuse(c, rows=perm)), ("normals turned round", gpu_fuse(c, sign=-1.0))):
        assert bytes_of(m) == ref, what
        assert header(m) == [0, want.outside, want.unusable], what
    # one replay of a captured graph: clear + both frames + a carve of each, on tensors that are on the device already
    carved = [a.tobytes() for a in H.carve_all(H.fuse_plane(c), c, 256).export()]
    g = gpu_map(c)
    g._ready(torch.device(DEV))
    held = [(dev(x), torch.full((1,), n, dtype=torch.int32).to(DEV), dev(p), dev(nr)) for (x, n, p), nr in zip(c.frames, c.normals)]

    def work():
        ops.tsdf_clear(g.table, g.max_voxels)
        for x, n, p, nr in held:
            g.integrate(x, p, length=n, normals=nr)
        for x, n, p, nr in held:
            g.carve(x, p, length=n)
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
    assert bytes_of(g) == carved, "replayed from a captured graph"
    log(f"gpu plane order: {len(want.sum)} voxels: identical bytes in order, again, frames swapped, rows permuted, normals turned "
        "round; fused and carved from a replayed graph")


def test_fusion_and_carving_make_no_host_synchronisation():
    from deeppointmap_amd import augment
    c, lst = H.plane_cases()["two_frames"], H.list_case(17, 257)
    m, ml = gpu_map(c), gpu_map(lst)
    m._ready(torch.device(DEV)), ml._ready(torch.device(DEV))
    held = [(dev(x), torch.full((1,), n, dtype=torch.int32).to(DEV), dev(p), dev(nr)) for (x, n, p), nr in zip(c.frames, c.normals)]
    store, lengths, rows, poses, normals = dev(lst.store), dev(lst.lengths), dev(lst.rows), dev(lst.poses), dev(lst.normal_store)
    torch.cuda.synchronize()
    before = augment.host_syncs()
    torch.cuda.set_sync_debug_mode("error")      # any synchronising torch call raises
    try:
        for x, n, p, nr in held:
            m.integrate(x, p, length=n, normals=nr)
        for x, n, p, nr in held:
            m.carve(x, p, length=n)
        ml.integrate_frames(store, lengths, rows, poses, normals=normals)
        ml.carve_frames(store, lengths, rows, poses)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert augment.host_syncs() == before
    n = augment.host_syncs()
    m.unusable()
    assert augment.host_syncs() == n + 1
    same_export(m, H.carve_all(H.fuse_plane(c), c, 256), "after the guarded calls")


# --------------------------------------------------------------------------------------------------------------------- frames
@pytest.mark.parametrize("F,P", C.LIST_SHAPES)
def test_the_list_forms_equal_the_per_frame_calls(F, P):
    c = H.list_case(F, P)
    store, lengths, rows, poses, normals = dev(c.store), dev(c.lengths), dev(c.rows), dev(c.poses), dev(c.normal_store)
    by_list = gpu_map(c).integrate_frames(store, lengths, rows, poses, normals=normals)    # one row may lie outside the store
    per_frame = gpu_map(c)
    per_frame._ready(torch.device(DEV))
    inside = [(f, r) for f, r in enumerate(c.rows) if 0 <= r < store.shape[0]]
    for f, r in inside:
        per_frame.integrate(store[r].t().contiguous(), c.poses[f], length=lengths[r:r + 1].clamp(0, P), normals=normals[r].contiguous())
    want = H.fuse_plane(c)
    same_export(by_list, want, "the list")
    same_export(per_frame, want, "per frame")
    if F:
        assert header(by_list) == header(per_frame) == [0, want.outside, want.unusable]
    # the carve of the same list on top, against the carve of each frame
    by_list.carve_frames(store, lengths, rows, poses, weight=1.5)
    for f, r in inside:
        per_frame.carve(store[r].t().contiguous(), c.poses[f], length=lengths[r:r + 1].clamp(0, P), weight=1.5)
    H.carve_all(want, c, 384)
    same_export(by_list, want, "the list, carved")
    same_export(per_frame, want, "per frame, carved")
    if F == 0:
        assert by_list.table is None or len(by_list.export()[0]) == 0
    if F >= 3:
        assert len(c.frames) == F - 1                                            # one entry named a row outside the store
    log(f"gpu plane frames F {F} P {P}: {len(want.sum)} voxels, {want.unusable} rows unusable: the lists, the per-frame calls and the "
        "restatement agree byte for byte, fused and carved")


# ---------------------------------------------------------------------------------------------------------------------- carve
def test_carve_on_a_ray_map_and_on_a_plane_map_twice_and_on_an_empty_table():
    from deeppointmap_amd import ops
    c = H.plane_cases()["two_frames"]
    # a ray map: weight in samples
    ray = gpu_map(c, "ray")
    for xyz, n, pose in c.frames:
        ray.integrate(dev(xyz), pose, length=n)
    want = fuse(c)
    untouched = [a.tobytes() for a in want.export()]
    same_export(gpu_carve(ray, c, 3), H.carve_all(want, c, 3), "ray map carved")
    assert [a.tobytes() for a in want.export()][0] == untouched[0] and [a.tobytes() for a in want.export()][1] != untouched[1]
    # a plane map: weight 1 is 256 count units; twice is once at weight 2; either order of the frames
    wantp = H.carve_all(H.fuse_plane(c), c, 512)
    twice = gpu_carve(gpu_carve(gpu_fuse(c), c, 1), c, 1, frames=c.frames[::-1])
    once = gpu_carve(gpu_fuse(c), c, 2)
    same_export(twice, wantp, "plane map carved twice")
    same_export(once, wantp, "plane map carved at weight 2")
    assert len(wantp.sum) == len(H.fuse_plane(c).sum) and header(once) == [0, wantp.outside, wantp.unusable]
    # an empty table stays empty, through the class (no table at all) and at the entry point
    assert gpu_map(c).carve(dev(c.frames[0][0]), c.frames[0][2]).table is None
    empty = gpu_map(c)
    empty._ready(torch.device(DEV))
    xyz, n, pose = c.frames[0]
    ops.tsdf_carve(empty.table, empty.max_voxels, empty.voxel_size, empty.origin, dev(xyz), torch.full((1,), n, dtype=torch.int32).to(DEV),
                   dev(pose), *empty._rays(), 256, 2.0)
    assert len(empty.export()[0]) == 0 and header(empty) == [0, 0, 0]
    log(f"gpu carve: a ray map and a plane map of {len(wantp.sum)} voxels carved: identical bytes; twice equals weight 2; an empty table "
        "stays empty")


def test_too_many_carve_steps_are_refused():
    from deeppointmap_amd import _lib, ops
    from deeppointmap_amd.tsdf import TsdfMap
    m = TsdfMap(0.5, truncation=0.6, step=1e-3, max_range=100.0, max_voxels=1 << 10, device=DEV)
    xyz = dev(np.array([[3.0, 0, 0]], np.float32))
    m.integrate(xyz, np.eye(4))
    before = bytes_of(m)
    with pytest.raises(ValueError, match="max_range / step"):
        m.carve(xyz, np.eye(4))
    import ctypes
    o = (ctypes.c_double * 3)(0, 0, 0)
    count, pose = torch.ones(1, dtype=torch.int32, device=DEV), dev(np.eye(4))
    rc = _lib.load().dpm_tsdf_carve(m.table.data_ptr(), m.max_voxels, 0.5, ctypes.addressof(o), xyz.data_ptr(), count.data_ptr(), 1,
                                    pose.data_ptr(), 0.0, 100.0, 0.6, 1e-3, 1, 1.0, torch.cuda.current_stream().cuda_stream)
    assert rc == -1 and bytes_of(m) == before
    assert ops.TSDF_MAX_CARVE_STEPS == 65536


# ----------------------------------------------------------------------------------------------------------------- extraction
def gpu_surface(m, min_count=1):
    s = m.surface(min_count)
    return (s.keys.cpu().numpy(), s.axes.cpu().numpy(), np.ascontiguousarray(s.xyz_map.t().cpu().numpy()),
            np.ascontiguousarray(s.normals.t().cpu().numpy()))


@pytest.mark.parametrize("name,min_count", [("wall", 1), ("wall", 2.5), ("two_frames", 1 / 256)])
def test_surface_and_mesh_of_a_plane_map_are_the_restatement_byte_for_byte(name, min_count):
    from deeppointmap_amd import ops, tsdf
    c = H.plane_cases()[name]
    want, got = H.fuse_plane(c), gpu_fuse(c)
    units = max(1, round(min_count * 256))
    fld = R.field(want.export(), units)
    gk, gD = got.field(min_count)
    assert gk.tobytes() == fld[0].tobytes() and gD.dtype == np.float32 and gD.tobytes() == fld[1].tobytes()
    ws, gs = R.surface(fld, c.voxel), gpu_surface(got, min_count)
    for x, y, what in zip(gs, ws, ("keys", "axes", "positions", "normals")):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (name, "surface", what)
    wt = R.sort_triangles(*R.mesh(fld, c.voxel))
    gt = R.sort_triangles(*[t.cpu().numpy() for t in ops.tsdf_mesh(got.table, got.max_voxels, got.voxel_size, units)[1:]])
    for x, y, what in zip(gt, wt, ("vertex keys", "vertex directions", "positions")):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (name, "mesh", what)
    vertices, faces = got.mesh(min_count)
    wv, wf = tsdf.weld(*wt)
    assert vertices.tobytes() == wv.tobytes() and faces.tobytes() == wf.tobytes()
    log(f"gpu plane extraction '{name}' min_count {min_count:g} ({units} count units): {len(gk)} qualified voxels, {len(gs[0])} surface "
        f"records, {len(gt[0])} triangles: identical bytes")
    assert len(gs[0]) > 0 and (len(gt[0]) > 0 or name == "two_frames")


# -------------------------------------------------------------------------------------------------------------------- answers
@pytest.mark.parametrize("tilt", H.TILTS)
def test_slanted_plane_known_answer_on_the_gpu(tilt):
    """Observed on an MI355X (test_logs/tsdf.log): the host test's figures, the tables being the same bytes: plane distance at
    most 2.1e-6 m from the plane (bound 1e-4), the along-ray form 36 to 43 mm on average (floor 10 mm)."""
    c = H.slanted(tilt)
    plane = gpu_fuse(c).check()
    same_export(plane, H.fuse_plane(c), f"slanted {tilt}")
    ray = gpu_map(c, "ray").integrate(dev(c.frames[0][0]), c.frames[0][2]).check()
    H.slanted_report("gpu", tilt, c, gpu_surface(plane, 1 / 256)[2], gpu_surface(ray, 1)[2])


def test_carve_known_answer_on_the_gpu():
    """Observed on an MI355X: 144 records of the wall at 5 m in front of the sensor before, 0 after; the 1200 records of the wall at
    10 m keep their bytes; 9926 keys before and after."""
    c = H.two_walls()
    m = gpu_fuse(c).check()
    before, n0 = gpu_surface(m, 1), len(m.export()[0])
    gpu_carve(m, c, 2, frames=c.frames[1:])
    want = PR.carve(H.fuse_plane(c), *valid(c.frames[1]), 512, c.truncation + c.voxel)
    same_export(m, want, "two walls, carved")
    H.walls_report("gpu", c, before, gpu_surface(m, 1), n0, len(m.export()[0]))


def test_normals_estimated_from_the_frame_cost_one_read_and_equal_the_normals_by_hand():
    from deeppointmap_amd import augment, ops
    c = H.plane_cases()["wall"]
    xyz, n, pose = c.frames[0]
    x = dev(xyz)
    before = augment.host_syncs()
    got = gpu_map(c).integrate(x, pose, length=n - 40, normals=0.7)
    assert augment.host_syncs() == before + 1
    lengths = torch.full((1,), n - 40, dtype=torch.int32, device=DEV)
    nrm = torch.zeros_like(x)
    nrm[:n - 40] = ops.icp_target_normals(x[:n - 40].t().contiguous()[None], lengths, lengths[:0], 0.7, host=([0], [n - 40]))[0]
    by_hand = gpu_map(c).integrate(x, pose, length=n - 40, normals=nrm)
    assert bytes_of(got) == bytes_of(by_hand) and len(got.export()[0]) > 100
    s = got.surface(1 / 256)
    n_w = np.array([1.0, -0.3, 0.2]) / np.linalg.norm([1.0, -0.3, 0.2])
    err = np.abs(s.xyz_map.double().cpu().numpy().T @ n_w - 4.0 * n_w[0])
    log(f"gpu plane, normals estimated within 0.7 m: {got.unusable()} rows unusable, {len(err)} surface records, max {err.max():.3e} m "
        "from the wall (reported, not asserted)")


# ----------------------------------------------------------------------------------------------------------------------- slam
def test_geometric_slam_surface_map_defaults_plane_and_carve():
    """8 simulated frames along a street under the point metric, so that the loop closer holds no normals until surface_map asks"""
    from deeppointmap_amd import augment
    from deeppointmap_amd import lidar_sim as LS
    from deeppointmap_amd.loop_closure import GeometricSlam
    from deeppointmap_amd.tsdf import TsdfMap
    n = 8
    scene = LS.street_scene(2, blocks=(1, 1))
    model = LS.LidarModel(np.linspace(10.0, -20.0, 16), 256, 0.9, 80.0, range_sigma=0.0, drop_prob=0.0)
    truth = LS.circuit(scene, spacing=1.0)[:n]
    frames = LS.LidarSimulator(scene, model, device=DEV).frames(truth)
    slam = GeometricSlam(odometry=dict(max_range=model.max_range, first_pose=truth[0], initial_motion=LS.sweep_delta(truth[0], truth[1]),
                                       sample_map=0.25, sample_register=0.75, metric="plane"),
                         loop=dict(capacity=n, points_per_frame=model.rays, metric="point",
                                   sc=dict(max_range=model.max_range, z_offset=LS.SENSOR_HEIGHT)))
    for f in frames:
        slam.step(f)
    lc, rows = slam.loop_closer, slam.surface_rows()
    assert rows == list(range(n)) and lc.normals is None
    kw = dict(truncation=0.9, max_voxels=1 << 20, max_range=model.max_range, min_range=0.9)
    before = augment.host_syncs()
    got = slam.surface_map(0.3, **kw)
    assert augment.host_syncs() == before and got.distance == "ray" and lc.normals is None
    by_hand = TsdfMap(0.3, **kw).integrate_frames(lc.store, lc.lengths, rows, slam.poses[rows])
    a, b = got.check().export(), by_hand.check().export()
    assert len(a[0]) > 5000 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    before = augment.host_syncs()
    plane = slam.surface_map(0.3, distance="plane", carve=1.0, cos_min=0.1, **kw)
    assert augment.host_syncs() == before and plane.unit == 256 and lc.normals is not None and lc.normals.shape == (n, model.rays, 3)
    hand = TsdfMap(0.3, distance="plane", cos_min=0.1, **kw).integrate_frames(lc.store, lc.lengths, rows, slam.poses[rows], normals=lc.normals)
    fused = hand.export()
    hand.carve_frames(lc.store, lc.lengths, rows, slam.poses[rows], weight=1.0)
    c, d = plane.check().export(), hand.export()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(c, d)) and c[0].tobytes() == fused[0].tobytes() and c[1].tobytes() != fused[1].tobytes()
    unusable, stored = plane.unusable(), int(lc.lengths.sum().item())
    assert 0 < unusable < stored                                       # grazing returns and returns without neighbours are left out
    again = slam.surface_map(0.3, distance="plane", cos_min=0.1, **kw)  # the normals are there now: the same map, not carved
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again.export(), fused))
    surf = plane.surface(min_count=2)
    log(f"gpu slam plane: {n} frames, {stored} stored points, {unusable} unusable, {len(c[0])} voxels, {surf.xyz.shape[1]} surface points "
        "with min_count 2; defaults equal the ray form by hand, plane + carve equal the calls by hand")
