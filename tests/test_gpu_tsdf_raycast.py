"""GPU: the ray-cast of the TSDF map (csrc/tsdf_map.hip: dpm_tsdf_blocks, dpm_tsdf_raycast; deeppointmap_amd/tsdf.py: raycast,
render, TsdfTracker.predicted; DESIGN §7l "Ray-casting the field") against its float32 restatement (tests/tsdf_raycast_restated.py)
read from the GPU's own export, byte for byte, with the occupied-block set and without it, on the inputs of
tests/test_tsdf_raycast_host.py -- which shows on the CPU that these inputs tell the restatement's mutants from the true form.

  bytes       range, normals and flag for R in 0, 1, 63, 64, 65, 257, F in 1 and 3, K = 1, min_count 1 and 2, a ray-form and a
              plane-form map, the origin 1 km out, an empty table, rays on the lattice (voxel faces, voxel centres, block faces,
              block corners, negative coordinates), BACK from inside the band, rays beyond every surface, max_range between the
              crossing's two samples, the 7-of-8-corner cell, a start ON an exact zero, zero and NaN directions, rays that leave
              the 21 bits.  The sorted export is unchanged by the block build and the cast; a block set that overflowed is none.
  plumbing    the same bytes twice and from one replay of a captured graph; guard bytes round the block buffer and the three
              outputs; no host synchronisation; the cache of block sets and what drops it; a block set too small makes check()
              raise; an unallocated map gives MISS everywhere.
  answers     the tilted plane, the sphere, the wall seen through and render -> register on the three patches, with the host
              test's bounds; render's frame (count, ray indices, rows, normals) and TsdfTracker.predicted.
Everything observed goes to test_logs/tsdf_raycast.log.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_raycast_cases as RC  # noqa: E402
import tsdf_raycast_restated as T  # noqa: E402
import tsdf_register_restated as RR  # noqa: E402
import test_tsdf_raycast_host as HH  # noqa: E402
from tsdf_raycast_cases import log  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
NAMES = ("range", "normals", "flag")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_map(c, **kw):
    from deeppointmap_amd.tsdf import TsdfMap
    m = c.map
    if c.distance == "plane":
        kw["cos_min"] = m.cos_min
    return TsdfMap(m.voxel, m.truncation, m.step, m.cap_vox, m.min_range, m.max_range, origin=m.origin, device=DEV, distance=c.distance, **kw)


def gpu_build(c, **kw):
    """the case's map on the GPU: its frames fused, or its hand-written table uploaded (an empty case: an empty table)"""
    m = gpu_map(c, **kw)
    m._ready(torch.device(DEV))
    if hasattr(c, "exported"):
        m.table.copy_(dev(RC.table_bytes(c.exported, c.map.cap_vox)))
        m._blocks = {}
    for f, (xyz, count, pose) in enumerate(c.map.frames):
        count = len(xyz) if count is None else count
        m.integrate(dev(xyz), pose, length=count, normals=dev(c.map.normals[f][:len(xyz)]) if c.distance == "plane" else None)
    return m


def gpu_cast(m, c, skip):
    out = m.raycast(c.poses, c.dirs, c.lo, c.hi, c.step, c.min_count, skip=skip)
    assert out.range.shape == (len(c.poses), len(c.dirs)) and out.normals.shape == (len(c.poses), len(c.dirs), 3)
    assert out.flag.shape == out.range.shape and out.flag.dtype == torch.int32 and out.range.dtype == out.normals.dtype == torch.float32
    return tuple(t.cpu().numpy() for t in out)


def same(got, want, what):
    for x, y, name in zip(got, want, NAMES):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name, x.dtype, y.dtype, x.shape, y.shape)
        if x.tobytes() != y.tobytes():
            bad = np.argwhere(x.view(np.uint32 if name != "flag" else np.int32) != y.view(np.uint32 if name != "flag" else np.int32))
            raise AssertionError((what, name, len(bad), bad[:4].tolist(), x[tuple(bad[0])], y[tuple(bad[0])]))


# ---------------------------------------------------------------------------------------------------------------------- bytes
@pytest.mark.parametrize("name", sorted(RC.cast_cases()))
def test_the_cast_is_the_restatement_byte_for_byte_with_the_block_set_and_without(name):
    c = RC.cast_cases()[name]
    m = gpu_build(c).check()
    exp = m.export()
    if hasattr(c, "exported"):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(exp, c.exported))
    want = RC.restated(c, exp)
    plain, skipped = gpu_cast(m, c, False), gpu_cast(m, c, True)
    same(plain, want, f"{name}: blocks = NULL against the restatement")
    same(skipped, plain, f"{name}: with the block set against blocks = NULL")
    m.check()                                                      # reads the block set's overflow word too
    assert all(a.tobytes() == b.tobytes() for a, b in zip(m.export(), exp)), "the block build or the cast wrote the table"
    f = want[2]
    log(f"gpu raycast {name}: {f.shape[0]} poses x {f.shape[1]} rays, {len(exp[0])} voxels: HIT {int((f == 1).sum())}, BACK {int((f == 2).sum())}, "
        f"MISS {int((f == 0).sum())}; all bytes equal, with the block set and without")


# ------------------------------------------------------------------------------------------------------------------- plumbing
def test_the_same_bytes_twice_from_a_captured_graph_and_inside_guard_bytes():
    from deeppointmap_amd import _lib, ops
    c = RC.cast_cases()["poses3"]
    m = gpu_build(c).check()
    want = RC.restated(c, m.export())
    F, R, guard = len(c.poses), len(c.dirs), 256
    poses, dirs = dev(c.poses), dev(c.dirs)
    nb = _lib.load().dpm_tsdf_blocks_bytes(m.max_blocks)
    held = [torch.full((n + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV) for n in (nb, 4 * F * R, 12 * F * R, 4 * F * R)]
    blocks = held[0][guard:guard + nb]
    outs = (held[1][guard:-guard].view(torch.float32).view(F, R), held[2][guard:-guard].view(torch.float32).view(F, R, 3),
            held[3][guard:-guard].view(torch.int32).view(F, R))

    def work():
        ops.tsdf_blocks(m.table, m.max_voxels, 1, m.max_blocks, out=blocks)
        ops.tsdf_raycast(*m._map(), blocks, m.max_blocks, poses, dirs, c.lo, c.hi, c.step, 1, out=outs)

    def check(what):
        torch.cuda.synchronize()
        same(tuple(t.cpu().numpy() for t in outs), want, what)
        for h in held:
            assert bool((h[:guard] == 0xA5).all()) and bool((h[-guard:] == 0xA5).all()), what
        assert int(blocks[:4].view(torch.int32).item()) == 0
    work()
    check("once")
    first = blocks.clone()
    work()
    check("twice")
    members = lambda b: np.sort(b[256:].view(torch.int64).cpu().numpy())       # the slots are not defined, the membership is
    assert (members(blocks) == members(first)).all()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        work()
    for t in outs:
        t.zero_()
    blocks.zero_()                  # not a set any more: the replay has to make it one
    graph.replay()
    check("replayed from a captured graph")
    assert (members(blocks) == members(first)).all()
    n_blocks = int((members(first) != -1).sum())
    log(f"gpu raycast plumbing: {n_blocks} occupied blocks of {len(m.export()[0])} voxels; identical bytes once, twice and from a replayed "
        f"graph; {guard} guard bytes round the block set and the three outputs intact")


def test_the_cast_makes_no_host_synchronisation_and_the_block_sets_are_cached_until_a_write():
    from deeppointmap_amd import augment
    c = RC.cast_cases()["poses3"]
    m = gpu_build(c).check()
    model = RC.render_model()
    poses, dirs = dev(c.poses), dev(c.dirs)
    m.raycast(poses[0], model, skip=False)                              # the model's direction table is uploaded at its first use
    assert m._blocks == {}
    torch.cuda.synchronize()
    before = augment.host_syncs()
    torch.cuda.set_sync_debug_mode("error")      # any synchronising torch call raises
    try:
        a = m.raycast(poses, dirs, c.lo, c.hi, c.step)                  # builds the block set on the way
        b = m.raycast(poses[0], dirs, c.lo, c.hi, c.step, min_count=2, skip=True)
        m.raycast(poses, dirs, c.lo, c.hi, c.step, skip=False)
        m.render(poses[0], model)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert augment.host_syncs() == before
    assert sorted(m._blocks) == [1, 2] and m.blocks(1) is m.blocks(1) and b.range.shape == (1, len(c.dirs))
    same(tuple(t.cpu().numpy() for t in a), RC.restated(c, m.export()), "inside the guarded region")
    n = augment.host_syncs()
    m.check()
    assert augment.host_syncs() == n + 3                                 # the table's word and one per cached set
    xyz, count, pose = c.map.frames[0]
    for write in (lambda: m.integrate(dev(xyz), pose, length=count), lambda: m.carve(dev(xyz), pose, length=count)):
        m.blocks(1)
        assert m._blocks
        write()
        assert m._blocks == {}


def test_a_block_set_that_is_too_small_makes_check_raise_and_an_unallocated_map_misses_everywhere():
    from deeppointmap_amd.tsdf import MISS, TsdfMap
    c = RC.cast_cases()["poses3"]
    m = gpu_build(c, max_blocks=2).check()
    m.raycast(c.poses, c.dirs, c.lo, c.hi, c.step)
    with pytest.raises(ValueError, match="max_blocks=2"):
        m.check()
    same(gpu_cast(m, c, False), RC.restated(c, m.export()), "the plain form does not read the set")
    out = TsdfMap(device=DEV).raycast(c.poses, c.dirs)
    assert out.flag.shape == (3, 257) and int((out.flag != MISS).sum()) == 0 and float(out.range.abs().sum()) == 0.0
    assert float(out.normals.abs().sum()) == 0.0 and out.range.is_cuda


# -------------------------------------------------------------------------------------------------------------------- answers
@pytest.mark.parametrize("tilt", HH.H.TILTS)
def test_tilted_plane_known_answer_on_the_gpu(tilt):
    """Observed on an MI355X (profiles/tsdf_raycast_accuracy.md): the host test's figures, the tables being the same bytes."""
    cc = RC.tilted_cast(tilt)
    m = gpu_build(cc).check()
    rng, _, flag = gpu_cast(m, cc, True)
    HH.tilted_report("gpu", tilt, cc, rng[0], flag[0])


@pytest.mark.parametrize("which", [0, 1])
def test_sphere_known_answer_on_the_gpu(which):
    cc = HH.sphere_yardstick(which)[0]
    m = gpu_build(cc).check()
    rng, nrm, flag = gpu_cast(m, cc, True)
    HH.sphere_report("gpu", which, rng[0], nrm[0], flag[0])


def test_wall_seen_through_known_answer_on_the_gpu():
    cc = RC.walls_cast()
    m = gpu_build(cc).check()
    before = gpu_cast(m, cc, True)
    xyz, count, pose = cc.map.frames[1]
    m.carve(dev(xyz), pose, length=count, weight=2)
    after = gpu_cast(m, cc, True)                                           # the carve dropped the cached block set
    same(after, gpu_cast(m, cc, False), "after the carve: with the block set against blocks = NULL")
    HH.walls_seen_report("gpu", cc, (before[0][0], before[2][0]), (after[0][0], after[2][0]))


def test_render_then_register_on_the_three_patches_and_the_predicted_scan():
    from deeppointmap_amd.tsdf import HIT, TsdfMap, TsdfTracker
    c = RR.patches_case()
    model = RC.render_model()
    pose, start = HH.patches_poses(c)
    m = TsdfMap(c.voxel, max_voxels=1 << 16, origin=c.origin, device=DEV, distance="plane")
    m.integrate(dev(c.xyz), c.pose, normals=dev(c.normals)).check()
    pcd, normals = m.render(pose, model, min_count=1 / 256)
    cast = m.raycast(pose, model, min_count=1 / 256)
    hit = (cast.flag[0] == HIT).cpu().numpy()
    n = int(pcd.count.item())
    dirs = model.directions()
    assert n == int(hit.sum()) and pcd.xyz.shape == (model.rays, 3) and normals.shape == (model.rays, 3)
    assert (pcd.idx[:n].cpu().numpy() == np.flatnonzero(hit)).all()                       # compacted in ray order; idx = the ray
    want_xyz = (torch.from_numpy(dirs).to(DEV) * cast.range[0][:, None]).cpu().numpy()[hit]
    assert pcd.xyz[:n].cpu().numpy().tobytes() == want_xyz.tobytes()
    assert normals[:n].cpu().numpy().tobytes() == cast.normals[0].cpu().numpy()[hit].tobytes() and float(normals[n:].abs().sum()) == 0.0
    assert np.allclose(pcd.R.numpy(), pose[:3, :3], atol=1e-6) and np.allclose(pcd.T.numpy()[:, 0], pose[:3, 3], atol=1e-6)
    res = m.register(pcd, start, ((3 * c.voxel, 30),), min_count=1 / 256)
    got, status, its = res.pose[0].cpu().numpy(), int(res.status.item()), int(res.iterations.item())
    dt, dr = RR.pose_error(got, pose)
    log(f"gpu raycast three patches: {n} HIT of {model.rays} rendered rays; registered from 0.35 m / 2 degrees off: status {status}, {its} "
        f"iterations, back to the rendering pose within {dt:.3e} m and {dr:.3e} (bounds 1e-4)")
    assert n > 300 and status == RR.CONVERGED and dt <= 1e-4 and dr <= 1e-4
    # the rendered frame is fused as it is: the plane form takes its normals in the sensor frame
    again = TsdfMap(c.voxel, max_voxels=1 << 16, origin=c.origin, device=DEV, distance="plane").integrate(pcd, pose, normals=normals).check()
    assert len(again.export()[0]) > 1000
    # ... described by ScanContext, and run through a transform chain on side streams
    from deeppointmap_amd import augment
    from deeppointmap_amd.loop_closure import ScanContext
    raw, norm, mask = ScanContext(max_range=12.0, z_offset=3.0).describe(pcd)
    assert int(mask.item()) != 0 and bool(torch.isfinite(norm).all()) and float(raw.max()) > 0
    fresh, _ = m.render(pose, model, min_count=1 / 256)
    out = augment.transform_frames([fresh], augment.DistanceSample(1.0, 5.5))
    torch.cuda.synchronize()
    kept = out[0].nbr_point
    rng = np.linalg.norm(want_xyz, axis=1)
    assert kept == int(((rng >= 1.0) & (rng <= 5.5)).sum()) and 0 < kept < n
    # the tracker's predicted scan: render at the constant-velocity prediction
    tr = TsdfTracker(c.voxel, max_voxels=1 << 16, origin=c.origin, device=DEV, distance="plane", min_count=1 / 256)
    tr.step(dev(c.xyz), normals=dev(c.normals), pose=c.pose)
    p1, n1 = tr.predicted(model)
    p2, n2 = tr.map.render(c.pose, model, min_count=1 / 256)
    k = int(p1.count.item())
    assert k == int(p2.count.item()) > 300 and p1.xyz[:k].cpu().numpy().tobytes() == p2.xyz[:k].cpu().numpy().tobytes()
    assert n1[:k].cpu().numpy().tobytes() == n2[:k].cpu().numpy().tobytes() and len(tr.poses) == 1
