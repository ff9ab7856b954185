"""GPU: the indexed, tile-owned extraction (csrc/tsdf_map.hip: dpm_tsdf_mesh_indexed, dpm_tsdf_surface_tiles) and meshing beyond
the table (deeppointmap_amd/tsdf.py: mesh_indexed, surface(tiles=), merged_mesh, merged_surface; GeometricSlam.surface_map with
an archive; DESIGN §7l "Meshing beyond the table"), byte for byte against `mesh()`, `surface()` and tests/tsdf_mesh_restated.py.
tests/test_tsdf_mesh_host.py shows the host side on the CPU.  Every map has at most 2^16 slots; tiles are 8 voxels a side.

  indexed     mesh_indexed equals mesh() and the restatement on wall, lattice and sphere at min_count 1 and 3 and on a 6 x 6 x 6
              block of constructed records that meets every tetrahedron case and every missing-corner exit; the same bytes a
              second time and with the frames, rows or records in reversed order.
  key ends    that block against either end of the 21 bits, where a cell's corners and a normal's neighbours leave the keys:
              mesh_indexed, mesh(), surface() and surface(tiles=) equal the restatements, byte for byte, in either record order.
  normals     on axis edges surface()'s bytes; unit or zero; the restatement's float32 bytes; within max(3 |r32 - r64|, 1e-6) of
              its float64 form.
  ownership   single-tile calls partition the sphere's mesh and surface: counts add up, merged they are the whole, byte for byte.
  rolled      merged_mesh / merged_surface of a rolled sphere in 6 batches equal the unrolled table's; closed, oriented, euler 2.
  max_out     below V or below F both counts are reported and nothing is written beyond.
  syncs       mesh_indexed synchronises once.
  slam        surface_map(archive=) then merged_export equals the unrolled surface_map's export, with and without carve.
Everything observed goes to test_logs/tsdf_mesh.log.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_cases as C  # noqa: E402
import tsdf_mesh_restated as MR  # noqa: E402
import tsdf_restated as R  # noqa: E402
from test_tsdf_host import fuse  # noqa: E402
from test_tsdf_mesh_host import BLOCK_ENDS, B, block_restated, log, same  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("vertices", "faces", "normals", "vertex_keys", "vertex_dirs")


def case(name):
    return C.sphere() if name == "sphere" else C.single_frame_cases()[name]


@functools.lru_cache(maxsize=None)
def exported(name):
    return fuse(case(name)).export()


@functools.lru_cache(maxsize=None)
def restated(name, min_count):
    """(vertices, faces, normals, keys, dirs) of the restated field's mesh: computed once, never written to"""
    return MR.indexed(R.field(exported(name), min_count), case(name).voxel)


def gpu_map(c, cap_vox=None):
    from deeppointmap_amd.tsdf import TsdfMap
    return TsdfMap(c.voxel, c.truncation, c.step, c.cap_vox if cap_vox is None else cap_vox, c.min_range, c.max_range,
                   origin=c.origin, device=DEV)


def gpu_fuse(c, backwards=False):
    """backwards: the frames in reversed order and the rows of each reversed -- other slots, the same voxels"""
    m = gpu_map(c)
    for xyz, count, pose in (c.frames[::-1] if backwards else c.frames):
        rows = np.ascontiguousarray(xyz[:count][::-1] if backwards else xyz[:count])
        m.integrate(torch.from_numpy(rows).to(DEV), pose)
    return m.check()


def host(mesh):
    return tuple(t.cpu().numpy() for t in mesh)


def typed(mesh):
    v, f, n, k, d = mesh
    return (v.dtype, f.dtype, n.dtype, k.dtype, d.dtype) == (np.float32, np.int32, np.float32, np.int64, np.int32) and \
        v.shape == n.shape == (len(k), 3) and f.shape[1:] == (3,) and d.shape == k.shape


@functools.lru_cache(maxsize=None)
def sphere_on_gpu():
    """the sphere fused once, with its whole indexed mesh and surface on the host: read by several tests, written by none"""
    m = gpu_fuse(C.sphere())
    s = m.surface()
    return m, host(m.mesh_indexed()), (s.keys.cpu().numpy(), s.axes.cpu().numpy(), s.xyz_map.cpu().numpy(), s.normals.cpu().numpy(),
                                        s.xyz.cpu().numpy())


# -------------------------------------------------------------------------------------------------------------------- indexed
@pytest.mark.parametrize("name,min_count", [("wall", 1), ("wall", 3), ("lattice", 1), ("lattice", 3), ("sphere", 1), ("sphere", 3)])
def test_mesh_indexed_is_mesh_and_the_restatement_byte_for_byte(name, min_count):
    c, want = case(name), restated(name, min_count)
    m = gpu_fuse(c)
    got = host(m.mesh_indexed(min_count))
    vertices, faces = m.mesh(min_count)
    assert typed(got) and same(got[:2], (vertices, faces)), (name, "mesh()")
    for x, y, what in zip(got, want, FIELDS):
        differ = -1 if x.shape != y.shape else int((x != y).sum())
        log(f"gpu indexed '{name}' min_count {min_count}: {what}: {len(x)} rows, {differ} entries differ from the restatement (-1: shapes)")
        assert same((x,), (y,)), (name, what)
    assert same(host(m.mesh_indexed(min_count)), got), (name, "a second time")
    assert same(host(gpu_fuse(c, backwards=True).mesh_indexed(min_count)), got), (name, "fused backwards")
    assert len(got[1]) > 0 or name == "lattice"


def test_a_block_of_constructed_records_meets_every_case():
    """195 of the 216 voxels of a 6 x 6 x 6 block, 21 of them with one sample (unqualified at min_count 2), four with D == 0:
    all 14 mixed sign patterns of a tetrahedron under both parities, and cells that leave at each of the corners 1 .. 7"""
    from deeppointmap_amd.tsdf import TsdfMap
    keys, sums, counts = MR.block_records(0)
    order = np.argsort(keys)
    fld = R.field((keys[order], sums[order], counts[order]), 2)
    cases, exits = MR.block_coverage(fld)
    assert {p for p, _ in cases} >= set(range(1, 15)) and len({x for x in cases if x[0] not in (0, 15)}) == 28 and exits == set(range(1, 8))
    assert 0.15 <= 1 - len(fld[0]) / 216 <= 0.25 and bool((fld[1] == 0).any())
    want = MR.indexed(fld, 0.5)
    got = []
    for k, s, n in ((keys, sums, counts), (keys[::-1], sums[::-1], counts[::-1])):
        m = TsdfMap(0.5, max_voxels=1 << 10, origin=np.zeros(3), device=DEV).absorb(k.copy(), s.copy(), n.copy()).check()
        got.append(host(m.mesh_indexed(2)))
        assert typed(got[-1]) and same(got[-1][:2], m.mesh(2))
        assert same(host(m.mesh_indexed(2)), got[-1])
    assert same(got[0], got[1]) and same(got[0], want)
    log(f"gpu indexed block: {len(keys)} records, {len(fld[0])} qualified, {len(cases)} (pattern, parity) cases, exits at corners "
        f"{sorted(exits)}: {len(want[0])} vertices, {len(want[1])} faces: mesh() and the restatement, byte for byte, in either order")
    assert len(want[1]) > 20


@pytest.mark.parametrize("corner", BLOCK_ENDS)
def test_the_block_at_either_end_of_the_keys(corner):
    """the cells and crossings whose neighbours would lie past coordinate 2^21 - 1, or below 0, on a table of 1024 slots"""
    from deeppointmap_amd import tsdf
    (keys, sums, counts), want, surf = block_restated(corner)
    tiles = np.unique(tsdf.tile_of(keys, B))
    got = []
    for k, s, n in ((keys, sums, counts), (keys[::-1], sums[::-1], counts[::-1])):
        m = tsdf.TsdfMap(0.5, max_voxels=1 << 10, origin=np.zeros(3), device=DEV).absorb(k.copy(), s.copy(), n.copy()).check()
        got.append(host(m.mesh_indexed(2)))
        for x, y, what in zip(got[-1], want, FIELDS):
            log(f"gpu block at {corner}: {what}: {len(x)} rows, {-1 if x.shape != y.shape else int((x != y).sum())} entries differ from "
                f"the restatement (-1: shapes)")
        assert typed(got[-1]) and same(got[-1], want) and same(m.mesh(2), want[:2])
        whole, owned = m.surface(2), m.surface(2, tiles=tiles, tile_bits=B)
        rows = (whole.keys, whole.axes, whole.xyz_map.t().contiguous(), whole.normals.t().contiguous())
        for x, y, what in zip(host(rows), surf, ("keys", "axes", "positions", "normals")):
            log(f"gpu block at {corner}: surface {what}: {len(x)} rows, {-1 if x.shape != y.shape else int((x != y).sum())} entries "
                f"differ from the restatement (-1: shapes)")
            assert same((x,), (y,)), what
        assert same(host((owned.keys, owned.axes, owned.xyz_map, owned.normals, owned.xyz)),
                    host((whole.keys, whole.axes, whole.xyz_map, whole.normals, whole.xyz)))
        assert m.outside() == 0 and m.overflow() == 0
    assert same(got[0], got[1]) and len(want[1]) > 20 and len(surf[0]) > 20 and len(tiles) >= 1
    log(f"gpu block at {corner}: {len(want[0])} vertices, {len(want[1])} faces, {len(surf[0])} crossings in {len(tiles)} tiles: "
        f"mesh_indexed, mesh(), surface() and surface(tiles=) are the restatements, byte for byte, in either order")


# -------------------------------------------------------------------------------------------------------------------- normals
@pytest.mark.parametrize("name,min_count", [("wall", 1), ("sphere", 1), ("sphere", 3)])
def test_vertex_normals(name, min_count):
    c = case(name)
    m = sphere_on_gpu()[0] if name == "sphere" else gpu_fuse(c)
    v, f, n, k, d = host(m.mesh_indexed(min_count))
    s = m.surface(min_count)
    at = {(key, axis): i for i, (key, axis) in enumerate(zip(s.keys.cpu().numpy().tolist(), s.axes.cpu().numpy().tolist()))}
    sn = np.ascontiguousarray(s.normals.t().cpu().numpy())
    axis = np.flatnonzero(d < 3)
    rows = [at[(int(k[i]), int(d[i]))] for i in axis]           # a KeyError: a vertex on an axis edge that surface() does not have
    assert len(at) >= len(axis) > 0 and n[axis].tobytes() == sn[rows].tobytes()      # surface() also has crossings outside whole cells
    length = np.linalg.norm(n.astype(np.float64), axis=1)
    zero = (n == 0).all(axis=1)
    # unit: three correctly rounded quotients by a length that is itself off by a few ulp of fp32 -- 1e-6 is 8 ulp of 1
    assert bool((zero | (np.abs(length - 1) <= 1e-6)).all())
    r32 = restated(name, min_count)[2]
    r64 = MR.vertex_normals(R.field(exported(name), min_count, np.float64), k, d, np.float64)
    bound = np.maximum(3 * np.abs(r32.astype(np.float64) - r64), 1e-6)
    err = np.abs(n.astype(np.float64) - r64)
    log(f"gpu normals '{name}' min_count {min_count}: {len(n)} vertices, {len(axis)} on axis edges equal surface()'s bytes; {int(zero.sum())} "
        f"zero, | |n| - 1 | <= {np.abs(length[~zero] - 1).max():.2e}; against float64 max {err.max():.3e} (largest bound "
        f"{bound.max():.3e}, smallest margin {(bound - err).min():.3e}); {int((n != r32).sum())} entries differ from the float32 form")
    assert bool((err <= bound).all()) and len(axis) > 0 and int((d >= 3).sum()) > 0


# ------------------------------------------------------------------------------------------------------------------ ownership
def test_single_tile_calls_partition_the_mesh_and_the_surface():
    from deeppointmap_amd import tsdf
    m, whole, surf = sphere_on_gpu()
    keys = exported("sphere")[0]
    tiles = np.unique(tsdf.tile_of(keys, B))
    x = MR.coords(tiles)
    assert all(len(set(x[:, a].tolist())) >= 3 for a in range(3))             # tile boundaries are crossed on all three axes
    held = set(keys.tolist())
    last = MR.coords(keys)
    last = last[((last & 7) == 7).all(axis=1)]                                # cells whose 8 corners lie in 8 tiles
    meet = [c for c in last if all(int(MR.pack(c + [g & 1, (g >> 1) & 1, g >> 2])[0]) in held for g in range(8))]
    assert meet, "no point of the sphere's band where 8 tiles meet"
    parts, faces, records, counts = [], 0, [], 0
    for t in tiles:
        one = host(m.mesh_indexed(tiles=[t], tile_bits=B))
        assert typed(one)
        base = MR.base_keys(one[3][one[1]]) if len(one[1]) else np.zeros(0, np.int64)
        assert bool((tsdf.tile_of(base, B) == t).all())                        # every face comes from a cell of this tile
        parts.append(one)
        faces += len(one[1])
        s = m.surface(tiles=[t], tile_bits=B)
        assert bool((tsdf.tile_of(s.keys.cpu().numpy(), B) == t).all())
        records.append(s)
        counts += len(s.keys)
    assert faces == len(whole[1]) and counts == len(surf[0])
    assert same(tsdf.weld_indexed(parts), whole)
    together = host(m.mesh_indexed(tiles=torch.from_numpy(tiles[::-1].copy()), tile_bits=B))      # all of them, unsorted, as a tensor
    assert same(together, whole)
    k, a = np.concatenate([s.keys.cpu().numpy() for s in records]), np.concatenate([s.axes.cpu().numpy() for s in records])
    order = np.lexsort((a, k))
    for j, field in enumerate(("xyz_map", "normals", "xyz")):
        got = np.concatenate([getattr(s, field).cpu().numpy() for s in records], axis=1)[:, order]
        assert got.tobytes() == surf[2 + j].tobytes(), field
    assert k[order].tobytes() == surf[0].tobytes() and a[order].tobytes() == surf[1].tobytes()
    absent = MR.pack([[5, 5, 5]])                                             # a tile far from the band
    assert absent[0] not in tiles
    empty = host(m.mesh_indexed(tiles=absent, tile_bits=B))
    assert typed(empty) and len(empty[0]) == 0 and len(empty[1]) == 0 and m.surface(tiles=absent, tile_bits=B).keys.numel() == 0
    with pytest.raises(ValueError):
        m.mesh_indexed(tiles=[], tile_bits=B)
    seams = sum(len(p[3]) for p in parts) - len(whole[0])
    log(f"gpu ownership: {len(tiles)} tiles, 8 of them meet at {len(meet)} cells: faces {faces} = F, {seams} vertices named in two "
        f"tiles, merged {len(whole[0])} vertices the whole mesh byte for byte; surface records {counts} = M, byte for byte; an absent "
        f"tile gives nothing")


# --------------------------------------------------------------------------------------------------------------------- rolled
def test_a_rolled_sphere_meshes_as_the_table_that_never_rolled():
    """the sphere's rays in four frames with a roll after each, the window's centre moving round the sphere with radii (1.0,
    1.5 m) far below `reach`, so that most tiles are on the host in the end: integrate alone is exact under any radii"""
    from deeppointmap_amd import tsdf
    c = C.sphere()
    m0, whole, surf = sphere_on_gpu()
    xyz, count, pose = c.frames[0]
    m, archive = gpu_map(c), tsdf.TsdfArchive(B)
    for i, centre in enumerate(([2.5, 0, 0], [0, -2.5, 0], [0, 0, 2.5], [-2.5, 1.0, 0.5])):
        at = np.eye(4)
        at[:3, 3] = centre
        m.integrate(torch.from_numpy(np.ascontiguousarray(xyz[i::4])).to(DEV), pose)
        m.roll(at, archive, keep_radius=1.5, load_radius=1.0)
    assert m.check().overflow() == 0 and same(tsdf.merged_export(m, archive), exported("sphere"))
    on_device, on_host = len(m.export()[0]), len(archive)
    assert on_host > on_device > 0
    table, records = m.table.clone(), [a.copy() for a in archive.records()]
    scratch = 1 << 13
    batches = tsdf.plan_batches(tsdf.records_by_tile(*tsdf.merged_export(m, archive), B), B, scratch)
    assert len(batches) >= 4
    v, f, n = tsdf.merged_mesh(m, archive, scratch_voxels=scratch)
    assert same((v, f), m0.mesh()) and same((v, f, n), whole[:3])
    s = tsdf.merged_surface(m, archive, scratch_voxels=scratch)
    assert not s.keys.is_cuda and np.array_equal(s.origin, c.origin)
    assert same((s.keys.numpy(), s.axes.numpy(), s.xyz_map.numpy(), s.normals.numpy(), s.xyz.numpy()), surf)
    top = R.topology(f)
    assert top["closed"] and top["oriented"] and top["euler"] == 2 and R.signed_volume(v, f) < 0       # seen from inside
    assert torch.equal(m.table, table) and same(archive.records(), records)
    alone = tsdf.merged_mesh(m0, None, scratch_voxels=scratch)                   # no archive: the table alone, in batches
    assert same(alone, whole[:3])
    log(f"gpu rolled sphere: {on_device} voxels on the device, {on_host} in the archive, {len(batches)} batches at scratch {scratch}: "
        f"{len(v)} vertices, {len(f)} faces, {s.keys.numel()} surface records: the unrolled table's bytes; closed, oriented, euler "
        f"{top['euler']}; table and archive untouched")


# -------------------------------------------------------------------------------------------------------------------- max_out
def test_max_out_below_v_or_below_f_reports_both_counts_and_writes_nothing_beyond():
    from deeppointmap_amd import _lib, ops
    c = C.wall()
    m = gpu_fuse(c)
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    V, F = ops.tsdf_mesh_indexed(m.table, m.max_voxels, c.voxel, 1, max_out=(0, 0))
    whole = ops.tsdf_mesh_indexed(m.table, m.max_voxels, c.voxel, 1)
    assert (V, F) == whole[0] == (len(restated("wall", 1)[0]), len(restated("wall", 1)[1])) and V > 8 and F > 8
    for nv, nf in ((V // 2, F), (V, F // 2), (V // 2, F // 2), (V + 5, F + 5), (0, F), (V, 0)):
        counts, *out = ops.tsdf_mesh_indexed(m.table, m.max_voxels, c.voxel, 1, max_out=(nv, nf))
        assert counts == (V, F) and [len(t) for t in out] == [min(nv, V)] * 4 + [min(nf, F)], (nv, nf)
    work = torch.empty(lib.dpm_tsdf_mesh_indexed_bytes(m.max_voxels), dtype=torch.uint8, device=DEV)
    for nv, nf in ((V // 2, F), (V, F // 2)):
        counts = torch.full((2,), -7, dtype=torch.int32, device=DEV)              # zeroed by the call
        vk, vd = torch.full((V,), -7, dtype=torch.int64, device=DEV), torch.full((V,), -7, dtype=torch.int32, device=DEV)
        xyz, nrm = torch.full((V, 3), -7.0, device=DEV), torch.full((V, 3), -7.0, device=DEV)
        faces = torch.full((F, 3), -7, dtype=torch.int32, device=DEV)
        _lib.check(lib.dpm_tsdf_mesh_indexed(m.table.data_ptr(), m.max_voxels, c.voxel, 1, B, None, 0, vk.data_ptr(), vd.data_ptr(),
                                             xyz.data_ptr(), nrm.data_ptr(), faces.data_ptr(), counts.data_ptr(), nv, nf,
                                             work.data_ptr(), st), "dpm_tsdf_mesh_indexed")
        assert counts.tolist() == [V, F]
        assert bool((vk[nv:] == -7).all() & (vd[nv:] == -7).all() & (xyz[nv:] == -7).all() & (nrm[nv:] == -7).all() & (faces[nf:] == -7).all())
        assert bool((vd[:nv] >= 0).all() & (vd[:nv] < 7).all() & (faces[:nf] >= 0).all() & (faces[:nf] < V).all())
    log(f"gpu max_out: V {V}, F {F} reported with half the room for either, nothing written past it")


# ---------------------------------------------------------------------------------------------------------------------- syncs
def test_mesh_indexed_synchronises_once():
    from deeppointmap_amd import augment
    m = sphere_on_gpu()[0]
    tiles = np.unique(MR.tile_of(exported("sphere")[0], B))[:7]
    torch.cuda.synchronize()
    for call in (lambda: m.mesh_indexed(), lambda: m.mesh_indexed(2, tiles=tiles, tile_bits=B), lambda: m.surface(tiles=tiles[:1], tile_bits=B)):
        before = augment.host_syncs()
        call()
        assert augment.host_syncs() == before + 1


# ----------------------------------------------------------------------------------------------------------------------- slam
def test_surface_map_with_an_archive_merges_to_the_unrolled_export():
    """the first 12 poses of the loop-closure test's two laps (4 m apart), chunks of poses within 5 m: six chunks, and tiles of 4 m
    with a reach of 15 m, so the first chunks' tiles are on the host in the end"""
    from deeppointmap_amd import lidar_sim as LS
    from deeppointmap_amd import tsdf
    from deeppointmap_amd.loop_closure import GeometricSlam
    n = 12
    scene = LS.street_scene(2, blocks=(1, 1))
    model = LS.LidarModel(np.linspace(10.0, -20.0, 16), 256, 0.9, 80.0, range_sigma=0.0, drop_prob=0.0)
    truth = LS.circuit(scene, spacing=4.0, laps=2)[:n]
    frames = LS.LidarSimulator(scene, model, device=DEV).frames(truth)
    slam = GeometricSlam(odometry=dict(max_range=model.max_range, first_pose=truth[0], initial_motion=LS.sweep_delta(truth[0], truth[1]),
                                       sample_map=0.25, sample_register=0.75, metric="plane"),
                         loop=dict(capacity=n, points_per_frame=model.rays, sc=dict(max_range=model.max_range, z_offset=LS.SENSOR_HEIGHT)))
    for f in frames:
        slam.step(f)
    rows = slam.surface_rows()
    span = np.linalg.norm(slam.poses[rows[-1]][:3, 3] - slam.poses[rows[0]][:3, 3])
    assert len(rows) >= 8 and span > 30.0
    kw = dict(truncation=1.0, max_voxels=1 << 16, max_range=10.0, min_range=0.9)
    for carve in (0.0, 1.0):
        plain = slam.surface_map(0.5, carve=carve, **kw)
        archive = tsdf.TsdfArchive(B)
        rolled = slam.surface_map(0.5, carve=carve, archive=archive, slack=5.0, **kw)
        assert plain.overflow() == 0 and rolled.overflow() == 0
        want, got = plain.export(), tsdf.merged_export(rolled, archive)
        assert same(got, want)
        log(f"gpu slam, carve {carve}: {len(rows)} frames over {span:.1f} m: {len(want[0])} voxels, {len(archive)} of them in the archive "
            f"({len(archive.tiles)} tiles), {len(rolled.export()[0])} on the device: merged_export is the unrolled export, byte for byte")
        assert len(archive) > 0 and len(want[0]) > 5000
    v, f, nrm = tsdf.merged_mesh(rolled, archive, min_count=2, scratch_voxels=1 << 15)
    assert same((v, f), plain.mesh(2)) and len(f) > 0
