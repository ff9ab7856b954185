"""CPU: the host side of meshing beyond the table (deeppointmap_amd/tsdf.py: needed_records, plan_batches, weld_indexed; DESIGN
§7l "Meshing beyond the table") against tests/tsdf_mesh_restated.py, on the sphere of tests/tsdf_cases.py cut into tiles of 8
voxels (tile_bits 3, the minimum).

  halo       needed_records equals the brute-force list (per owned base voxel its 64 offsets) for one tile, several, all, and for
             voxels at both ends of the 21 bits, where an offset that leaves them must not wrap into another axis.
  mutants    the restated out-of-core mesh with the contract's halo equals the mesh of the whole field, normals included, and no
             seam vertex comes with two different sets of bytes; with a halo one layer thinner at -1, or at +2, it does not.
  weld       weld_indexed over per-batch indexed meshes equals tsdf.weld of the concatenated soups, byte for byte.
  planner    never more than half the scratch table, every tile exactly once, sorted; a tile too large raises.
  key ends   the constructed 6 x 6 x 6 block placed against either end of the 21 bits restates to the faces, directions, axes and
             normal bytes it has in the middle; only keys and positions move (the yardstick of the GPU test at those placements).
Everything observed goes to test_logs/tsdf_mesh.log.
"""
import functools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_cases as C  # noqa: E402
import tsdf_mesh_restated as MR  # noqa: E402
import tsdf_restated as R  # noqa: E402
from test_tsdf_host import fuse  # noqa: E402

B = 3     # tile_bits: tiles of 8 voxels a side
BLOCK_BASE = (5, -3, 6)
BLOCK_ENDS = ((2 ** 20 - 6,) * 3, (-2 ** 20,) * 3)     # biased coordinates 2097146 .. 2097151 and 0 .. 5: the ends of the 21 bits


def log(line):
    print(line)
    try:
        os.makedirs(os.path.join(ROOT, "test_logs"), exist_ok=True)
        with open(os.path.join(ROOT, "test_logs", "tsdf_mesh.log"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


@pytest.fixture(scope="module")
def sphere():
    """the sphere's export, its tiles, batches of them, the whole field's indexed mesh and each batch's from its needed records"""
    from deeppointmap_amd import tsdf
    c = C.sphere()
    exported = fuse(c).export()
    by_tile = tsdf.records_by_tile(*exported, B)
    batches = tsdf.plan_batches(by_tile, B, 1 << 13)
    parts = [MR.batch_mesh(exported, c.voxel, owners, B) for owners in batches]
    return c, exported, by_tile, batches, MR.indexed(R.field(exported), c.voxel), parts


def same(a, b):
    return all(np.asarray(x).dtype == np.asarray(y).dtype and np.asarray(x).shape == np.asarray(y).shape
               and np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def block_restated(corner):
    """the constructed block (tsdf_mesh_restated.block_records, seed 0) with its first voxel at the unbiased `corner`, at min_count 2
    and voxel 0.5 -> (its records, the restated indexed mesh, the restated surface): computed once, never written to"""
    keys, sums, counts = MR.block_records(0, corner=corner)
    order = np.argsort(keys)
    fld = R.field((keys[order], sums[order], counts[order]), 2)
    return (keys, sums, counts), MR.indexed(fld, 0.5), R.surface(fld, 0.5)


# ----------------------------------------------------------------------------------------------------------------------- halo
def test_tiles_are_the_restatements_and_cover_the_records(sphere):
    from deeppointmap_amd import tsdf
    c, exported, by_tile, _, _, _ = sphere
    assert np.array_equal(tsdf.tile_of(exported[0], B), MR.tile_of(exported[0], B))
    assert sorted(by_tile) == sorted(set(MR.tile_of(exported[0], B).tolist()))
    assert same(tsdf.merge_records(*[np.concatenate(p) for p in zip(*by_tile.values())]), exported)
    x = MR.coords(sorted(by_tile))
    assert all(len(set(x[:, a].tolist())) >= 3 for a in range(3))          # tile boundaries are crossed on all three axes


def test_needed_records_are_the_brute_force_list(sphere):
    from deeppointmap_amd import tsdf
    c, exported, by_tile, batches, _, _ = sphere
    tiles = np.array(sorted(by_tile), np.int64)
    rng = np.random.default_rng(3)
    sets = [tiles[:1], tiles[len(tiles) // 2:len(tiles) // 2 + 1], tiles[rng.permutation(len(tiles))[:5]], batches[1], tiles,
            np.array([tiles[0], MR.pack([[5, 5, 5]])[0]])]        # the last: an owner tile that holds nothing
    for owners in sets:
        got = tsdf.needed_records(by_tile, owners, B)
        want = MR.needed_keys(exported[0], owners, B)
        assert same(got, MR.cut(exported, want)), len(owners)
        own = int(np.isin(MR.tile_of(want, B), owners).sum())
        log(f"host halo: {len(owners)} owner tiles: {own} own voxels + {len(want) - own} halo voxels of {len(exported[0])}: the brute "
            f"force's, byte for byte")
        assert len(owners) == len(tiles) or len(want) - own > 0
    assert len(tsdf.needed_records(by_tile, [MR.pack([[5, 5, 5]])[0]], B)[0]) == 0
    assert len(tsdf.needed_records({}, tiles[:1], B)[0]) == 0


def test_the_halo_does_not_wrap_at_the_ends_of_the_21_bits():
    """voxels within 20 of coordinate 0 and of 2^21 - 1 on every axis: x - 2 below 0 or x + 1 above the last coordinate names no
    voxel, and packed without a clamp it would borrow from the next axis"""
    from deeppointmap_amd import tsdf
    rng = np.random.default_rng(5)
    low, high = rng.integers(0, 20, (300, 3)), MR.AXIS - rng.integers(0, 20, (300, 3))
    mixed = np.where(rng.integers(0, 2, (300, 3)) > 0, rng.integers(0, 20, (300, 3)), MR.AXIS - rng.integers(0, 20, (300, 3)))
    keys = np.unique(MR.pack(np.concatenate([low, high, mixed])))
    exported = (keys, np.arange(len(keys), dtype=np.int64) - 7, np.ones(len(keys), np.uint32))
    by_tile = tsdf.records_by_tile(*exported, B)
    tiles = np.array(sorted(by_tile), np.int64)
    for owners in (tiles[:1], tiles[-1:], tiles[::3], tiles):
        assert same(tsdf.needed_records(by_tile, owners, B), MR.cut(exported, MR.needed_keys(keys, owners, B))), len(owners)
    log(f"host halo at the ends of the keys: {len(keys)} voxels in {len(tiles)} tiles: the brute force's, byte for byte")


# -------------------------------------------------------------------------------------------------------------------- mutants
def test_the_halo_is_needed_one_layer_thinner_on_either_side_fails(sphere):
    c, exported, by_tile, batches, whole, parts = sphere
    assert len(batches) >= 4
    v, f, n, clash = MR.merge(parts)
    assert clash == 0 and same((v, f, n), whole[:3])
    log(f"host merged sphere: {len(batches)} batches: {len(v)} vertices, {len(f)} faces: the whole field's mesh and normals, byte for "
        f"byte; no seam vertex with two sets of bytes")
    want = MR.indexed(R.field(exported), c.voxel, batches[1], B)
    assert same(parts[1], want)
    for lo, hi in ((0, 2), (-1, 1)):
        mv, mf, mn, _, _ = MR.batch_mesh(exported, c.voxel, batches[1], B, lo=lo, hi=hi)
        differ = int((mn.view(np.uint32) != want[2].view(np.uint32)).any(axis=1).sum()) if mn.shape == want[2].shape else -1
        log(f"host merged sphere, MUTANT halo {lo} .. {hi}: {differ} of {len(want[2])} normals of batch 1 differ (-1: another shape)")
        assert not same((mv, mf, mn), want[:3])
        assert same((mv, mf), want[:2]) and differ > 0      # the 8 corners are inside either halo: it is the normals that read further


# ----------------------------------------------------------------------------------------------------------------------- weld
def test_weld_indexed_is_weld_of_the_concatenated_soups(sphere):
    from deeppointmap_amd import tsdf
    c, exported, by_tile, batches, whole, parts = sphere
    want = tsdf.weld(*[np.concatenate(p) for p in zip(*[MR.soup(p) for p in parts])])
    rng = np.random.default_rng(9)
    shuffled = []
    for v, f, n, k, d in parts:                       # a batch's own order is no canonical one: slots
        p = rng.permutation(len(k))
        inv = np.empty_like(p)
        inv[p] = np.arange(len(p))
        shuffled.append((v[p], inv[f][rng.permutation(len(f))][:, [1, 2, 0]].astype(np.int32), n[p], k[p], d[p]))
    for what, given in (("sorted", parts), ("shuffled", shuffled), ("with an empty batch", parts[:1] + [tuple(a[:0] for a in parts[0])] + parts[1:])):
        got = tsdf.weld_indexed(given)
        assert same(got[:2], want), what
        assert same((got[0], got[1], got[3], got[4]), (whole[0], whole[1], whole[3], whole[4])), what
        assert got[2].shape == got[0].shape and got[2].dtype == np.float32
    seams = sum(len(p[3]) for p in parts) - len(want[0])
    log(f"host weld: {len(parts)} batches, {len(want[0])} vertices ({seams} came from two batches), {len(want[1])} faces: weld of the "
        f"concatenated soups, byte for byte")
    assert seams > 0
    empty = tsdf.weld_indexed([])
    assert [a.shape for a in empty] == [(0, 3), (0, 3), (0, 3), (0,), (0,)] and empty[1].dtype == np.int32


# -------------------------------------------------------------------------------------------------------------------- planner
@pytest.mark.parametrize("scratch", [1 << 12, 1 << 13, 1 << 14, 1 << 16])
def test_the_planner_keeps_to_half_the_scratch_and_covers_every_tile_once(sphere, scratch):
    from deeppointmap_amd import tsdf
    c, exported, by_tile, _, _, _ = sphere
    batches = tsdf.plan_batches(by_tile, B, scratch)
    flat = np.concatenate(batches)
    assert flat.tolist() == sorted(by_tile)                                       # every tile once, in sorted order
    sizes = [len(MR.needed_keys(exported[0], owners, B)) for owners in batches]
    log(f"host planner: scratch {scratch}: {len(batches)} batches of {[len(b) for b in batches]} tiles needing {sizes} voxels")
    assert max(sizes) <= scratch // 2
    assert all(b.dtype == np.int64 and b.tolist() == sorted(b.tolist()) for b in batches)
    if scratch == 1 << 16:
        assert len(batches) == 1


def test_a_tile_too_large_for_the_scratch_raises(sphere):
    from deeppointmap_amd import tsdf
    c, exported, by_tile, _, _, _ = sphere
    biggest = max(len(MR.needed_keys(exported[0], [t], B)) for t in by_tile)
    with pytest.raises(ValueError, match="scratch_voxels"):
        tsdf.plan_batches(by_tile, B, 2 * biggest - 2)
    assert tsdf.plan_batches(by_tile, B, 2 * biggest)
    assert tsdf.plan_batches({}, B, 64) == []


# ------------------------------------------------------------------------------------------------------------------- key ends
@pytest.mark.parametrize("corner", BLOCK_ENDS)
def test_the_block_at_either_end_of_the_keys_restates_as_in_the_middle(corner):
    """A placement moves every key by one offset and nothing else: a voxel past either end of the 21 bits does not exist, like the
    voxels round the block in the middle.  Positions: a centre ((i - 2^20) + 0.5) * 0.5 is exact in float32 and c + f * v is rounded
    once, so a coordinate is within half an ulp of its exact value: at most 2^-5 at |x| <= 2^19, the block at the ends (below 1e-6
    in the middle)."""
    (_, mesh0, surf0), (records, mesh, surf) = block_restated(BLOCK_BASE), block_restated(corner)
    shift = np.asarray(corner) - np.asarray(BLOCK_BASE)
    v, f, n, k, d = mesh
    assert len(records[0]) == 195 and (len(v), len(f), len(surf[0])) == (len(mesh0[0]), len(mesh0[1]), len(surf0[0]))
    assert same((f, n, d), (mesh0[1], mesh0[2], mesh0[4])) and same((surf[1], surf[3]), (surf0[1], surf0[3]))
    assert np.array_equal(MR.coords(k), MR.coords(mesh0[3]) + shift) and np.array_equal(MR.coords(surf[0]), MR.coords(surf0[0]) + shift)
    x = MR.coords(records[0])
    assert x.min() == (0 if corner[0] < 0 else MR.AXIS - 5) and x.max() == (5 if corner[0] < 0 else MR.AXIS)
    bound = 2.0 ** -5 + 1e-6
    moved = [float(np.abs(a.astype(np.float64) - 0.5 * shift - b.astype(np.float64)).max()) for a, b in ((v, mesh0[0]), (surf[2], surf0[2]))]
    log(f"host block at {corner}: {len(v)} vertices, {len(f)} faces, {len(surf[0])} crossings: faces, directions, axes and normal bytes "
        f"of the block at {BLOCK_BASE}; keys moved by {shift.tolist()}, positions by 0.5 times that within {max(moved):.3e} (bound {bound:.3e})")
    assert max(moved) <= bound and v.tobytes() != mesh0[0].tobytes() and len(f) > 20 and len(surf[0]) > 20
