"""CPU: rolling the TSDF map (DESIGN §7l "Rolling the map"): the restatement (tests/tsdf_roll_restated.py), the inputs of the GPU
tests (tests/tsdf_roll_cases.py) and the host side of deeppointmap_amd/tsdf.py -- TsdfArchive, merged_export and the refusals.

  mutants     the cases tell each of the restatement's three mutants from the true form, and hold what their docstrings say: a
              tile at squared distance r2 exactly, tiles on both sides of the bias, b = 3 and b = 10, an origin 1 km out.
  numpy form  tsdf.tile_of / tile_near / merge_records equal the restatement on every case.
  archive     add / take / records against a dictionary written out by hand; equal keys add; tiles_near equals brute force over
              all tiles; save / load gives equal bytes and a map of another voxel_size, origin or distance is refused.
  merged      merged_export of an export split in two equals the export.
  refusals    roll refuses keep_radius < load_radius and a pose on the device; the C entry points refuse bad arguments before
              any HIP call.
Everything observed goes to test_logs/tsdf_roll.log.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_roll_cases as C  # noqa: E402
import tsdf_roll_restated as R  # noqa: E402

from conftest import ROOT  # noqa: E402


def log(line):
    print(line)
    try:
        os.makedirs(os.path.join(ROOT, "test_logs"), exist_ok=True)
        with open(os.path.join(ROOT, "test_logs", "tsdf_roll.log"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def partition(c, mutant=None):
    return R.evict(c.records, c.b, c.voxel, c.origin, c.pose, c.radius, mutant)


# -------------------------------------------------------------------------------------------------------------------- mutants
def test_the_cases_tell_every_mutant_from_the_true_form():
    cases = C.cases()
    told = {m: [] for m in R.MUTANTS}
    for name, c in cases.items():
        kept, out = partition(c)
        assert len(kept[0]) and len(out[0]), (name, len(kept[0]), len(out[0]))      # both sides of the partition are tested
        for m in R.MUTANTS:
            if not R.same(partition(c, m)[1], out):
                told[m].append(name)
        log(f"host roll case '{name}': b {c.b}, voxel {c.voxel}, {len(kept[0])} voxels kept, {len(out[0])} evicted; differs under "
            f"{[m for m in R.MUTANTS if name in told[m]]}")
    assert "exact" in told["strict"] and "exact" in told["voxel_centre"], told
    assert "straddle_b3" in told["unbiased"] and "straddle_b10" in told["unbiased"], told
    assert all(told.values()), told
    for shape in C.SHAPES:
        c = C.shaped(*shape)
        kept, out = partition(c)
        assert (len(kept[0]) + len(out[0]), len(out[0])) == shape[1:], shape


def test_the_exact_case_has_tiles_at_r2_exactly_and_they_are_near():
    c = C.exact()
    keys = c.records[0]
    ctr = np.stack(R.centres(keys, c.b, c.voxel), 1).astype(np.float64)
    d2 = ((ctr - (c.pose[:3, 3] - c.origin)) ** 2).sum(1)                         # exact in float64: small dyadic numbers
    on = d2 == c.radius ** 2
    tiles_on = np.unique(R.tile_keys(keys[on], c.b))
    assert len(tiles_on) == 4 and on.sum() == 4 * 512
    near = R.near(keys, c.b, c.voxel, c.origin, c.pose, c.radius)
    assert near[on].all() and not R.near(keys, c.b, c.voxel, c.origin, c.pose, c.radius, "strict")[on].any()
    assert (near == (d2 <= c.radius ** 2)).all()
    log(f"host roll exact: {len(tiles_on)} tiles at squared distance {c.radius ** 2} exactly: near by <=, far by <")


def test_the_cases_straddle_the_bias_use_both_tile_sizes_and_a_far_origin():
    cases = C.cases()
    assert {c.b for c in cases.values()} >= {3, 5, 10}
    for name in ("straddle_b3", "straddle_b10", "big_tiles"):
        idx = np.stack(R.axes(cases[name].records[0]), 1)
        assert (idx < R.BIAS).any(0).all() and (idx >= R.BIAS).any(0).all(), name
        assert (idx == R.BIAS - 1).any() and (idx == R.BIAS).any() if name != "big_tiles" else True
    assert np.abs(cases["far_origin"].origin).min() >= 1000.0


# ----------------------------------------------------------------------------------------------------------------- numpy form
def test_the_numpy_form_of_tsdf_py_is_the_restatement():
    from deeppointmap_amd import tsdf
    for name, c in C.cases().items():
        keys = c.records[0]
        tiles = tsdf.tile_of(keys, c.b)
        assert tiles.dtype == np.int64 and (tiles == R.tile_keys(keys, c.b)).all(), name
        got = tsdf.tile_near(tiles, c.b, c.pose[:3, 3] - c.origin, c.radius, c.voxel)
        assert (got == R.near(keys, c.b, c.voxel, c.origin, c.pose, c.radius)).all(), name
    rng = np.random.default_rng(3)
    keys = rng.integers(0, 50, 400)
    sums, counts = C.values(400, rng)
    want, outside = R.absorb((np.zeros(0, np.int64),) * 3, (keys, sums, counts))          # no count is 0: nothing is skipped
    assert outside == 0 and R.same(tsdf.merge_records(keys, sums, counts), want)


# -------------------------------------------------------------------------------------------------------------------- archive
def key(x, y, z):
    return int(R.pack(x + R.BIAS, y + R.BIAS, z + R.BIAS))


def test_archive_add_take_records_against_a_dictionary_written_out_by_hand():
    from deeppointmap_amd.tsdf import TsdfArchive
    a = TsdfArchive(tile_bits=3)
    assert len(a) == 0 and [x.shape for x in a.records()] == [(0,)] * 3 and [x.shape for x in a.take([1, 2])] == [(0,)] * 3
    # tiles of 8 voxels: (0,0,0) and (7,7,7) share tile A; (8,0,0) is tile B; (-1,0,0) is tile C
    k = [key(8, 0, 0), key(0, 0, 0), key(-1, 0, 0), key(7, 7, 7)]
    a.add(np.array(k), np.array([10, -20, 30, 40]), np.array([1, 2, 3, 0xFFFFFFFF], np.uint32))
    A, B, Cc = (int(R.tile_keys(np.array([q]), 3)[0]) for q in (k[1], k[0], k[2]))
    assert len({A, B, Cc}) == 3 and int(R.tile_keys(np.array([k[3]]), 3)[0]) == A
    hand = {A: ([k[1], k[3]], [-20, 40], [2, 0xFFFFFFFF]), B: ([k[0]], [10], [1]), Cc: ([k[2]], [30], [3])}
    assert sorted(a.tiles) == sorted(hand) and len(a) == 4
    for t, (hk, hs, hc) in hand.items():
        assert R.same(a.tiles[t], (np.array(hk, np.int64), np.array(hs, np.int64), np.array(hc, np.uint32))), t
    # equal keys add: inside one call and onto held ones; the count wraps as a uint32 does
    a.add(np.array([k[3], k[3], k[0]]), np.array([1, 2, -10]), np.array([1, 1, 5], np.uint32))
    assert R.same(a.tiles[A], (np.array([k[1], k[3]], np.int64), np.array([-20, 43], np.int64), np.array([2, 1], np.uint32)))
    assert R.same(a.tiles[B], (np.array([k[0]], np.int64), np.array([0], np.int64), np.array([6], np.uint32)))
    everything = a.records()
    assert list(everything[0]) == sorted(k) and len(a) == 4                      # records() takes nothing out
    got = a.take([B, A, 12345])                                                  # a tile it does not hold gives nothing
    assert R.same(got, R.sort_records([k[1], k[3], k[0]], [-20, 43, 0], np.array([2, 1, 6], np.uint32)))
    assert sorted(a.tiles) == [Cc] and len(a) == 1
    with pytest.raises(ValueError):
        a.add(np.array([-1]), np.array([0]), np.array([1], np.uint32))           # bit 63: no voxel
    with pytest.raises(ValueError):
        a.add(np.array([1, 2]), np.array([0]), np.array([1], np.uint32))
    for bad in (2, 11):
        with pytest.raises(ValueError):
            TsdfArchive(tile_bits=bad)


def test_archive_tiles_near_equals_brute_force_over_all_tiles():
    from deeppointmap_amd.tsdf import TsdfArchive
    for name, c in C.cases().items():
        a = TsdfArchive(c.b).add(*c.records)
        centre = c.pose[:3, 3] - c.origin
        got = a.tiles_near(centre, c.radius, c.voxel)
        keys = R.sort_records(*c.records)[0]
        near = R.near(keys, c.b, c.voxel, c.origin, c.pose, c.radius)
        want = np.unique(R.tile_keys(keys[near], c.b))
        assert got.dtype == np.int64 and (got == want).all(), name
        assert len(np.unique(R.tile_keys(keys[~near], c.b))) + len(want) == len(a.tiles), name   # a tile is on one side only
        kept, out = R.evict(c.records, c.b, c.voxel, c.origin, c.pose, c.radius)
        assert R.same(a.take(got), kept) and R.same(a.records(), out), name
        log(f"host roll archive '{name}': {len(want)} of {len(want) + len(a.tiles)} tiles near, as brute force says")


def bound(voxel=0.25, origin=(0.0, 0.0, 0.0), distance="ray", **kw):
    from deeppointmap_amd.tsdf import TsdfMap
    return TsdfMap(voxel_size=voxel, origin=np.array(origin), distance=distance, max_voxels=64, **kw)


def test_archive_save_load_round_trip_and_the_mismatch_checks(tmp_path):
    from deeppointmap_amd.tsdf import TsdfArchive
    c = C.cases()["far_origin"]
    a = TsdfArchive(c.b).add(*c.records)
    with pytest.raises(ValueError):
        a.save(tmp_path / "early.npz")                                           # no map has given it its geometry yet
    a.bind(bound(c.voxel, c.origin, truncation=1.0, step=0.125))
    path = tmp_path / "archive.npz"
    a.save(path)
    b = TsdfArchive.load(path)
    assert R.same(b.records(), a.records()) and sorted(b.tiles) == sorted(a.tiles) and len(b) == len(a)
    assert (b.tile_bits, b.voxel_size, b.distance, b.truncation, b.step) == (c.b, c.voxel, "ray", 1.0, 0.125)
    assert b.origin.tobytes() == np.asarray(c.origin, np.float64).tobytes()
    b.bind(bound(c.voxel, c.origin, truncation=2.0))                             # truncation and step are carried, not checked
    for other in (bound(0.5, c.origin), bound(c.voxel, c.origin + [0, 0, 1e-9]), bound(c.voxel, c.origin, "plane")):
        with pytest.raises(ValueError, match="archive"):
            other.absorb(b)                                                      # refused before anything touches a device
        assert other.table is None
        with pytest.raises(ValueError, match="archive"):
            other.roll(np.eye(4), b)
    assert len(b) == len(a)                                                      # a refusal takes nothing out
    with pytest.raises(ValueError):
        bound().absorb(TsdfArchive())                                            # an archive no map ever used


# --------------------------------------------------------------------------------------------------------------------- merged
def test_merged_export_of_a_split_export_is_the_export():
    from deeppointmap_amd.tsdf import TsdfArchive, merged_export
    c = C.general()
    whole = R.sort_records(*c.records)
    rng = np.random.default_rng(5)
    # every voxel's content is split by addition between the two sides; some voxels are on one side only
    part = rng.integers(-(1 << 39), 1 << 39, len(whole[0]))
    cpart = (whole[2].astype(np.int64) * rng.uniform(0, 1, len(whole[0]))).astype(np.uint32)
    side = rng.integers(0, 3, len(whole[0]))
    dev = (whole[0][side != 1], np.where(side == 0, whole[1] - part, whole[1])[side != 1],
           np.where(side == 0, whole[2] - cpart, whole[2])[side != 1])
    host = (whole[0][side != 2], np.where(side == 0, part, whole[1])[side != 2], np.where(side == 0, cpart, whole[2])[side != 2])
    got = merged_export(SimpleNamespace(export=lambda: dev), TsdfArchive(c.b).add(*host))
    assert R.same(got, whole)
    assert R.same(merged_export(SimpleNamespace(export=lambda: whole), TsdfArchive(c.b)), whole)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_roll_and_evict_refuse_bad_arguments_before_any_hip_call():
    import torch
    from deeppointmap_amd.tsdf import TsdfArchive, TsdfTracker
    m = bound(0.2, max_range=8.0)
    a = TsdfArchive()
    with pytest.raises(ValueError, match="keep_radius"):
        m.roll(np.eye(4), a, keep_radius=10.0, load_radius=10.5)
    with pytest.raises(ValueError, match="host"):
        m.roll(torch.eye(4, dtype=torch.float64), a)
    with pytest.raises(ValueError):
        m.roll(np.eye(3), a)
    side = 32 * 0.2
    assert m.reach(5) == pytest.approx(8.0 + (0.6 + 0.2) + 0.5 * np.sqrt(3.0) * side + 0.2)
    for kw in (dict(radius=-1.0), dict(radius=1.0, tile_bits=2), dict(radius=1.0, tile_bits=11), dict(radius=1.0, max_out=-1)):
        with pytest.raises(ValueError):
            m.evict(np.eye(4), **kw)
    assert [x.shape for x in m.evict(np.eye(4), 1.0)] == [(0,)] * 3 and m.table is None      # no table: nothing to evict
    with pytest.raises(ValueError):
        m.absorb(np.zeros(2, np.int64), np.zeros(2, np.int64))
    with pytest.raises(ValueError):
        TsdfTracker(slack=0.0, archive=True)
    assert isinstance(TsdfTracker(archive=True, tile_bits=4).archive, TsdfArchive) and TsdfTracker().archive is None


def test_the_entry_points_refuse_bad_arguments_before_any_hip_call():
    import ctypes
    from deeppointmap_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 255) & ~255          # never dereferenced: every call below is refused first, or is a no-op
    q = p + 4096
    o = (ctypes.c_double * 3)(0, 0, 0)
    bad_o = (ctypes.c_double * 3)(0, float("nan"), 0)
    names = ("src", "dst", "cap_vox", "voxel", "origin", "pose", "radius", "b", "keys", "sums", "counts", "count", "max_out", "stream")
    good = dict(src=p, dst=q, cap_vox=64, voxel=0.2, origin=ctypes.addressof(o), pose=p, radius=5.0, b=5, keys=p, sums=p, counts=p,
                count=p, max_out=4, stream=None)
    for k in (dict(src=None), dict(dst=None), dict(dst=p), dict(src=p + 8), dict(dst=q + 8), dict(cap_vox=65), dict(cap_vox=1),
              dict(cap_vox=1 << 25), dict(voxel=0.0), dict(voxel=float("nan")), dict(origin=None), dict(origin=ctypes.addressof(bad_o)),
              dict(pose=None), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=1e18), dict(b=2), dict(b=11), dict(count=None),
              dict(max_out=-1), dict(keys=None), dict(sums=None), dict(counts=None)):
        assert lib.dpm_tsdf_evict(*[{**good, **k}[n] for n in names]) == -1, k
    names = ("map", "cap_vox", "keys", "sums", "counts", "n", "stream")
    good = dict(map=p, cap_vox=64, keys=p, sums=p, counts=p, n=4, stream=None)
    for k in (dict(map=None), dict(map=p + 8), dict(cap_vox=65), dict(cap_vox=1 << 25), dict(n=-1), dict(keys=None), dict(sums=None),
              dict(counts=None)):
        assert lib.dpm_tsdf_absorb(*[{**good, **k}[n] for n in names]) == -1, k
    assert lib.dpm_tsdf_absorb(*[{**good, **dict(n=0, keys=None, sums=None, counts=None)}[n] for n in names]) == 0   # a no-op
