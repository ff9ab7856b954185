"""GPU: rolling the TSDF map (dpm_tsdf_evict, dpm_tsdf_absorb in csrc/tsdf_map.hip; TsdfMap.evict / absorb / roll, TsdfArchive,
merged_export and the rolling TsdfTracker in deeppointmap_amd/tsdf.py; DESIGN §7l "Rolling the map") against the numpy
restatement (tests/tsdf_roll_restated.py), byte for byte, on the inputs of tests/tsdf_roll_cases.py -- tests/test_tsdf_roll_host.py
shows on the CPU that these inputs tell the restatement's three mutants from the true form.

  evict       kept export and sorted list equal the restatement for the cases (a tile at r2 exactly, tiles on both sides of the
              bias, b = 3, 5, 10, an origin 1 km out) and for cap_vox 2, 64, 256, 512 x occupied 0 .. 512 x evicted 0, 1, 64, 65,
              all (full tables among them); the header words are carried over and src keeps its bytes; a list shorter than
              wanted keeps the rest in the map; a second run and one replay of a captured graph give the same sorted bytes.
  absorb      into an empty table, onto held keys, equal keys in one list, n in 0, 1, 255, 256, 257, permuted records, count 0 and
              bit 63 skipped, a table too small.
  round trip  evict at radius 0 then absorb of the list gives the export of the start, ray and plane forms.
  rolled      six frames on a 60 m line fused into a map rolled before every frame and into one never rolled: merged_export of
              the first is export of the second -- integrate alone, with carve under the default radii, and integrate alone under
              radii far below the reach; sample, register and raycast of the rolled map give the unrolled map's bytes.
  tracker     150 frames along a ribbed corridor: the rolling tracker in 2^16 slots gives the poses and steps of the plain tracker
              in 2^17, byte for byte, and ends with overflow() == 0, while the plain tracker in 2^16 slots overflows.
  syncs       evict is one host synchronisation, absorb none.
Everything observed goes to test_logs/tsdf_roll.log.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_cases as TC  # noqa: E402
import tsdf_roll_cases as C  # noqa: E402
import tsdf_roll_restated as R  # noqa: E402
from test_tsdf_roll_host import log  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("keys", "sums", "counts")


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def same(got, want, what):
    for x, y, name in zip(got, want, NAMES):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name, x.dtype, y.dtype, x.shape, y.shape)
        assert x.tobytes() == y.tobytes(), (what, name)


def loaded(c, cap_vox=None):
    """the case's records in a map of its own, put there by absorb (test_absorb_* check that against the restatement)"""
    from deeppointmap_amd.tsdf import TsdfMap
    m = TsdfMap(c.voxel, max_voxels=c.cap_vox if cap_vox is None else cap_vox, origin=c.origin, device=DEV)
    return m.absorb(*c.records)


def header(m, words=3):
    return (m.table[:4 * words].view(torch.int32).cpu().numpy().astype(np.int64) & 0xFFFFFFFF).tolist()


def evicted_as_restated(c, what):
    m = loaded(c)
    before = R.sort_records(*c.records)
    same(m.export(), before, what + ": loaded")
    m.table[:12].view(torch.int32).copy_(torch.tensor([5, 7, 9], dtype=torch.int32))       # the three counters, to be carried over
    src, src_bytes = m.table, m.table.clone()
    out = m.evict(c.pose, c.radius, c.b, max_out=c.cap_vox)
    want_kept, want_out = R.evict(c.records, c.b, c.voxel, c.origin, c.pose, c.radius)
    same(out, want_out, what + ": the list")
    same(m.export(), want_kept, what + ": kept")
    assert m.wanted == len(want_out[0])
    assert m.table.data_ptr() != src.data_ptr() and m._spare.data_ptr() == src.data_ptr()    # the tables changed places
    assert torch.equal(src, src_bytes), what + ": src keeps its bytes"
    assert header(m, 64) == [5, 7, 9] + [0] * 61, what
    return len(want_kept[0]), len(want_out[0])


# ---------------------------------------------------------------------------------------------------------------------- evict
@pytest.mark.parametrize("name", sorted(C.cases()))
def test_evict_is_the_restatement_byte_for_byte(name):
    c = C.cases()[name]
    kept, out = evicted_as_restated(c, name)
    assert kept and out
    log(f"gpu evict '{name}': b {c.b}, {kept} voxels kept, {out} listed: identical bytes; header carried, src untouched")


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "cap%d_occ%d_out%d" % s)
def test_evict_at_the_wave_and_block_edges_and_in_full_tables(shape):
    c = C.shaped(*shape)
    kept, out = evicted_as_restated(c, str(shape))
    assert (kept + out, out) == shape[1:]
    log(f"gpu evict shape cap_vox {shape[0]}, occupied {shape[1]}, evicted {shape[2]}: identical bytes")


@pytest.mark.parametrize("short", [0, 1, -1])
def test_a_list_shorter_than_wanted_keeps_the_rest_in_the_map(short):
    from deeppointmap_amd.tsdf import merge_records
    c = C.shaped(512, 257, 65)
    max_out = short if short >= 0 else c.evicted - 1
    m = loaded(c)
    out = m.evict(c.pose, c.radius, c.b, max_out=max_out)
    kept = m.export()
    assert m.wanted == c.evicted and len(out[0]) == min(c.evicted, max_out)
    assert not R.near(out[0], c.b, c.voxel, c.origin, c.pose, c.radius).any()                # only far voxels leave
    assert len(np.intersect1d(out[0], kept[0])) == 0 and len(kept[0]) + len(out[0]) == c.occupied
    same(merge_records(*[np.concatenate(p) for p in zip(kept, out)]), R.sort_records(*c.records), "kept + list")
    log(f"gpu evict max_out {max_out} of {c.evicted} wanted: {len(out[0])} listed, {len(kept[0])} kept, nothing dropped")


def test_the_staging_list_is_the_default_and_what_found_no_room_leaves_later():
    c = C.shaped(256, 256, 256)                                  # the staging list holds 256 // 4 records
    m = loaded(c)
    got, wanted = [], []
    for _ in range(4):
        got.append(m.evict(c.pose, c.radius, c.b))
        wanted.append(m.wanted)
    assert wanted == [256, 192, 128, 64] and [len(g[0]) for g in got] == [64] * 4
    assert len(m.export()[0]) == 0
    same(R.sort_records(*[np.concatenate(p) for p in zip(*got)]), R.sort_records(*c.records), "four lists")
    assert m._stage[0].numel() == 64


def test_evict_twice_and_from_a_captured_graph():
    from deeppointmap_amd import ops
    c = C.cases()["general_b5"]
    want_kept, want_out = R.evict(c.records, c.b, c.voxel, c.origin, c.pose, c.radius)
    m = loaded(c)
    n = c.cap_vox
    dst = ops.tsdf_new(n, DEV)
    lists = [torch.empty(n, dtype=t, device=DEV) for t in (torch.int64, torch.int64, torch.int32)]
    count = torch.empty(1, dtype=torch.int32, device=DEV)
    pose = dev(c.pose)

    def work():
        ops.tsdf_evict(m.table, dst, n, c.voxel, c.origin, pose, c.radius, c.b, *lists, count)

    def check(what):
        torch.cuda.synchronize()
        k = int(count.item())
        assert k == len(want_out[0]), what
        same(R.sort_records(lists[0][:k].cpu().numpy(), lists[1][:k].cpu().numpy(), lists[2][:k].cpu().numpy().view(np.uint32)),
             want_out, what)
        keys, sums, counts = ops.tsdf_export(dst, n)[1:]
        same(R.sort_records(keys.cpu().numpy(), sums.cpu().numpy(), counts.cpu().numpy().view(np.uint32)), want_kept, what)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work()
    torch.cuda.current_stream().wait_stream(side)
    check("first run")
    work()
    check("second run")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        work()
    dst.zero_(), count.fill_(-3)
    for t in lists:
        t.zero_()
    graph.replay()
    check("replayed from a captured graph")
    log(f"gpu evict: {len(want_kept[0])} kept, {len(want_out[0])} listed: identical sorted bytes twice and from a captured graph")


# --------------------------------------------------------------------------------------------------------------------- absorb
EMPTY3 = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.uint32))


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_absorb_into_an_empty_table_exports_the_records(n):
    c = C.shaped(512, n, 0)
    m = loaded(c)
    same(m.export(), R.sort_records(*c.records), f"n {n}")
    assert header(m) == [0, 0, 0] and m.check() is m


def test_absorb_adds_onto_held_keys_and_equal_keys_in_any_order_and_skips_what_is_no_record():
    from deeppointmap_amd.tsdf import TsdfMap
    c = C.general()
    held = tuple(a[:600] for a in c.records)
    rng = np.random.default_rng(8)
    fresh = c.records[0][600:700]
    keys = np.concatenate([held[0][:200], fresh, fresh[:40], fresh[:40], held[0][:5]])       # held keys, new ones, repeats of both
    sums, counts = C.values(len(keys), rng)
    counts[[3, 210, 301]] = 0                                                                 # skipped, sum and all
    bad = np.array([-1, -(1 << 63), int(fresh[0]) - (1 << 63)], np.int64)                     # bit 63 set: ~0, 2^63, a voxel's key with it
    keys = np.concatenate([keys, bad])
    sums, counts = np.concatenate([sums, [7, 7, 7]]), np.concatenate([counts, np.array([1, 1, 1], np.uint32)])
    want, outside = R.absorb(R.sort_records(*held), (keys, sums, counts))
    assert outside == 3
    ref = None
    for trial in range(3):
        p = rng.permutation(len(keys)) if trial else np.arange(len(keys))
        m = TsdfMap(c.voxel, max_voxels=c.cap_vox, origin=c.origin, device=DEV).absorb(*held)
        if trial == 2:
            m.absorb(dev(keys[p]), dev(sums[p]), dev(counts[p].view(np.int32)))                # tensors on the device
        else:
            m.absorb(keys[p].astype(np.uint64), sums[p], counts[p])                            # numpy, keys as the ABI's uint64
        same(m.export(), want, f"trial {trial}")
        assert header(m) == [0, 3, 0] and m.outside() == 3
        ref = ref or [a.tobytes() for a in m.export()]
        assert [a.tobytes() for a in m.export()] == ref
    log(f"gpu absorb: {len(keys)} records onto {len(held[0])} held voxels -> {len(want[0])}: the restatement's bytes in three orders; "
        f"3 records of count 0 skipped, 3 keys with bit 63 counted in header word 1")


def test_absorb_into_a_table_too_small_counts_the_records_and_check_raises():
    c = C.shaped(512, 100, 0)
    m = loaded(c, cap_vox=64)
    n = m.overflow()
    log(f"gpu absorb overflow: 100 records offered to 64 slots: {n} found none")
    assert n == 36 and len(m.export()[0]) == 64
    with pytest.raises(ValueError, match="full"):
        m.check()


# ----------------------------------------------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("distance", ["ray", "plane"])
def test_evict_at_radius_0_then_absorb_gives_the_export_of_the_start(distance):
    from deeppointmap_amd.tsdf import TsdfMap
    c = TC.two_frames()
    m = TsdfMap(c.voxel, c.truncation, c.step, c.cap_vox, c.min_range, c.max_range, origin=c.origin, device=DEV, distance=distance)
    rng = np.random.default_rng(4)
    for xyz, count, pose in c.frames:
        nrm = rng.normal(size=xyz.shape)
        nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
        m.integrate(dev(xyz), pose, length=count, normals=dev(nrm) if distance == "plane" else None)
    start = m.check().export()
    head = header(m)
    out = m.evict(c.frames[0][2], 0.0, 5, max_out=c.cap_vox)
    same(out, start, "everything leaves at radius 0")
    assert len(m.export()[0]) == 0 and len(start[0]) > 1000
    m.absorb(*out)
    same(m.export(), start, "and comes back")
    assert header(m) == head
    log(f"gpu round trip, {distance} form: {len(start[0])} voxels out at radius 0 and back: identical bytes")


# -------------------------------------------------------------------------------------------------------- rolled equals unrolled
def line_maps(mode, upto=None):
    """the six frames of the line in a map rolled before every frame and in one never rolled -> (rolled, archive, plain, absorbed)"""
    from deeppointmap_amd.tsdf import TsdfArchive, TsdfMap
    K = C.LINE
    make = lambda: TsdfMap(K["voxel"], max_voxels=1 << 15, max_range=K["max_range"], origin=np.zeros(3), device=DEV)
    rolled, plain, archive = make(), make(), TsdfArchive(K["b"])
    radii = dict(keep_radius=3.0, load_radius=2.0) if mode == "small" else {}
    absorbed = 0
    for xyz, P in C.line_frames()[:upto]:
        x = dev(xyz)
        held = len(archive)
        rolled.roll(P, archive, slack=K["slack"], **radii)
        absorbed += held + rolled.wanted - len(archive)
        for m in (rolled, plain):
            m.integrate(x, P)
            if mode == "carve":
                m.carve(x, P)
    return rolled, archive, plain, absorbed


@pytest.mark.parametrize("mode", ["integrate", "carve", "small"])
def test_merged_export_of_the_rolled_map_is_the_export_of_the_unrolled_one(mode):
    from deeppointmap_amd.tsdf import merged_export
    rolled, archive, plain, absorbed = line_maps(mode)
    want = plain.check().export()
    rolled.check()
    same(merged_export(rolled, archive), want, mode)
    resident = len(rolled.export()[0])
    log(f"gpu rolled == unrolled, {mode}: {len(want[0])} voxels; the rolled map holds {resident}, the archive {len(archive)} in "
        f"{len(archive.tiles)} tiles; {absorbed} voxels came back from the archive on the way")
    assert 0 < resident < len(want[0]) and len(archive) > 0
    if mode == "small":
        assert resident + len(archive) > len(want[0])            # voxels split between the device and the host: they add
    else:
        assert absorbed > 0                                       # tiles came back whole before a frame touched them


def test_reads_of_the_rolled_map_are_those_of_the_unrolled_one():
    from deeppointmap_amd.tsdf import HIT
    rolled, archive, plain, _ = line_maps("integrate")
    frames = C.line_frames()
    rng = np.random.default_rng(6)
    seen = dict(valued=0, hit=0, rows=0)
    for k in (5, 4, 1, 3):                                       # 12, 36, 24, 60 m: back along the line and out again
        xyz, P = frames[k]
        rolled.roll(P, archive, slack=C.LINE["slack"])
        q = dev((xyz + rng.normal(0, 0.05, xyz.shape)).astype(np.float32))
        a, b = rolled.sample(q, P), plain.sample(q, P)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), ("sample", k)
        seen["valued"] += int((a[2] == 1).sum())
        init = P.copy()
        init[:3, 3] += (0.03, -0.02, 0.04)
        (ra, ea), (rb, eb) = rolled.register(dev(xyz), init, debug=True), plain.register(dev(xyz), init, debug=True)
        assert all(torch.equal(x, y) for x, y in zip(tuple(ra) + tuple(ea), tuple(rb) + tuple(eb))), ("register", k)
        seen["rows"] += int((ea[0] == 1).sum())
        dirs = dev(xyz / np.linalg.norm(xyz, axis=1, keepdims=True), np.float32)
        ca, cb = rolled.raycast(P, dirs), plain.raycast(P, dirs)
        assert all(torch.equal(x, y) for x, y in zip(ca, cb)), ("raycast", k)
        seen["hit"] += int((ca.flag == HIT).sum())
    resident, whole = len(rolled.export()[0]), len(plain.export()[0])
    log(f"gpu reads of the rolled map at 4 poses: sample ({seen['valued']} valued points), register ({seen['rows']} rows given) and "
        f"raycast ({seen['hit']} hits): the unrolled map's bytes; {resident} of {whole} voxels resident")
    assert seen["valued"] > 100 and seen["rows"] > 100 and seen["hit"] > 50     # the CPU restatement counts about 400, 340
    assert resident < whole


# -------------------------------------------------------------------------------------------------------------------- tracker
def test_the_rolling_tracker_is_the_plain_one_and_fits_where_that_one_overflows():
    """Sizes, chosen on the CPU (tests/tsdf_roll_cases.touched and the restatement's tracker over the same frames): the 150
    gated frames touch 83 thousand voxels under the true poses and 95 thousand under the registered ones, 0.63 thousand a
    frame; with tile_bits 3, slack 1 m and max_range 4 m the reach is 6.98 m, rolls come every second frame (74 of them) and at
    most 16 thousand voxels are resident.  So 2^17 slots hold the plain run (72 % full), 2^16 do not (full near frame 100), and
    the rolling run needs a quarter of 2^16."""
    from deeppointmap_amd.tsdf import TsdfTracker, merged_export
    K = C.CORRIDOR
    xyz, nrm, true = C.gated_corridor()
    frames = [(dev(a), dev(b)) for a, b in zip(xyz, nrm)]
    kw = dict(voxel_size=K["voxel"], max_range=K["max_range"], device=DEV, distance="plane", register_every=K["register_every"])
    plain = TsdfTracker(max_voxels=1 << 17, **kw)
    rolling = TsdfTracker(max_voxels=1 << 16, archive=True, slack=K["slack"], tile_bits=K["b"], **kw)
    peak = 0
    for k, (a, b) in enumerate(frames):
        plain.step(a, b, pose=true[0] if k == 0 else None)
        rolling.step(a, b, pose=true[0] if k == 0 else None)
        if k % 10 == 0:
            peak = max(peak, len(rolling.map.export()[0]))
    assert plain.map.overflow() == 0 and plain.lost == 0
    assert rolling.rolls >= 2 and rolling.lost == 0
    assert np.stack(rolling.poses).tobytes() == np.stack(plain.poses).tobytes()
    assert rolling.steps == plain.steps
    assert rolling.map.overflow() == 0
    whole = plain.map.export()
    same(merged_export(rolling.map, rolling.archive), whole, "the rolling tracker's map and archive")
    assert len(whole[0]) > 1 << 16 > 2 * peak
    small = TsdfTracker(max_voxels=1 << 16, **kw)
    full_at = None
    for k, (a, b) in enumerate(frames):
        small.step(a, b, pose=true[0] if k == 0 else None)
        if small.map.overflow():
            full_at = k
            break
    assert full_at is not None
    with pytest.raises(ValueError, match="full"):
        small.map.check()
    log(f"gpu tracker, corridor of {len(frames)} frames: the rolling tracker (2^16 slots, {rolling.rolls} rolls, peak {peak} resident, "
        f"{len(rolling.archive)} archived at the end) gives the poses and steps of the plain one (2^17 slots, {len(whole[0])} voxels) "
        f"byte for byte; the plain one in 2^16 slots overflows at frame {full_at}")


# ---------------------------------------------------------------------------------------------------------------------- syncs
def test_evict_is_one_host_synchronisation_and_absorb_none():
    from deeppointmap_amd import augment
    c = C.cases()["general_b5"]
    m = loaded(c)
    pose = dev(c.pose)
    m.evict(pose, c.radius, c.b)                                  # the second table and the staging list exist from here on
    torch.cuda.synchronize()
    n = augment.host_syncs()
    out = m.evict(pose, 0.5 * c.radius, c.b)
    assert augment.host_syncs() - n == 1
    n = augment.host_syncs()
    m.absorb(*out)
    m.absorb(dev(out[0]), dev(out[1]), dev(out[2].view(np.int32)))
    assert augment.host_syncs() - n == 0
