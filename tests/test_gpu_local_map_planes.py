"""GPU: the voxel planes of the local map (csrc/local_map.hip: dpm_local_map_planes) against the numpy restatement
(tests/lidar_plane_restated.py) computed from the GPU map's own export.

  counts           equal to the float32 restatement on every held voxel: lattice points on voxel faces and on the ball's surface
                   at equality, negative coordinates, s = 1, 2, 3.
  normals          within 1e-6 rad of the float64 restatement (numpy.linalg.eigh about the mean) and w within 1e-5 absolute on the
                   voxels whose gap (l1 - l0) / l2 is >= 1e-3: fp64 cumulants leave the angle error near 1e-13 / gap, the fp32
                   rounding of the normal about 6e-8.  Voxels below the gap are left out of the angle check only and are at
                   most 2 % of those with >= 5 points (tests/test_lidar_plane_host.py shows it on the restatement alone).
  exact cases      axis-plane lattices bit for bit: (0,0,1,0) and the like; a straight line rounded to fp32 has no plane.
  content only     permuted rows, the other stamp assignment, a prune against a fresh map of another size, colliding keys that
                   wrap a 64-slot table: the sorted export_planes() is the same bytes.
  empty, overflow  (0,0,0,-1) and count 0; an overflowed map raises at read-back.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restated as I  # noqa: E402
import lidar_odometry_restated as L  # noqa: E402
import lidar_plane_restated as PR  # noqa: E402
from test_gpu_local_map import colliding_voxels, frame, gpu_map, lattice, log  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EYE = np.eye(4)
NONE = np.array([0, 0, 0, -1], np.float32).tobytes()


def both(g, dtype, radius=None):
    """the GPU's sorted planes and the restatement's from the GPU map's own export, keys checked"""
    got = g.export_planes()
    want = PR.planes(g.export(), g.voxel_size, g.plane_radius if radius is None else radius, dtype)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == got[3].dtype == np.float32
    assert np.array_equal(got[0], want.keys)
    return got, want


def same_planes(a, b):
    for x, y, name in zip(a, b, ("keys", "counts", "normals", "w")):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), name


def close(got, want, what):
    """angle and w on the voxels with a gap; -> the number left out"""
    _, counts, normal, w = got
    big = want.counts >= 5
    low = big & (want.gap < 1e-3)
    check = big & ~low
    assert low.sum() <= 0.02 * big.sum(), (int(low.sum()), int(big.sum()))
    assert np.array_equal(w[check] >= 0, want.w[check] >= 0)
    ang, dw = PR.angle(normal[check], want.normal[check]), np.abs(w[check] - want.w[check])
    log(f"planes {what}: {len(counts)} voxels, {int(check.sum())} compared, {int(low.sum())} below the gap, "
        f"max angle to the float64 restatement {ang.max():.3e} rad, max |dw| {dw.max():.3e}")
    assert ang.max() <= 1e-6 and dw.max() <= 1e-5
    return int(low.sum())


@pytest.mark.parametrize("s,cap_vox", [(1, 512), (2, 1024), (3, 4096)])
def test_counts_are_the_float32_restatements(s, cap_vox):
    rng = np.random.default_rng(40 + s)
    g = gpu_map(s=s, cap_vox=cap_vox)
    g.insert(frame(lattice(rng, 700, 0.25, 3.0)), I.se3([0, 0, 0], [0.5, -0.25, 1.0]))
    got, want = both(g, np.float32)
    assert np.array_equal(got[1], want.counts) and got[1].max() >= 9 and got[1].min() >= 1
    # the lattice puts members exactly on the ball's surface (d = (1, 1, .5) and the like) and points on voxel faces
    _, vi, pi, d = PR.members(g.export(), 1.0, 1.5, np.float64)
    assert ((d * d).sum(axis=1) == 2.25).sum() > 20 and (g.export()[3] == np.floor(g.export()[3])).any()
    assert (L.unpack_key(got[0]) < 0).any()
    # a smaller ball, with its own equalities (d = (1, 0, 0))
    from deeppointmap_amd.odometry import LocalMap
    g2 = LocalMap(1.0, s, cap_vox, 1e4, origin=(0, 0, 0), device=DEV, plane_radius=1.0)
    g2.insert(frame(g.export()[3]), EYE)
    got2, want2 = both(g2, np.float32)
    assert np.array_equal(got2[1], want2.counts) and (got2[1] < got[1]).any()
    defined = want.w >= 0
    assert np.array_equal(got[3] >= 0, defined) and all(r.tobytes() == NONE for r in np.column_stack([got[2], got[3]])[~defined])


@pytest.mark.parametrize("s", [1, 3])
def test_normals_are_the_float64_restatements(s):
    g = gpu_map(s=s, cap_vox=4096)
    g.insert(frame(PR.normals_scene()), EYE)
    got, want = both(g, np.float64)
    assert np.array_equal(got[1], want.counts), "the scene has no point within rounding of a ball's surface"
    close(got, want, f"room scene s {s}")
    mirror = PR.planes(g.export(), 1.0, 1.5, np.float32)
    ok = mirror.w >= 0
    assert np.array_equal(got[3] >= 0, ok) and np.abs(got[3] - mirror.w).max() <= 1e-5
    assert (np.linalg.norm(got[2][ok].astype(np.float64), axis=1) - 1).max() < 2e-7


@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_axis_plane_lattices_bit_for_bit(axis, s):
    g = gpu_map(s=s, cap_vox=64)
    g.insert(frame(PR.plane_lattice(axis, 0.25, centre=(-0.5, 0.25, 1.0))), EYE)
    got, want = both(g, np.float32)
    same_planes(got, (want.keys, want.counts, want.normal, want.w))
    exact = np.zeros(4, np.float32)
    exact[axis] = 1
    rows = np.column_stack([got[2], got[3]])
    assert sum(r.tobytes() == exact.tobytes() for r in rows) >= 4
    assert all(r.tobytes() in (exact.tobytes(), NONE) for r in rows)


def test_a_line_rounded_to_float32_has_no_plane():
    g = gpu_map(cap_vox=64)
    g.insert(frame(PR.wall_line()), EYE)
    got, want = both(g, np.float32)
    assert np.array_equal(got[1], want.counts) and got[1].max() >= 5
    assert all(r.tobytes() == NONE for r in np.column_stack([got[2], got[3]])) and (want.w == -1).all()


def test_arrival_order_does_not_matter():
    rng = np.random.default_rng(7)
    pts = np.concatenate([lattice(rng, 300, 0.125, 3.0), rng.uniform(-3, 3, (500, 3)).astype(np.float32)])
    n = len(pts)
    idx = np.arange(n, dtype=np.int32)
    perm = rng.permutation(n)
    a = gpu_map(cap_vox=1024).insert(frame(pts, n + 3, idx), EYE)
    b = gpu_map(cap_vox=1024).insert(frame(pts[perm], n, idx[perm]), EYE)
    ref = a.export_planes()
    same_planes(ref, b.export_planes())
    assert (ref[3] >= 0).sum() > 100
    # one point per sub-cell, dealt to two frames: whichever frame comes first, the map keeps the same points
    kept = a.export()[3]
    first = rng.random(len(kept)) < 0.5
    c = gpu_map(cap_vox=1024).insert(frame(kept[first]), EYE).insert(frame(kept[~first]), EYE)
    d = gpu_map(cap_vox=1024).insert(frame(kept[~first]), EYE).insert(frame(kept[first]), EYE)
    assert c.export()[3].tobytes() == d.export()[3].tobytes() == kept.tobytes()
    assert c.export()[2].tobytes() != d.export()[2].tobytes(), "the owner words differ"
    same_planes(ref, c.export_planes()), same_planes(ref, d.export_planes())


def test_planes_after_a_prune_are_those_of_a_fresh_map():
    g = gpu_map(cap_vox=4096)
    g.insert(frame(PR.normals_scene(seed=4)), EYE)
    before = g.export_planes()
    g.prune(I.se3([0, 0, 0], [1.0, -0.5, 0.5]), 6.0)
    after = g.export_planes()
    assert 50 < len(after[0]) < len(before[0])
    at = np.searchsorted(before[0], after[0])
    assert (after[1] < before[1][at]).sum() > 10, "voxels at the border lost neighbours"
    fresh = gpu_map(cap_vox=1024)          # another table size: other slots
    fresh.insert(frame(g.export()[3]), EYE)
    same_planes(after, fresh.export_planes())
    close(after, PR.planes(g.export(), 1.0, 1.5, np.float64), "after a prune")
    # the cache follows the map: a second read without a change is the same tensors, an insert makes it stale
    p1, p2 = g.planes(), g.planes()
    assert p1[0] is p2[0] and not g._planes_stale
    g.insert(frame(np.array([[0.1, 0.2, 0.3]], np.float32)), EYE)
    assert g._planes_stale


def test_colliding_keys_that_wrap_a_64_slot_table():
    vox = colliding_voxels(48, 64, 60)
    offs = np.array([[0.25, 0.25, 0.25], [0.75, 0.25, 0.5], [0.25, 0.75, 0.75], [0.75, 0.75, 0.25]], np.float32)
    xyz = (vox[:, None, :] + offs[None, :, :]).reshape(-1, 3)
    g = gpu_map(s=2, cap_vox=64)
    g.insert(frame(xyz), EYE)
    assert g.overflow == 0
    got, want = both(g, np.float32)
    assert len(got[0]) == 48 and np.array_equal(got[1], want.counts) and got[1].min() >= 4
    ok = want.w >= 0
    assert np.array_equal(got[3] >= 0, ok) and PR.angle(got[2][ok & (want.gap >= 1e-3)], want.normal[ok & (want.gap >= 1e-3)]).max() <= 1e-6
    other = gpu_map(s=2, cap_vox=256)
    other.insert(frame(xyz), EYE)
    same_planes(got, other.export_planes())


def test_empty_slots_and_an_empty_map():
    g = gpu_map(cap_vox=128)
    assert [len(a) for a in g.export_planes()] == [0, 0, 0, 0]
    g.prune(EYE, 1.0)                                  # allocates the table: a map without a point
    planes, counts = g.planes()
    assert planes.shape == (128, 4) and counts.shape == (128,)
    assert (counts == 0).all() and all(r.tobytes() == NONE for r in planes.cpu().numpy())
    g.insert(frame(PR.plane_lattice(2, 0.5)), EYE)
    planes, counts = [t.cpu().numpy() for t in g.planes()]
    held = len(g.export_planes()[0])
    assert 0 < held < 128 and (counts > 0).sum() == held
    assert all(r.tobytes() == NONE for r in planes[counts == 0])


def test_an_overflowed_map_raises_at_read_back():
    xyz = np.stack([np.arange(65), np.zeros(65), np.zeros(65)], axis=1).astype(np.float32) + np.float32(0.5)
    g = gpu_map(s=2, cap_vox=64)
    g.insert(frame(xyz), EYE)
    with pytest.raises(ValueError, match="local map is full"):
        g.export_planes()


def test_same_bytes_twice_and_from_a_captured_graph():
    from deeppointmap_amd import ops
    g = gpu_map(cap_vox=1024)
    g.insert(frame(PR.normals_scene(seed=5, n=600)), EYE)
    first = [t.clone() for t in g.planes()]
    again = ops.local_map_planes(*g._args(), g.plane_radius)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, again))
    out = [torch.zeros_like(t) for t in first]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.local_map_planes(*g._args(), g.plane_radius, *out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t in out:
        t.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.local_map_planes(*g._args(), g.plane_radius, *out)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, out)), "replayed from a captured graph"
