"""GPU: the rolling local map and the registration against it (csrc/local_map.hip) kernel by kernel against the numpy
restatement (tests/lidar_odometry_restated.py).

  insert / prune   the exported map, sorted by (key, sub-cell), byte for byte against the float32 restatement: lattice points on
                   voxel and sub-cell faces and at negative coordinates, both rules of the owner word, both range gates at
                   equality, rows past the count (NaN) untouched, colliding hashes whose probe chain wraps the table's end,
                   permuted rows, the overflow path.
  search           every query's (key, sub-cell) equals the exhaustive search over the exported map, constructed ties included.
  sums             the 29 values on the kernel's own matches against the float64 restatement, per entry
                   max(3 |r32 - r64|, floor) -- the idiom and the floor of tests/test_gpu_icp.py, the floor extended by the
                   weight's own sensitivity (lidar_odometry_restated.system_floor).
  known answer     three lattice planes, a pose of 0.3 m and 2 degrees recovered within 1e-4 m / 1e-4 rad; the same 1 km from
                   the world's zero with the map's origin there, within 1 mm.
  repeatability    the same bytes twice, a schedule equals chained calls, one replay of a captured graph.
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restated as I  # noqa: E402
import lidar_odometry_restated as L  # noqa: E402
from test_lidar_odometry_host import known_pose_case, pose_error  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EYE = np.eye(4)


def log(line):
    print(line)
    try:
        os.makedirs(os.path.join(ROOT, "test_logs"), exist_ok=True)
        with open(os.path.join(ROOT, "test_logs", "lidar_odometry_errors.log"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def frame(xyz, cap=None, idx=None):
    """a frame whose first len(xyz) rows are valid; the rows past them hold NaN and an index that would win every sub-cell"""
    from deeppointmap_amd.augment import PointCloud
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    cap = n if cap is None else cap
    buf = np.full((cap, 3), np.nan, np.float32)
    buf[:n] = xyz
    rows = np.zeros(cap, np.int32)
    rows[:n] = np.arange(n) if idx is None else idx
    return PointCloud.from_buffers(torch.from_numpy(buf).to(DEV), torch.from_numpy(rows).to(DEV),
                                   torch.tensor([n], dtype=torch.int32, device=DEV), host_n=n)


def gpu_map(voxel=1.0, s=3, cap_vox=1 << 12, origin=(0, 0, 0), min_range=0.0, max_range=1e4):
    from deeppointmap_amd.odometry import LocalMap
    return LocalMap(voxel, s, cap_vox, max_range, min_range, origin=origin, device=DEV)


def same_export(g, r):
    """the GPU map's sorted export and the float32 restatement's: the same bytes"""
    a, b = g.export(), r.export()
    for x, y, name in zip(a, b, ("keys", "sub-cells", "owner words", "coordinates")):
        assert x.dtype == y.dtype and x.shape == y.shape, (name, x.dtype, y.dtype, x.shape, y.shape)
        assert x.tobytes() == y.tobytes(), name
    return a


def lattice(rng, n, step=0.25, half=3.0):
    """n points on a lattice of `step` in [-half, half]^3: voxel faces (integers), sub-cell faces, negative coordinates"""
    k = int(round(half / step))
    return (rng.integers(-k, k + 1, (n, 3)) * step).astype(np.float32)


# --------------------------------------------------------------------------------------------------------------------- insert
@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("cap", [1, 63, 64, 65, 257])
def test_insert_is_the_restatement_byte_for_byte(cap, s):
    rng = np.random.default_rng(100 * cap + s)
    pose = I.se3([0, 0, 0], [0.5, -0.25, 1.0])        # a lattice shift: the fp32 transform is exact
    g, r = gpu_map(s=s), L.Map(1.0, s, dtype=np.float32, max_range=1e4)
    t32 = pose[:3, 3].astype(np.float32)
    for stamp, n in enumerate([0, cap - cap // 3, cap, min(cap, 2)]):   # count 0, count < cap over NaN rows, a full frame ...
        xyz = lattice(rng, n)
        idx = rng.permutation(cap)[:n].astype(np.int32)   # within a frame the smaller ROW NUMBER wins, wherever it lies
        if stamp == 3:                                     # ... and a later frame that offers row 0 to cells that are taken
            xyz, idx = r.export()[3][:n] - t32, np.zeros(n, np.int32)
        g.insert(frame(xyz, cap, idx), pose)
        r.insert(xyz, idx, pose, stamp)
        same_export(g, r)
    assert g.overflow == 0 and g.n_points == len(r.export()[0])
    # the frame with the most points, again, its rows permuted and idx along: the same map; and a second run of it
    xyz, idx = lattice(rng, cap), np.arange(cap, dtype=np.int32)
    perm = rng.permutation(cap)
    maps = [gpu_map(s=s) for _ in range(3)]
    maps[0].insert(frame(xyz, cap + 3, idx), pose)
    maps[1].insert(frame(xyz[perm], cap, idx[perm]), pose)
    maps[2].insert(frame(xyz, cap + 3, idx), pose)
    ref = L.Map(1.0, s, dtype=np.float32, max_range=1e4)
    ref.insert(xyz, idx, pose, 0)
    for m in maps:
        same_export(m, ref)


def test_rule_within_and_across_frames_and_floor_at_negative_coordinates():
    g, r = gpu_map(s=2), L.Map(1.0, 2, dtype=np.float32, max_range=1e4)
    steps = [([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2]], [5, 2]),            # one sub-cell, one frame: row 2 keeps it
             ([[0.3, 0.3, 0.3]], [0]),                                  # a later frame with a lower row: the older frame wins
             ([[0.6, 0.1, 0.1], [-0.1, -0.1, -0.1], [-1.0, -0.5, 0.0], [0.5, 0.5, 0.5], [1.0, 1.0, 1.0]], [0, 1, 2, 3, 4])]
    for stamp, (xyz, idx) in enumerate(steps):
        g.insert(frame(xyz, 7, idx), EYE)
        r.insert(np.array(xyz, np.float32), idx, EYE, stamp)
    keys, sub, owner, xyz = same_export(g, r)
    first = np.nonzero((keys == L.pack_key([0, 0, 0])) & (sub == 0))[0]
    assert owner[first[0]] == 2 and np.allclose(xyz[first[0]], 0.2)
    assert (-1, -1, -1) in {tuple(v) for v in L.unpack_key(keys)} and (-1, -1, 0) in {tuple(v) for v in L.unpack_key(keys)}


def test_range_gates_at_equality():
    g = gpu_map(s=1, min_range=5.0, max_range=13.0)
    r = L.Map(1.0, 1, min_range=5.0, max_range=13.0, dtype=np.float32)
    xyz = np.array([[3, 4, 0], [2.5, 4, 0], [5, 12, 0], [5, 12.5, 0], [np.nan, 0, 0], [0, 0, 13], [0, -5, 0]], np.float32)
    pose = I.se3([0, 0, 0], [100.0, 0, 0])      # the gate is on the SENSOR-frame range
    g.insert(frame(xyz, 9), pose)
    r.insert(xyz, np.arange(len(xyz)), pose, 0)
    assert len(same_export(g, r)[0]) == 4


def colliding_voxels(n, cap_vox, first_slot):
    """n voxel coordinates whose keys all start probing at or after first_slot of a table of cap_vox slots"""
    out = []
    for x in range(-40, 40):
        for y in range(-40, 40):
            if L.mix64(int(L.pack_key([x, y, 0]))) & (cap_vox - 1) >= first_slot:
                out.append((x, y, 0))
                if len(out) == n:
                    return np.array(out, np.float32)
    raise AssertionError("not enough colliding keys")


def test_colliding_hashes_wrap_the_end_of_the_table():
    vox = colliding_voxels(48, 64, 60)            # 48 voxels start in the last 4 of 64 slots: the chain wraps to slot 0
    xyz = vox + np.float32(0.5)
    g, r = gpu_map(s=1, cap_vox=64), L.Map(1.0, 1, dtype=np.float32, max_range=1e4)
    g.insert(frame(xyz), EYE)
    r.insert(xyz, np.arange(48), EYE, 0)
    keys = same_export(g, r)[0]
    assert len(keys) == 48 and g.overflow == 0
    # every voxel is found again through its chain: each point is its own nearest neighbour at distance 0
    res, (key, sub, system) = g.register(frame(xyz), EYE, [(0.5, 1)], debug=True)
    assert np.array_equal(key.cpu().numpy(), L.pack_key(vox.astype(np.int64))) and system[27].item() == 48 and system[28].item() == 0


def test_overflow_is_counted_and_python_raises():
    xyz = np.stack([np.arange(65), np.zeros(65), np.zeros(65)], axis=1).astype(np.float32) + np.float32(0.5)
    g, r = gpu_map(s=2, cap_vox=64), L.Map(1.0, 2, dtype=np.float32, max_range=1e4)
    g.insert(frame(xyz), EYE)
    r.insert(xyz, np.arange(65), EYE, 0)
    assert g.overflow == 1                         # 65 voxels of one point each: exactly one point finds no slot
    keys, sub, owner, pts = g.export(check=False)
    rk, rs, ro, rp = r.export()
    assert len(keys) == 64 and len(set(keys.tolist())) == 64
    where = {int(k): i for i, k in enumerate(rk)}
    for i, k in enumerate(keys):                   # whichever 64 voxels made it: each holds what the rule gives its key
        j = where[int(k)]
        assert sub[i] == rs[j] and owner[i] == ro[j] and pts[i].tobytes() == rp[j].tobytes()
    for read in (g.points, g.check, lambda: g.n_points):
        with pytest.raises(ValueError, match="local map is full"):
            read()


# ---------------------------------------------------------------------------------------------------------------------- prune
@pytest.mark.parametrize("s", [1, 3])
def test_prune_at_the_radius_to_empty_and_insert_after(s):
    rng = np.random.default_rng(5)
    g, r = gpu_map(s=s, cap_vox=256), L.Map(1.0, s, dtype=np.float32, max_range=1e4)
    xyz = np.concatenate([np.array([[3.2, 4.2, 0.2], [3.2, 5.2, 0.2], [0.2, 0.2, 0.2], [-4.8, 0.2, 0.2]], np.float32), lattice(rng, 60, 0.25, 6.0)])
    g.insert(frame(xyz), EYE), r.insert(xyz, np.arange(len(xyz)), EYE, 0)
    P = I.se3([0, 0, 0.3], [0.5, 0.5, 0.5])        # centres (3.5, 4.5, .5) and (-4.5, .5, .5) lie exactly 5 away
    g.prune(P, 5.0), r.prune(P, 5.0)
    kept = {tuple(v) for v in L.unpack_key(same_export(g, r)[0])}
    assert (3, 4, 0) in kept and (-5, 0, 0) in kept and (3, 5, 0) not in kept
    more = lattice(rng, 40, 0.25, 6.0)              # insert after a prune: into the other half, older points still win
    g.insert(frame(more), EYE), r.insert(more, np.arange(40), EYE, 1)
    same_export(g, r)
    g.prune(P, 2.0), r.prune(P, 2.0)
    same_export(g, r)
    far = I.se3([0, 0, 0], [100.0, 0, 0])
    g.prune(far, 1.0), r.prune(far, 1.0)
    assert len(same_export(g, r)[0]) == 0 and g.n_points == 0
    g.insert(frame(more), EYE), r.insert(more, np.arange(40), EYE, 2)
    assert len(same_export(g, r)[0]) > 0 and g.overflow == 0


# ------------------------------------------------------------------------------------------------------------ search and sums
def matches_of(key, sub, exported):
    """the kernel's (key, sub-cell) per query -> rows of the sorted export, -1 for none"""
    where = {(int(k), int(c)): i for i, (k, c) in enumerate(zip(exported[0], exported[1]))}
    return np.array([where[(int(k), int(c))] if k >= 0 else -1 for k, c in zip(key.cpu().numpy(), sub.cpu().numpy())], np.int64)


@pytest.mark.parametrize("voxel,s,max_dist", [(1.0, 2, 1.0), (1.0, 3, 0.75), (0.5, 3, 0.5), (2.0, 1, 1.0)])
def test_every_match_is_the_exhaustive_search(voxel, s, max_dist):
    rng = np.random.default_rng(11)
    pts = np.concatenate([rng.uniform(-5, 5, (900, 3)), lattice(rng, 300, voxel / 4, 4 * voxel)]).astype(np.float32)
    v = np.float32(voxel)
    g = gpu_map(voxel, s, 1 << 12)
    # two points in two sub-cells of one voxel (one sub-cell when s = 1: the first row keeps it) and a third one voxel
    # further, owned by the first frame; then the crowd
    g.insert(frame(np.array([[0.75, 0.25, 0.25], [1.25, 0.25, 0.25], [0.25, 0.25, 0.25]], np.float32) * v), EYE)
    g.insert(frame(pts), EYE)
    ties = np.array([[0.5, 0.25, 0.25], [1.0, 0.25, 0.25], [-1.0, -0.5, 0.125], [0.0, 0.0, 0.0]], np.float32) * v
    # a query with no voxel around it, and one exactly max_dist from a lonely point (d == max_dist; with max_dist == voxel too)
    lonely = np.array([[40.0, 40.0, 40.0]], np.float32) * v
    g.insert(frame(lonely + np.float32(0.25) * v), EYE)
    ex = g.export()
    edge = lonely + np.float32(0.25) * v + np.array([[0, np.float32(max_dist), 0]], np.float32)
    beyond = edge + np.array([[0, np.float32(max_dist) / 64, 0]], np.float32)
    q = np.concatenate([ties, np.array([[80.0, 0, 0]], np.float32), edge, beyond, lattice(rng, 200, voxel / 4, 4 * voxel),
                        rng.uniform(-6, 6, (317, 3)).astype(np.float32)])
    res, (key, sub, system) = g.register(frame(q, len(q) + 5), EYE, [(max_dist, 1)], debug=True)
    got = matches_of(key, sub, ex)
    win, near = L.search_exhaustive(q, ex, np.float32(voxel), s, max_dist, np.float32)
    assert near.all() and np.array_equal(got[:len(q)], win) and (got[len(q):] == -1).all()
    n = len(ties)
    assert win[n] == -1 and win[n + 1] >= 0 and win[n + 2] == -1, "no voxel around / d == max_dist / just beyond"
    d2 = L._d2(q[:, None, :], ex[3][None, :, :], np.float32)
    tied = int(((d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) > 1)[win >= 0].sum())
    assert tied >= (2 if s > 1 else 1), "exact ties are among the cases"
    assert system[27].item() == (win >= 0).sum()
    log(f"search voxel {voxel} s {s} max_dist {max_dist}: {len(q)} queries, {int((win >= 0).sum())} matched, {tied} exact ties, "
        f"all equal to the exhaustive search over {len(ex[0])} map points")


@pytest.mark.parametrize("kernel_scale", [0.0, 0.1])
def test_the_29_sums_on_the_kernels_own_matches(kernel_scale):
    rng = np.random.default_rng(17)
    world = I.room(3000, seed=31).astype(np.float32)
    g = gpu_map(1.0, 3, 1 << 13)
    g.insert(frame(world), EYE)
    ex = g.export()
    true = I.se3([0.01, -0.02, 0.03], [0.3, -0.2, 0.1])
    src = I.moved(world[rng.choice(len(world), 1100, replace=False)].astype(np.float64) + rng.normal(0, 0.01, (1100, 3)), true)
    src[7] += np.float32(0.6)                         # a gross outlier that still finds a match
    init = I.perturbed(true, seed=5, trans=0.05, deg=0.2)
    res, (key, sub, system) = g.register(frame(src, 1300), init, [(1.0, 1)], kernel_scale=kernel_scale, debug=True)
    system = system.cpu().numpy()
    win = matches_of(key, sub, ex)[:len(src)]
    assert win[7] >= 0 and (win >= 0).sum() > 1000
    S, parts = {}, {}
    for dtype in (np.float32, np.float64):
        q = I.transform(init, src, dtype)
        S[dtype], *parts[dtype] = L.system(q, win, ex[3], kernel_scale, dtype)
    J, e, w3 = parts[np.float64]
    q32 = I.transform(init, src, np.float32)
    delta = 4 * 2.0 ** -24 * max(float(np.abs(q32).max()), float(np.abs(ex[3]).max()))
    floor = L.system_floor(J, e, w3, kernel_scale, delta)
    bound = np.maximum(3 * np.abs(S[np.float32] - S[np.float64]), floor)
    err = np.abs(system - S[np.float64])
    assert system[27] == S[np.float64][27] == (win >= 0).sum()
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))))
    m = int(system[27])
    out_w = float(w3[int((win[:7] >= 0).sum())])
    log(f"sums kernel_scale {kernel_scale}: matches {m}/{len(src)}, max |gpu-r64| / bound over 29 sums {ratio:.3e}, "
        f"max |r32-r64| / |r64| {float(np.max(np.abs(S[np.float32] - S[np.float64]) / np.maximum(np.abs(S[np.float64]), 1e-300))):.3e}, "
        f"the outlier's weight {out_w:.3e}")
    assert (err <= bound).all(), (np.nonzero(err > bound)[0], err, bound)
    assert out_w == 1.0 if kernel_scale == 0 else out_w < 1e-2
    x, bad = I.solve(system)
    assert bad is None and int(res.iterations) == 1
    assert np.abs(res.pose[0].cpu().numpy() - I.update(init, x)).max() <= 1e-12


def test_empty_map_and_empty_frame_are_no_match_and_leave_the_pose():
    init = I.se3([0.1, 0.2, 0.3], [1.0, 2.0, 3.0])
    g = gpu_map()
    some = frame(np.zeros((5, 3), np.float32) + 0.5)
    for m, f in ((g, some), (gpu_map().insert(some, EYE), frame(np.zeros((0, 3), np.float32), 9))):
        res = m.register(f, init, [(1.0, 4)])
        assert int(res.status) == L.NO_MATCH and int(res.iterations) == 0 and float(res.fitness) == 0 and float(res.rmse) == 0
        assert res.pose[0].cpu().numpy().tobytes() == init.tobytes()
    # five copies of one point: a match for each, and a system no one can solve -- a result, not a NaN
    res = gpu_map().insert(some, EYE).register(some, EYE, [(1.0, 4)])
    assert int(res.status) == L.SINGULAR and res.pose[0].cpu().numpy().tobytes() == EYE.tobytes()


# --------------------------------------------------------------------------------------------------------------- known answer
@pytest.mark.parametrize("origin,bound_t", [((0.0, 0.0, 0.0), 1e-4), ((1000.0, -500.0, 20.0), 1e-3)])
def test_known_pose_is_recovered(origin, bound_t):
    pts, true, src, start = known_pose_case(origin)
    g = gpu_map(1.0, 3, 1 << 12, origin=origin, max_range=100.0)
    g.insert(frame((pts - np.asarray(origin)).astype(np.float32)), start)
    assert g.n_points == len(pts)
    res = g.register(frame(src, len(src) + 11), start, [(1.0, 40)])
    dt, dr = pose_error(res.pose[0].cpu().numpy(), true)
    log(f"known pose (0.3 m, 2 deg), map origin {origin}: status {int(res.status)}, iterations {int(res.iterations)}, "
        f"translation error {dt:.3e} m, rotation error {dr:.3e} rad, fitness {float(res.fitness):.3f}, rmse {float(res.rmse):.3e}")
    assert int(res.status) == L.CONVERGED and float(res.fitness) == 1.0
    assert dt <= bound_t and dr <= 1e-4, (dt, dr)
    # the points come back in world coordinates, float64, within fp32 of the map frame
    assert np.abs(np.sort(g.points(), axis=0) - np.sort(pts, axis=0)).max() < 1e-5


# -------------------------------------------------------------------------------------------------------------- repeatability
def test_same_bytes_twice_chained_stages_and_a_captured_graph():
    pts, true, src, start = known_pose_case()
    g = gpu_map(1.0, 3, 1 << 12)
    g.insert(frame(pts.astype(np.float32)), start)
    f = frame(src)
    init = torch.from_numpy(start).to(DEV)
    as_bytes = lambda r: [t.cpu().numpy().tobytes() for t in r]
    both = g.register(f, init, [(1.0, 2), (0.5, 6)], kernel_scale=0.2)
    again = g.register(f, init, [(1.0, 2), (0.5, 6)], kernel_scale=0.2)
    assert as_bytes(both) == as_bytes(again)
    first = g.register(f, init, [(1.0, 2)], kernel_scale=0.2)
    second = g.register(f, first.pose[0], [(0.5, 6)], kernel_scale=0.2)
    assert as_bytes(both)[:3] == as_bytes(second)[:3] and torch.equal(both.status, second.status)
    assert torch.equal(both.iterations, first.iterations + second.iterations) and int(first.iterations) == 2
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g.register(f, init, [(1.0, 1)])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = g.register(f, init, [(1.0, 2), (0.5, 6)], kernel_scale=0.2)
    graph.replay()
    torch.cuda.synchronize()
    assert as_bytes(captured) == as_bytes(both), "replayed from a captured graph"
