"""GPU: the batched ICP (csrc/icp.hip, ops.icp_refine, refine.py) against its numpy restatement (tests/icp_restated.py) and
against scenes whose answer is known.

One scan tensor of 4100-point capacity serves every test: a 40 x 30 x 6 m room as exact target (4100 points: two grid
chunks) and as noisy target (1500), exact sources (subsets of the target moved by a known pose; 1000 and 257 points: a ragged
last block), noisy sources (sampled independently), and a floor-only target.  Rows past a frame's length hold other room
points, which a kernel that ignored `lengths` would match.  max_dist 1.0 gives the fine grid (5 x 5 cells), 0.05 runs into
the 512-cell cap (3 x 3 cells).

Bounds:
  matches      equal to the exhaustive float32 search, except queries whose two best squared distances differ by less than
               4 float32 ulp of the larger -- at most 0.5 % of the queries, for the kernel and for float32 against float64.
  H, g, sums   against the float64 restatement ON THE KERNEL'S OWN MATCHES, per entry max(3 |r32 - r64|, floor): the
               project's three-way bound.  The floor is what an error of delta = 4 * 2^-24 * (largest coordinate) in the
               float32 transformed point can move the entry by (icp_restated.system_floor).  The match count is exact.
  exact scenes <= 1e-4 m and ||R - R_true||_F <= 1e-4 (the project's pose bar).
  noisy scenes final pose against the float64 restatement within max(3 |r32 - r64|, 1e-4), iteration count within 1.
Every observed figure goes to test_logs/icp_errors.log (scripts/icp_bench.py --accuracy -> profiles/icp_accuracy.md).
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restated as I  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 4100
METRICS = [("point", I.POINT), ("plane", I.PLANE)]
NORMALS_RADIUS = 2.0


def log(line):
    print(line)
    try:
        os.makedirs(os.path.join(ROOT, "test_logs"), exist_ok=True)
        with open(os.path.join(ROOT, "test_logs", "icp_errors.log"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


# ------------------------------------------------------------------------------------------------------------------ the scene
POSE = {1: I.se3([0.02, -0.03, 0.09], [1.5, -0.8, 0.2]), 3: I.se3([-0.01, 0.02, -0.12], [-0.7, 1.1, -0.1]),
        4: I.se3([0.03, 0.01, 0.05], [0.4, 0.9, 0.3]), 5: I.se3([0.0, -0.02, 0.2], [2.0, 0.5, 0.1]),
        7: I.se3([0.01, 0.02, -0.05], [0.6, -0.4, 0.1])}
TARGET = {1: 0, 3: 2, 4: 0, 5: 0, 7: 6}


def _scene():
    A = I.room(4100, seed=11).astype(np.float32)
    B = I.room(1500, seed=12, noise=0.02).astype(np.float32)
    floor = A[A[:, 2] == 0]
    frames = {0: A, 1: I.exact_source(A, 1000, POSE[1], seed=21), 2: B,
              3: I.moved(I.room(257, seed=13, noise=0.02), POSE[3]), 4: I.exact_source(A, 257, POSE[4], seed=24),
              5: I.moved(I.room(1000, seed=14, noise=0.02), POSE[5]), 6: floor,
              7: I.exact_source(floor, 300, POSE[7], seed=27)}
    pcd = np.zeros((len(frames), 3, N), np.float32)
    lengths = np.zeros(len(frames), np.int32)
    for f, pts in frames.items():
        fill = I.room(N, seed=100 + f).astype(np.float32)   # what lies past the length: plausible points that must not count
        fill[:len(pts)] = pts
        pcd[f], lengths[f] = fill.T, len(pts)
    return frames, pcd, lengths


FRAMES, PCD, LENGTHS = _scene()
PAIRS = [(1, 0), (4, 0), (3, 2), (0, 0), (5, 0)]   # a repeated target, source == target, unequal lengths
EXACT, NOISY = [(1, 0), (4, 0)], [(3, 2), (5, 0)]


def init_of(pair, trans=0.2, deg=1.0):
    s, d = pair
    return np.eye(4) if s == d else I.perturbed(POSE[s], seed=40 + s, trans=trans, deg=deg)


@pytest.fixture(scope="module")
def gpu():
    from deeppointmap_amd import ops
    pcd, lengths = torch.from_numpy(PCD).to(DEV), torch.from_numpy(LENGTHS).to(DEV)
    every = torch.arange(len(FRAMES), dtype=torch.int32, device=DEV)
    normals = ops.icp_target_normals(pcd, lengths, every, NORMALS_RADIUS)
    nrm = normals.cpu().numpy()
    for f in FRAMES:
        n = np.linalg.norm(nrm[f, :LENGTHS[f]], axis=1)
        assert np.abs(n - 1).max() < 1e-4 and not nrm[f, LENGTHS[f]:].any()
    return SimpleNamespace(pcd=pcd, lengths=lengths, normals=normals, nrm=nrm)


def prep(pairs, inits):
    src = torch.tensor([p[0] for p in pairs], dtype=torch.int32, device=DEV)
    dst = torch.tensor([p[1] for p in pairs], dtype=torch.int32, device=DEV)
    return src, dst, torch.from_numpy(np.stack(inits)).to(DEV)


def run(gpu, pairs, inits, schedule, metric, debug=False, prepped=None):
    from deeppointmap_amd import ops
    src, dst, init = prepped or prep(pairs, inits)
    return ops.icp_refine(gpu.pcd, gpu.lengths, src, dst, init, schedule, metric, normals=gpu.normals, debug=debug)


def as_bytes(outs, k):
    return [o[k].cpu().numpy().tobytes() for o in outs[:5]]


_RESTATED = {}


def restated(gpu, pair, metric, dtype, max_dist=1.0, max_iter=40):
    """a full run of the restatement, computed once per (pair, metric, precision)"""
    key = (pair, metric, np.dtype(dtype).name, max_dist, max_iter)
    if key not in _RESTATED:
        s, d = pair
        _RESTATED[key] = I.icp(FRAMES[s], FRAMES[d], gpu.nrm[d, :LENGTHS[d]], init_of(pair), max_dist, max_iter, metric, dtype=dtype)
    return _RESTATED[key]


# -------------------------------------------------------------------------------------------------------------- one iteration
@pytest.mark.parametrize("max_dist", [1.0, 0.05])
@pytest.mark.parametrize("name,metric", METRICS)
def test_one_iteration_matches_and_sums(gpu, name, metric, max_dist):
    trans, deg = (0.2, 1.0) if max_dist == 1.0 else (0.01, 0.02)
    inits = [init_of(p, trans, deg) for p in PAIRS]
    pose, fitness, rmse, iters, status, match, system = run(gpu, PAIRS, inits, [(max_dist, 1)], metric, debug=True)
    match, system = match.cpu().numpy(), system.cpu().numpy()
    queries = excused = flips = 0
    worst = 0.0
    for k, (s, d) in enumerate(PAIRS):
        src, tgt, nrm = FRAMES[s], FRAMES[d], gpu.nrm[d, :LENGTHS[d]]
        n1 = len(src)
        assert (match[k, n1:] == -1).all() and match[k, :n1].max() < len(tgt), "rows past a frame's length are neither queries nor targets"
        q32, win32, d1, d2 = I.match(inits[k], src, tgt, max_dist, np.float32)
        _, win64, e1, e2 = I.match(inits[k], src, tgt, max_dist, np.float64)
        tie = np.abs(e2 - e1) < 4 * np.spacing(np.maximum(e1, e2).astype(np.float32)).astype(np.float64)
        differs = match[k, :n1] != win32
        assert not (differs & ~tie).any(), (PAIRS[k], np.nonzero(differs & ~tie)[0][:8])
        queries, excused, flips = queries + n1, excused + int(differs.sum()), flips + int((win32 != win64).sum())
        # the sums, on the kernel's own matches
        win = match[k, :n1].astype(np.int64)
        S = {}
        for dtype in (np.float32, np.float64):
            J, e = I.rows(I.transform(inits[k], src, dtype), win, tgt, nrm, metric, dtype)
            S[dtype] = I.system(J, e, int((win >= 0).sum()), dtype)
        delta = 4 * 2.0 ** -24 * max(float(np.abs(q32).max()), float(np.abs(tgt).max()))
        floor = I.system_floor(J, e, delta)
        bound = np.maximum(3 * np.abs(S[np.float32] - S[np.float64]), floor)
        err = np.abs(system[k] - S[np.float64])
        assert system[k, 27] == S[np.float64][27] == (win >= 0).sum()
        ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))))
        worst = max(worst, ratio)
        log(f"one iteration {name} max_dist {max_dist} pair {PAIRS[k]}: matches {int(S[np.float64][27])}/{n1}, "
            f"differing from float32 exhaustive {int(differs.sum())}, max |gpu-r64| / bound over 29 sums {ratio:.3e}, "
            f"max |r32-r64| / |r64| {float(np.max(np.abs(S[np.float32] - S[np.float64]) / np.maximum(np.abs(S[np.float64]), 1e-300))):.3e}")
        assert (err <= bound).all(), (PAIRS[k], np.nonzero(err > bound)[0], err, bound)
        # the step the kernel took from these sums is the restatement's
        x, bad = I.solve(system[k])
        if bad is None:
            assert np.abs(pose[k].cpu().numpy() - I.update(inits[k], x)).max() <= 1e-12 and int(iters[k]) == 1
        else:
            assert int(status[k]) == bad and np.array_equal(pose[k].cpu().numpy(), inits[k]) and int(iters[k]) == 0
    log(f"one iteration {name} max_dist {max_dist}: {excused} of {queries} matches excused as ties, float32 against float64 "
        f"exhaustive differ on {flips}; worst sum ratio {worst:.3e}")
    assert excused <= 0.005 * queries and flips <= 0.005 * queries


# ------------------------------------------------------------------------------------------------------------------ full runs
@pytest.fixture(scope="module")
def full(gpu):
    """the five pairs, 40 iterations at most, both metrics: shared by the tests below"""
    inits = [init_of(p) for p in PAIRS]
    return {metric: run(gpu, PAIRS, inits, [(1.0, 40)], metric) for _, metric in METRICS}


@pytest.mark.parametrize("name,metric", METRICS)
def test_exact_scenes_recover_the_known_pose(gpu, full, name, metric):
    pose, fitness, rmse, iters, status = (t.cpu().numpy() for t in full[metric])
    for pair in EXACT:
        k = PAIRS.index(pair)
        dt = np.linalg.norm(pose[k, :3, 3] - POSE[pair[0]][:3, 3])
        dR = np.linalg.norm(pose[k, :3, :3] - POSE[pair[0]][:3, :3])
        log(f"exact scene {name} pair {pair}: |t - t_true| {dt:.3e} m, |R - R_true|_F {dR:.3e}, {iters[k]} iterations, "
            f"fitness {fitness[k]:.4f}, rmse {rmse[k]:.3e}, status {status[k]}")
        assert status[k] == I.CONVERGED and dt <= 1e-4 and dR <= 1e-4 and fitness[k] == 1.0
    k = PAIRS.index((0, 0))   # source == target from the identity: the identity comes back
    assert np.array_equal(pose[k], np.eye(4)) and status[k] == I.CONVERGED and fitness[k] == 1.0 and rmse[k] == 0.0
    assert np.array_equal(pose[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (len(PAIRS), 1)))


@pytest.mark.parametrize("name,metric", METRICS)
def test_noisy_scenes_against_the_restatement(gpu, full, name, metric):
    pose, fitness, rmse, iters, status = (t.cpu().numpy() for t in full[metric])
    for pair in NOISY:
        k = PAIRS.index(pair)
        r32, r64 = restated(gpu, pair, metric, np.float32), restated(gpu, pair, metric, np.float64)
        err, e = np.abs(pose[k] - r64["pose"]).max(), np.abs(r32["pose"] - r64["pose"]).max()
        log(f"noisy scene {name} pair {pair}: max |gpu - r64| {err:.3e}, max |r32 - r64| {e:.3e}, iterations gpu {iters[k]} "
            f"r32 {r32['iterations']} r64 {r64['iterations']}, fitness {fitness[k]:.4f} (r64 {r64['fitness']:.4f}), "
            f"rmse {rmse[k]:.4e} (r64 {r64['rmse']:.4e}), status {status[k]} (r64 {r64['status']})")
        assert err <= max(3 * e, 1e-4), (pair, err, e)
        assert abs(int(iters[k]) - r64["iterations"]) <= 1
        assert status[k] == r64["status"] or abs(int(iters[k]) - r64["iterations"]) == 1


# ----------------------------------------------------------------------------------------------------------------- degenerate
def test_degenerate_pairs_are_results_and_leave_the_others_alone(gpu, full):
    far = POSE[1].copy()
    far[:3, 3] += [500.0, 0.0, 0.0]
    pairs = [(1, 0)] + PAIRS[:2] + [(7, 6)] + PAIRS[2:]
    inits = [far] + [init_of(p) for p in PAIRS[:2]] + [init_of((7, 6), 0.05, 0.2)] + [init_of(p) for p in PAIRS[2:]]
    out = run(gpu, pairs, inits, [(1.0, 40)], I.PLANE)
    pose, fitness, rmse, iters, status = (t.cpu().numpy() for t in out)
    assert status[0] == I.NO_MATCH and pose[0].tobytes() == far.tobytes() and fitness[0] == 0 and iters[0] == 0
    assert status[3] == I.SINGULAR and np.isfinite(pose[3]).all() and np.array_equal(pose[3], inits[3])
    log(f"degenerate: floor-only target under the plane metric: status {status[3]}, fitness {fitness[3]:.3f}, rmse {rmse[3]:.3e}")
    assert np.isfinite(pose).all() and np.isfinite(fitness).all() and np.isfinite(rmse).all()
    others = [1, 2, 4, 5, 6]
    for k, j in enumerate(others):
        assert as_bytes(out, j) == as_bytes(full[I.PLANE], k), f"pair {PAIRS[k]} changed next to degenerate pairs"
    # the same floor under the point metric is a well-posed problem
    p2 = run(gpu, [(7, 6)], [inits[3]], [(1.0, 40)], I.POINT)
    assert int(p2[4][0]) == I.CONVERGED and np.abs(p2[0][0].cpu().numpy() - POSE[7]).max() <= 1e-4


# ---------------------------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("name,metric", METRICS)
def test_same_bytes_twice_in_any_order_and_from_a_graph(gpu, full, name, metric):
    inits = [init_of(p) for p in PAIRS]
    again = run(gpu, PAIRS, inits, [(1.0, 40)], metric)
    for k in range(len(PAIRS)):
        assert as_bytes(again, k) == as_bytes(full[metric], k)
    order = [3, 0, 4, 2, 1]
    shuffled = run(gpu, [PAIRS[i] for i in order], [inits[i] for i in order], [(1.0, 40)], metric)
    for k, i in enumerate(order):
        assert as_bytes(shuffled, k) == as_bytes(full[metric], i), f"pair {PAIRS[i]} depends on its place in the batch"
    # eight pairs: the launch then deals a pair's blocks to one XCD (another block-to-workgroup mapping, the same partials)
    eight = run(gpu, PAIRS + PAIRS[:3], inits + inits[:3], [(1.0, 40)], metric)
    for k in range(8):
        assert as_bytes(eight, k) == as_bytes(full[metric], k % len(PAIRS)), "a batch of eight"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(gpu, PAIRS, inits, [(1.0, 3)], metric)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    prepped = prep(PAIRS, inits)   # host-to-device copies stay outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(gpu, PAIRS, inits, [(1.0, 40)], metric, prepped=prepped)
    graph.replay()
    torch.cuda.synchronize()
    for k in range(len(PAIRS)):
        assert as_bytes(captured, k) == as_bytes(full[metric], k), "replayed from a captured graph"


# ------------------------------------------------------------------------------------------------------------------- schedule
def test_schedule_equals_chained_calls(gpu):
    from deeppointmap_amd import refine
    inits = [init_of(p) for p in PAIRS]
    src = torch.tensor([p[0] for p in PAIRS], dtype=torch.int32, device=DEV)
    dst = torch.tensor([p[1] for p in PAIRS], dtype=torch.int32, device=DEV)
    init = torch.from_numpy(np.stack(inits))
    kw = dict(metric="plane", normals=gpu.normals)
    both = refine.icp(gpu.pcd, gpu.lengths, src, dst, init, schedule=[(1.0, 10), (0.2, 20)], **kw)
    first = refine.icp(gpu.pcd, gpu.lengths, src, dst, init, max_dist=1.0, max_iter=10, **kw)
    second = refine.icp(gpu.pcd, gpu.lengths, src, dst, first.pose, max_dist=0.2, max_iter=20, **kw)
    assert torch.equal(both.pose, second.pose) and torch.equal(both.fitness, second.fitness)
    assert torch.equal(both.rmse, second.rmse) and torch.equal(both.status, second.status)
    assert torch.equal(both.iterations, first.iterations + second.iterations)
    log(f"schedule [(1.0, 10), (0.2, 20)]: iterations {both.iterations.tolist()}, status {both.status.tolist()}")


# ----------------------------------------------------------------------------------------------------------------- end to end
class _Stub(torch.nn.Module):
    def __init__(self, out=None):
        super().__init__()
        self.out = out

    def set_train_stage(self, stage):
        return self

    def forward(self, pcd, mask):
        return self.out


class _Seen(Exception):
    pass


def test_table_end_to_end_into_the_training_step(gpu, monkeypatch):
    """six frames of one exact scene (the same 4096 world points seen from six sensor poses), global poses off by 0.1 m and
    0.5 degrees: the table holds the true relative poses, and the training step's ops.map_poses returns them"""
    from deeppointmap_amd import ops, refine
    from deeppointmap_amd.train_pipeline import DeepPointModelPipeline
    n, Fr = 4096, 6
    world = I.room(n, seed=31)
    truth = [I.se3([0.0, 0.0, np.radians(0.5 * f)], [0.5 * f, 0.1 * f, 0.0]) for f in range(Fr)]
    rng = np.random.default_rng(32)
    scans = torch.from_numpy(np.ascontiguousarray(np.stack([I.moved(world, truth[f])[rng.permutation(n)].T for f in range(Fr)]))).to(DEV)
    noisy = [I.perturbed(truth[f], seed=50 + f, trans=0.1, deg=0.5) for f in range(Fr)]
    R, T = np.stack([M[:3, :3] for M in noisy]), np.stack([M[:3, 3:] for M in noisy])
    table = refine.build_refined_table(scans, R, T, distance=100.0, batch_pairs=4, min_fitness=0.5, max_shift=1.0,
                                       max_dist=1.0, max_iter=40, metric="plane", normals_radius=NORMALS_RADIUS)
    assert sorted(table) == [(i, j) for i in range(Fr) for j in range(i + 1, Fr)]
    worst = 0.0
    for (i, j), M in table.items():
        want = np.linalg.inv(truth[i]) @ truth[j]
        assert M.dtype == np.float64 and M.shape == (4, 4)
        worst = max(worst, float(np.linalg.norm(M[:3, 3] - want[:3, 3])))
        assert np.linalg.norm(M[:3, 3] - want[:3, 3]) <= 1e-4 and np.linalg.norm(M[:3, :3] - want[:3, :3]) <= 1e-4, (i, j)
    log(f"end to end: 15 table entries of 6 frames, worst |t - t_true| {worst:.3e} m")
    # the training step reads it
    S, S1 = Fr, 3
    seen = {}

    def spy(*args, **kw):
        seen["rel"], seen["gt"] = real(*args, **kw)
        raise _Seen

    real = ops.map_poses
    monkeypatch.setattr(ops, "map_poses", spy)
    coor = torch.zeros(Fr, 3, 8, device=DEV)
    model = DeepPointModelPipeline(SimpleNamespace(), _Stub((coor, torch.zeros(Fr, 4, 8, device=DEV), torch.zeros(Fr, 8, dtype=torch.bool, device=DEV))),
                                   _Stub(), None)
    model.refined_SE3_cache["scene"] = table
    info = {"num_map": 1, "dsf_index": [(0, 0, f) for f in range(Fr)], "refined_SE3_file": ["scene"]}
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(DEV)   # noqa: E731
    with pytest.raises(_Seen):
        model(scans, f32(R), f32(T), torch.zeros(Fr, n, dtype=torch.bool, device=DEV), torch.eye(4, device=DEV).repeat(Fr, 1, 1), info, s1=S1)
    rel, gt = seen["rel"].cpu().numpy().reshape(Fr, 3, 4), seen["gt"].cpu().numpy().reshape(3, 4)
    for s in (1, 2, 4, 5):
        first = 0 if s < S1 else S1
        want = np.linalg.inv(truth[first]) @ truth[s]
        glob = np.linalg.inv(noisy[first]) @ noisy[s]
        assert np.abs(rel[s] - table[(first, s)][:3]).max() <= 1e-6, "the table's entry in float32"
        assert np.abs(rel[s] - want[:3]).max() <= 1e-4 + 1e-6
        assert np.abs(rel[s] - glob[:3]).max() > 0.02, "the perturbed global poses are somewhere else"
    assert np.abs(gt - (np.linalg.inv(truth[S1]) @ truth[0])[:3]).max() <= 1e-4 + 1e-5
