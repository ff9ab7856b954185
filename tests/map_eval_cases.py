"""Scenes, clouds and hand-made rule cases shared by tests/test_evaluate_host.py and tests/test_gpu_map_eval.py."""
import math
import os
from types import SimpleNamespace

import numpy as np

import lidar_sim_cases as LC
import lidar_sim_restated as LR
from deeppointmap_amd import lidar_sim as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

DIST_BOUND = 1e-3        # |dist32 - dist64|: the simulator's bound (one twentieth of a 2 cm range noise)
GAP = 2e-3               # ids are compared where the two nearest surfaces are further apart than this (twice the bound)
EXCLUDED_CAP = 0.01      # at most this share of a test's points may fall under the gap


def log(line):
    """what a test observed: test_logs/map_eval_errors.log (DESIGN.md 7h quotes it)"""
    print(line)
    try:
        os.makedirs(os.path.join(ROOT, "test_logs"), exist_ok=True)
        with open(os.path.join(ROOT, "test_logs", "map_eval_errors.log"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def bbox_centre(points):
    """float64 centre of the bounding box of the finite points of a (3,M) float32 cloud"""
    p = np.asarray(points)
    ok = np.isfinite(p).all(axis=0)
    if not ok.any():
        return [0.0, 0.0, 0.0]
    q = p[:, ok].astype(np.float64)
    return (0.5 * (q.min(axis=1) + q.max(axis=1))).tolist()


def world_points(xyz, pose):
    """(n,3) float32 sensor-frame points, (4,4) float64 pose -> (3,n) float32 world points: moved in float64, rounded once"""
    w = np.asarray(xyz).astype(np.float64) @ pose[:3, :3].T + pose[:3, 3]
    return np.ascontiguousarray(w.T.astype(f32))


# ------------------------------------------------------------------------------------------------------------
# scene distance against the float32 restatement: mixed scenes of P primitives, M points of every kind
# ------------------------------------------------------------------------------------------------------------
def mixed_scene(P, ground=True):
    """P yawed boxes and cylinders (two to one) over a 60 m square, many overlapping; P = 0: the ground alone"""
    return LC.random_scene(31 + P, P, 30.0, z0=0.0 if ground else None)


def mixed_points(scene, M, seed=5):
    """(3,M) float32: random points over the scene's volume, then -- as far as M has room, from the END, so that M = 1 is
    a random point -- primitive centres (inside), points on +x faces / on the side of cylinders, points on the ground, and
    one row with a NaN"""
    rng = np.random.Generator(np.random.PCG64(seed + 7 * M + scene.P))
    pts = np.stack([rng.uniform(-34, 34, M), rng.uniform(-34, 34, M), rng.uniform(-1.0, 12.0, M)]).astype(f32)
    special = []
    q, kind = scene.params, scene.kind
    for p in range(min(scene.P, 40)):
        x, y, z, e0, e1, e2, yaw = q[p]
        if kind[p] == 0:
            special.append((x, y, z))
            special.append((x + math.cos(yaw) * e0, y + math.sin(yaw) * e0, z))
        else:
            special.append((x, y, z + 0.5 * e1))
            special.append((x + e0, y, z + 0.25 * e1))
    special += [(3.0, -2.0, 0.0), (float("nan"), 1.0, 1.0)]
    special = special[-max(M - 1, 0):] if M > 1 else []
    for k, s in enumerate(special[:M - 1]):
        pts[:, M - 1 - k] = np.asarray(s, np.float64).astype(f32)
    return np.ascontiguousarray(pts)


# ------------------------------------------------------------------------------------------------------------
# hand-made rule cases: answers that are exact in float32
# ------------------------------------------------------------------------------------------------------------
def rule_cases():
    """[case]: name, scene, points (3,n) float32, want_dist, want_surf.  The box is yawed by pi / 2: cos rounds to 6e-17, which
    changes no float32 result below and float64 results by less than 1e-15."""
    cases = []

    def case(name, scene, pts, want):
        cases.append(SimpleNamespace(name=name, scene=scene, points=np.ascontiguousarray(np.asarray(pts, f32).T.reshape(3, -1)),
                                     want_dist=[w[0] for w in want], want_surf=[w[1] for w in want]))

    s = LS.Scene(z0=None)         # centre (10, 20, 2), half extents (2, 1, 1) along ITS axes: +-1 in world x, +-2 in world y
    s.add_box((10, 20, 2), (2, 1, 1), yaw=0.5 * math.pi)
    case("yawed box: face, edge, vertex, inside", s,
         [(14, 20, 2), (14, 26, 2), (13, 25, 9), (10.5, 20, 2), (10, 20, 2)],
         [(3.0, 0), (5.0, 0), (7.0, 0), (0.5, 0), (1.0, 0)])

    s = LS.Scene(z0=None)         # base (0, 0, 0), radius 1, height 4
    s.add_cylinder((0, 0, 0), 1.0, 4.0)
    case("cylinder: inside, above the cap, beyond the rim, beside", s,
         [(0.25, 0, 2), (0.5, 0, 7), (4, 0, 8), (0, -3, 1)],
         [(0.75, 0), (3.0, 0), (5.0, 0), (2.0, 0)])

    s = LS.Scene(z0=None)         # two coincident boxes, and a third further off: the lower index wins the tie
    s.add_box((0, 0, 0), (1, 1, 1)), s.add_box((8, 0, 0), (1, 1, 1)), s.add_box((0, 0, 0), (1, 1, 1))
    case("tie between two primitives", s, [(3, 0, 0), (4, 0, 0)], [(2.0, 0), (3.0, 0)])

    s = LS.Scene(z0=0.0)          # a box floating 2 m up: one metre below it is one metre above the ground; the primitive wins
    s.add_box((0, 0, 3), (1, 1, 1))
    case("tie with the ground", s, [(0, 0, 1), (0, 0, 0.5), (5, 0, 0)], [(1.0, 0), (0.5, 1), (0.0, 1)])

    case("empty scene without ground", LS.Scene(z0=None), [(1, 2, 3)], [(math.inf, -1)])
    case("ground alone and a NaN row", LS.Scene(z0=-1.0), [(1, 2, 3), (1, math.nan, 3)], [(4.0, 0), (math.inf, -1)])
    return cases


# ------------------------------------------------------------------------------------------------------------
# noisy returns of a scene, for the float64 comparison
# ------------------------------------------------------------------------------------------------------------
def noisy_returns(scene, poses, model, sigma, seed):
    """the float64 restatement's returns of every pose with N(0, sigma) range noise, moved to the world in float64 and
    rounded to float32: (3,M) float32"""
    rng = np.random.Generator(np.random.PCG64(seed))
    dirs = model.directions().astype(np.float64)
    out = []
    for M in poses:
        r, prim, _ = LR.cast64(scene.params, scene.kind, scene.z0, M, model.directions(), model.min_range, model.max_range)
        hit = prim >= 0
        t = r[hit] + sigma * rng.standard_normal(int(hit.sum()))
        out.append(((t[:, None] * dirs[hit]) @ M[:3, :3].T + M[:3, 3]).T.astype(f32))
    return np.ascontiguousarray(np.concatenate(out, axis=1))


FAR_NOISE_SEED = 3


def far_cloud():
    """lidar_sim_cases.scene_far (1 km from the origin) scanned with SMALL16 from its two poses, 2 cm noise"""
    scene, poses, _ = LC.scene_far()
    return scene, noisy_returns(scene, poses, LS.SMALL16, 0.02, FAR_NOISE_SEED)


# ------------------------------------------------------------------------------------------------------------
# neighbour-search clouds
# ------------------------------------------------------------------------------------------------------------
def nn_cases():
    """[case]: name, query (3,Nq), target (3,Nt) float32, max_dist, origin"""
    cases = []

    def case(name, q, t, max_dist, origin=(0.0, 0.0, 0.0)):
        cases.append(SimpleNamespace(name=name, query=np.ascontiguousarray(np.asarray(q, f32).reshape(3, -1)),
                                     target=np.ascontiguousarray(np.asarray(t, f32).reshape(3, -1)), max_dist=max_dist,
                                     origin=[float(v) for v in origin]))

    def rand(seed, n, scale=(20.0, 20.0, 3.0), centre=(0.0, 0.0, 0.0)):
        rng = np.random.Generator(np.random.PCG64(seed))
        return (np.asarray(centre).reshape(3, 1) + rng.uniform(-1, 1, (3, n)) * np.asarray(scale).reshape(3, 1)).astype(f32)

    case("no target", rand(1, 1), np.zeros((3, 0), f32), 0.5)
    case("one and one", [[0.25], [0.0], [0.0]], [[0.0], [0.0], [0.0]], 0.5)
    # 257 x 300: duplicated targets (ties), a query at exactly max_dist (in) and one just beyond (out), both representable
    t = rand(2, 300, scale=(4.0, 4.0, 1.0))
    t[:, 150:300] = t[:, 0:150]                              # every target twice: the lower index must win
    q = rand(3, 257, scale=(4.0, 4.0, 1.0))
    q[:, :100] = t[:, 40:140]                                # queries on targets: distance 0, tie between the two copies
    t[:, 7], t[:, 157] = (64.0, 0.0, 0.0), (64.0, 0.0, 0.0)
    q[:, 255], q[:, 256] = (64.5, 0.0, 0.0), (64.50001, 0.0, 0.0)    # 0.5 exactly; 64.50001 rounds to 64.5 + one ulp
    case("ties and the boundary", q, t, 0.5)
    case("all targets at one position", rand(4, 257, scale=(0.4, 0.4, 0.4), centre=(5.0, 5.0, 5.0)),
         np.tile(np.asarray([[5.0], [5.0], [5.0]], f32), (1, 300)), 0.5)
    # non-finite coordinates: such a target is nobody's neighbour, such a query has none
    t, q = rand(11, 300, scale=(3.0, 3.0, 1.0)), rand(12, 257, scale=(3.0, 3.0, 1.0))
    t[0, 5], t[2, 6], t[1, 7] = np.nan, np.inf, -np.inf
    q[0, 3], q[1, 4], q[2, 5] = np.nan, np.inf, -np.inf
    case("non-finite coordinates", q, t, 0.5)
    # two clusters 5 km apart with max_dist 0.1: 50 000 cells per axis wanted, 128 given -- the edge grows
    t = np.concatenate([rand(5, 2500, scale=(1.0, 1.0, 0.5)), rand(6, 2500, scale=(1.0, 1.0, 0.5), centre=(5000.0, 0.0, 0.0))], axis=1)
    q = np.concatenate([rand(7, 2048, scale=(1.0, 1.0, 0.5)), rand(8, 2049, scale=(1.0, 1.0, 0.5), centre=(5000.0, 0.0, 0.0))], axis=1)
    case("two clusters 5 km apart", q, t, 0.1, origin=(2500.0, 0.0, 0.0))
    # 1 km from the supplied origin's opposite: the shift brings the cloud to the origin's neighbourhood
    c = (1000.0, -1000.0, 30.0)
    case("1 km from the world's origin", rand(9, 4097, centre=c), rand(10, 5000, centre=c), 0.75, origin=c)
    return cases


# ------------------------------------------------------------------------------------------------------------
# simulated scans of a street scene (GPU tests 5-7)
# ------------------------------------------------------------------------------------------------------------
STREET_SEED = 2
SHIFT = 0.3


def street():
    """street_scene(STREET_SEED), 8 poses of its circuit about 15 m apart, and the same poses with every second one
    shifted by SHIFT m along world x"""
    scene = LS.street_scene(STREET_SEED, blocks=(2, 2))
    poses = LS.circuit(scene, 15.0)[:8].copy()
    shifted = poses.copy()
    shifted[1::2, 0, 3] += SHIFT
    return scene, poses, shifted
