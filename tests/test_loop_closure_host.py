"""CPU: the graph side of the loop closer (deeppointmap_amd/loop_closure.py) on plain poses.  The optimiser is host code in the
library, so none of this needs a GPU: a consistent graph comes back unchanged, exact loop edges take a yaw drift out, and
the accept rule is tested on hand-made IcpResults."""
import math

import numpy as np
import torch

from deeppointmap_amd import loop_closure as LC
from deeppointmap_amd.refine import CONVERGED, MAX_ITER, NO_MATCH, SINGULAR, IcpResult


def rz(a, t=(0.0, 0.0, 0.0)):
    T = LC._rz(a)
    T[:3, 3] = t
    return T


def square(n_side=10, step=2.0, laps=1, offset=0.0):
    """poses on a square of n_side steps a side, heading along the side; lap k runs `offset` * k metres to the right"""
    out = []
    for lap in range(laps):
        for side in range(4):
            th = side * 0.5 * math.pi
            corner = np.array([(0, 0), (1, 0), (1, 1), (0, 1)][side], float) * n_side * step
            for k in range(n_side):
                p = corner + k * step * np.array([math.cos(th), math.sin(th)]) + lap * offset * np.array([math.sin(th), -math.cos(th)])
                out.append(rz(th, (p[0], p[1], 0.3 * math.sin(k))))
    return np.stack(out)


def relative(poses, s, t):
    """X of an edge (s, t): source-scan coordinates -> the target's frame"""
    return np.linalg.inv(poses[t]) @ poses[s]


def info(w_rot=400.0, w_trans=100.0):
    return np.diag([w_rot] * 3 + [w_trans] * 3)


def ate(est, truth):
    return float(np.sqrt((np.linalg.norm(est[:, :3, 3] - truth[:, :3, 3], axis=1) ** 2).mean()))


def test_consistent_graph_comes_back_unchanged():
    truth = square()
    assert len(truth) == 40
    edges = [(i, i - 1, relative(truth, i, i - 1), info()) for i in range(1, 40)]
    edges.append((39, 0, relative(truth, 39, 0), info()))
    out = LC.optimise_graph(truth, edges)
    assert out.shape == (40, 4, 4) and out.dtype == np.float64
    assert np.abs(out - truth).max() < 1e-9


def drifted(truth, bias):
    out = [truth[0].copy()]
    for k in range(1, len(truth)):
        out.append(out[-1] @ relative(truth, k, k - 1) @ rz(bias))
    return np.stack(out)


def test_exact_loop_edges_take_a_yaw_drift_out():
    truth = square(laps=2, offset=0.3)
    given = drifted(truth, 0.002)
    n, per_lap = len(truth), len(truth) // 2
    edges = [(i, i - 1, relative(given, i, i - 1), info()) for i in range(1, n)]          # what a drifting odometry measured
    loops = [(i, i - per_lap) for i in range(per_lap, n, 5)]
    edges += [(s, t, relative(truth, s, t), info()) for s, t in loops]                   # exact loop measurements
    out = LC.optimise_graph(given, edges)
    assert np.array_equal(out[0], given[0])                                              # node 0 is held
    before, after = ate(given, truth), ate(out, truth)
    assert after < before, (before, after)
    for s, t in loops:
        want = relative(truth, s, t)
        d0 = np.linalg.norm((np.linalg.inv(want) @ relative(given, s, t))[:3, 3])
        d1 = np.linalg.norm((np.linalg.inv(want) @ relative(out, s, t))[:3, 3])
        a0 = abs(LC.yaw_between(want[None], relative(given, s, t)[None])[0])
        a1 = abs(LC.yaw_between(want[None], relative(out, s, t)[None])[0])
        assert d1 < d0 and a1 < a0, (s, t, d0, d1, a0, a1)


def test_loop_closer_without_loops_returns_its_poses_and_edges_follow_the_convention():
    lc = LC.LoopCloser(capacity=4, points_per_frame=8)
    assert lc.optimise().shape == (0, 4, 4) and lc.edges() == []
    truth = square()[:3]
    lc.poses = [p.copy() for p in truth]
    assert np.array_equal(lc.optimise(), truth)
    lc._odometry_info = [torch.eye(6), torch.zeros(6, 6)]
    (s0, t0, X0, I0), (s1, t1, X1, I1) = lc.edges()
    assert (s0, t0, s1, t1) == (1, 0, 2, 1) and np.allclose(truth[0] @ X0, truth[1]) and np.allclose(truth[1] @ X1, truth[2])
    assert np.array_equal(I0, np.eye(6)) and np.array_equal(I1, np.eye(6))     # an edge without correspondences keeps a weight


def result(poses, fitness, status):
    n = len(poses)
    return IcpResult(torch.from_numpy(np.stack(poses)), torch.tensor(fitness, dtype=torch.float32), torch.zeros(n),
                     torch.zeros(n, dtype=torch.int32), torch.tensor(status, dtype=torch.int32))


def test_accept_rule_on_hand_made_results():
    init = np.stack([rz(0.5)] * 9)
    nan = np.full((4, 4), np.nan)
    poses = [rz(0.5, (1, 0, 0)), rz(0.5, (1, 0, 0)), rz(0.5, (1, 0, 0)), rz(0.5, (1, 0, 0)), rz(0.5, (1, 0, 0)),
             rz(0.5, (3, 4, 0.1)), rz(0.5, (3, 4, 0)), rz(0.5 + 0.21, (0, 0, 0)), nan]
    fitness = [0.9, 0.9, 0.9, 0.9, 0.39, 0.9, 0.9, 0.9, 0.9]
    status = [CONVERGED, MAX_ITER, NO_MATCH, SINGULAR, CONVERGED, CONVERGED, CONVERGED, CONVERGED, CONVERGED]
    ok = LC.accept_loops(result(poses, fitness, status), init, min_fitness=0.4, max_offset=5.0, max_yaw_change=0.2)
    assert ok.tolist() == [True, True, False, False, False, False, True, False, False]
    # the yaw is measured from the start, across the +-pi seam, whatever roll and pitch the registration added
    init = np.stack([rz(math.pi - 0.05)] * 2)
    tilt = np.eye(4)
    tilt[:3, :3] = [[1, 0, 0], [0, math.cos(0.02), -math.sin(0.02)], [0, math.sin(0.02), math.cos(0.02)]]
    poses = [rz(-math.pi + 0.05) @ tilt, rz(-math.pi + 0.2) @ tilt]
    ok = LC.accept_loops(result(poses, [0.9, 0.9], [CONVERGED, CONVERGED]), init, 0.4, 5.0, 0.2)
    assert ok.tolist() == [True, False]
    assert abs(LC.yaw_between(rz(0.3)[None], rz(-0.4)[None])[0] + 0.7) < 1e-12


def test_scan_context_parameters_are_checked_on_the_host():
    import pytest
    for kw in (dict(rings=0), dict(rings=33), dict(sectors=2), dict(sectors=66), dict(sectors=7), dict(min_range=5.0, max_range=4.0)):
        with pytest.raises(ValueError):
            LC.ScanContext(**kw)
    sc = LC.ScanContext()
    assert sc.tables[0].shape == (20,) and sc.tables[1].shape == (29, 2) and sc.tables[0].dtype == np.float32
    assert sc.tables[0][-1] == np.float32(6400.0) and abs(sc.yaw(15) - 0.5 * math.pi) < 1e-15
