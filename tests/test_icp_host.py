"""CPU: the ICP restatement on scenes with a known answer, the refined-pose table's convention through
train_pipeline.refined_pose / icp_table, candidate_pairs, the rejection filter, and the ABI rows."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_restated as I  # noqa: E402

TRUE_POSE = I.se3([0.02, -0.03, 0.09], [1.5, -0.8, 0.2])


@pytest.mark.parametrize("metric", [I.POINT, I.PLANE])
@pytest.mark.parametrize("n1,n2", [(257, 1500), (1000, 4100)])
def test_restatement_recovers_exact_scenes(metric, n1, n2):
    """the source is a subset of the target moved by a known pose: both precisions come back to it (the float32 of the
    moved coordinates is all that separates the answer from the pose)"""
    tgt = I.room(n2, seed=n2).astype(np.float32)
    src = I.exact_source(tgt, n1, TRUE_POSE, seed=n1)
    normals = np.zeros((n2, 3))   # the exact planes: floor z = 0, walls at x = +-20 / y = +-15
    t64 = tgt.astype(np.float64)
    normals[:, 2] = t64[:, 2] == 0
    normals[:, 0] = (np.abs(np.abs(t64[:, 0]) - 20) < 1e-4) & (normals[:, 2] == 0)
    normals[:, 1] = (normals[:, 0] == 0) & (normals[:, 2] == 0)
    init = I.perturbed(TRUE_POSE, seed=3, trans=0.2, deg=1.0)
    ends = {}
    for dtype in (np.float32, np.float64):
        r = I.icp(src, tgt, normals, init, max_dist=1.0, max_iter=30, metric=metric, dtype=dtype)
        assert r["status"] == I.CONVERGED and r["iterations"] <= 8, r
        assert np.linalg.norm(r["pose"][:3, 3] - TRUE_POSE[:3, 3]) <= 5e-6
        assert np.linalg.norm(r["pose"][:3, :3] - TRUE_POSE[:3, :3]) <= 5e-6
        assert r["fitness"] == 1.0
        ends[dtype] = r["pose"]
    assert np.abs(ends[np.float32] - ends[np.float64]).max() <= 5e-6


def test_restatement_search_shortcut_equals_exhaustive():
    """the cKDTree candidate path of icp_restated.nearest gives what the exhaustive search gives, in both precisions"""
    tgt = I.room(1500, seed=7, noise=0.02).astype(np.float32)
    src = I.moved(I.room(257, seed=8, noise=0.02), TRUE_POSE)
    for dtype in (np.float32, np.float64):
        q = I.transform(I.perturbed(TRUE_POSE, 9), src, dtype)
        fast, slow = I.nearest(q, tgt, dtype), I.nearest(q, tgt, dtype, exhaustive=True)
        assert all(np.array_equal(a, b) for a, b in zip(fast, slow))


def test_restatement_degenerate_systems():
    tgt = I.room(600, seed=1).astype(np.float32)
    src = I.exact_source(tgt, 100, TRUE_POSE, seed=2)
    far = TRUE_POSE.copy()
    far[0, 3] += 500
    r = I.icp(src, tgt, None, far, metric=I.POINT)
    assert r["status"] == I.NO_MATCH and r["fitness"] == 0 and np.array_equal(r["pose"], far)
    floor = tgt[tgt[:, 2] == 0]
    n = np.tile([0.0, 0.0, 1.0], (len(floor), 1))
    r = I.icp(I.exact_source(floor, 100, TRUE_POSE, seed=2), floor, n, I.perturbed(TRUE_POSE, 4, 0.05, 0.2), metric=I.PLANE)
    assert r["status"] == I.SINGULAR and np.isfinite(r["pose"]).all()


def _table():
    rng = np.random.default_rng(0)
    return {(i, j): I.se3(rng.normal(size=3) * 0.1, rng.normal(size=3)) for i, j in [(0, 1), (0, 2), (2, 5), (0, 5)]}


def test_table_round_trip_and_lookup(tmp_path):
    from deeppointmap_amd import refine
    from deeppointmap_amd.train_pipeline import icp_table, refined_pose
    table = _table()
    path = str(tmp_path / "refined_SE3.pkl")
    refine.write_refined_table(path, table)
    back = refine.read_refined_table(path)
    assert sorted(back) == sorted(table)
    for k, M in table.items():
        assert back[k].dtype == np.float64 and back[k].shape == (4, 4) and np.array_equal(back[k], M)
    assert np.array_equal(refined_pose(back, 2, 0), table[(0, 2)])                           # s > d: the entry
    assert np.allclose(refined_pose(back, 0, 2), np.linalg.inv(table[(0, 2)]), atol=1e-12)   # s < d: its inverse
    assert np.array_equal(refined_pose(back, 3, 3), np.eye(4))                               # s == d
    assert refined_pose(back, 1, 2) is None                                                  # no entry, no bridge
    want = np.linalg.inv(table[(0, 2)]) @ table[(0, 1)]   # frame 1 in frame 2 over the bridge 0: (0 -> 2) @ (1 -> 0)
    assert np.allclose(refined_pose(back, 1, 2, bridge=0), want, atol=1e-12)
    # one map of frames [0, 1, 2 | 5, 4]: entries exactly where the table answers
    icp, has = icp_table(np.array([[0, 1, 2, 5, 4]]), [back], 3)
    #           s=0  s=1  s=2  s=3  s=4 (4 -> 5 has no entry; bridge 0: (0,4) missing)   F+b: 0 -> 5
    assert has.tolist() == [0, 1, 1, 0, 0, 1]
    assert np.array_equal(icp[1].reshape(4, 4), table[(0, 1)].astype(np.float32))
    assert np.allclose(icp[5].reshape(4, 4), np.linalg.inv(table[(0, 5)]), atol=1e-6)


def test_candidate_pairs_against_brute_force():
    from deeppointmap_amd import refine
    rng = np.random.default_rng(5)
    T = np.cumsum(rng.normal(size=(60, 3)) * [2.0, 2.0, 0.1], axis=0)
    for distance in (0.0, 3.0, 9.75, 1e9):
        d = np.linalg.norm(T[:, None] - T[None], axis=2)
        want = [(i, j) for i in range(60) for j in range(i + 1, 60) if d[i, j] <= distance]
        got = refine.candidate_pairs(T.reshape(60, 3, 1), distance)
        assert got.dtype == np.int64 and got.shape == (len(want), 2) and [tuple(p) for p in got.tolist()] == want
    assert refine.candidate_pairs(np.zeros((1, 3)), 1.0).shape == (0, 2)


def test_relative_poses_are_frame_j_in_frame_i():
    from deeppointmap_amd import refine
    poses = np.stack([I.se3([0.0, 0.0, 0.1 * k], [k, 0.5 * k, 0.0]) for k in range(4)])
    rel = refine.relative_poses(poses[:, :3, :3], poses[:, :3, 3:], [(0, 2), (1, 3)])
    assert np.allclose(rel[0], np.linalg.inv(poses[0]) @ poses[2], atol=1e-12)
    assert np.allclose(rel[1], np.linalg.inv(poses[1]) @ poses[3], atol=1e-12)


def test_rejection_filter():
    from deeppointmap_amd import refine
    init = np.tile(np.eye(4), (6, 1, 1))
    pose = init.copy()
    pose[4, 0, 3] = 3.0          # moved further than max_shift
    pose[5, 1, 3] = 1.9          # inside
    result = refine.IcpResult(torch.from_numpy(pose), torch.tensor([0.9, 0.9, 0.9, 0.2, 0.9, 0.3]), torch.zeros(6),
                              torch.zeros(6, dtype=torch.int32),
                              torch.tensor([refine.CONVERGED, refine.NO_MATCH, refine.SINGULAR, refine.CONVERGED,
                                            refine.MAX_ITER, refine.MAX_ITER], dtype=torch.int32))
    keep = refine.accept(result, init, min_fitness=0.3, max_shift=2.0)
    assert keep.tolist() == [True, False, False, False, False, True]


def test_abi_rows_exist():
    from deeppointmap_amd import _lib, ops
    assert _lib.SIGNATURES["dpm_icp_workspace_bytes"][1] == [_lib.I, _lib.I]
    assert len(_lib.SIGNATURES["dpm_icp_refine_batched"][1]) == 24
    lib = _lib.load()
    small, big = lib.dpm_icp_workspace_bytes(1, 257), lib.dpm_icp_workspace_bytes(5, 4100)
    assert 0 < small < big and lib.dpm_icp_workspace_bytes(0, 10) == 0
    assert (ops.ICP_CONVERGED, ops.ICP_MAX_ITER, ops.ICP_NO_MATCH, ops.ICP_SINGULAR) == (I.CONVERGED, I.MAX_ITER, I.NO_MATCH, I.SINGULAR)
    with pytest.raises(_lib.DpmError):   # no CPU fallback
        ops.icp_refine(torch.zeros(1, 3, 8), torch.full((1,), 8, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                       torch.zeros(1, dtype=torch.int32), torch.eye(4, dtype=torch.float64)[None], [(1.0, 1)], ops.ICP_POINT)
