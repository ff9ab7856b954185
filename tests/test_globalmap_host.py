"""CPU: the pieces of the global map that need no GPU -- the binary PCD writer, the fp64 numpy restatement of open3d's
VoxelDownSample that the GPU tests hold csrc/voxel_map.hip to (checked here against hand-worked cases: a test of the test),
and that `slam_system.result_maps` is off unless a configuration turns it on."""
import numpy as np
import pytest


def _round32(s: np.ndarray, e: np.ndarray) -> np.ndarray:
    """the fp32 rounding of the exact value s + e (s = fp64 sum, e = its TwoSum error): rounding s alone is right unless s is
    exactly halfway between two fp32 values and e != 0, where e decides (a plain fp64 -> fp32 cast would round twice)"""
    r = s.astype(np.float32)
    d = s - r.astype(np.float64)                            # exact
    nb = np.nextafter(r, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    mid = (d != 0) & (2 * np.abs(d) == np.abs(nb.astype(np.float64) - r.astype(np.float64))) & (e != 0)
    away = mid & (np.sign(e) == np.sign(d))
    return np.where(away, nb, r).astype(np.float32)


def _sum32(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """fp32(a + b) of two fp64 values, correctly rounded (TwoSum)"""
    s = a + b
    bb = s - a
    e = (a - (s - bb)) + (b - bb)
    return _round32(s, e)


def transform_fp32(xyz: np.ndarray, se3: np.ndarray) -> np.ndarray:
    """(3,N) fp32 cloud, (4,4) pose -> (3,N) fp32, bit for bit the kernel's arithmetic (csrc/voxel_map.hip xform, as
    dpm_map_tile): w_a = fma(R_a2, z, fma(R_a1, y, R_a0 * x)) + T_a in fp32.  A product of two fp32 values is exact in fp64;
    each fma / add is that exact sum rounded once to fp32 (_sum32)."""
    P = np.asarray(se3, dtype=np.float32).astype(np.float64)
    x, y, z = (np.asarray(xyz[i], dtype=np.float32).astype(np.float64) for i in range(3))
    out = np.empty((3, x.shape[0]), np.float32)
    for a in range(3):
        t = (P[a, 0] * x).astype(np.float32).astype(np.float64)
        t = _sum32(P[a, 1] * y, t).astype(np.float64)
        t = _sum32(P[a, 2] * z, t).astype(np.float64)
        out[a] = _sum32(t, np.full_like(t, P[a, 3]))
    return out


def voxel_down_sample_ref(points: np.ndarray, vs: float):
    """open3d PointCloud::VoxelDownSample restated in fp64 (points (3,N) fp32, transformed): min_b = min - vs/2,
    index = floor((p - min_b) / vs), centroid = fp64 mean; voxels in order of first appearance.
    -> (centroids (3,M) fp64, counts (M,), index of each voxel's first point (M,), ref_coord (3,N) fp64)"""
    p = np.asarray(points, dtype=np.float32).astype(np.float64)
    if p.shape[1] == 0:
        return np.zeros((3, 0)), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((3, 0))
    min_b = p.min(axis=1) - vs / 2.0
    ref = (p - min_b[:, None]) / vs
    idx = np.floor(ref).astype(np.int64)
    key = idx[0] | (idx[1] << 21) | (idx[2] << 42)
    _, first, inv, counts = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    sums = np.stack([np.bincount(inv, weights=p[a], minlength=first.shape[0]) for a in range(3)])
    means = sums / counts[None, :]
    order = np.argsort(first, kind="stable")
    return means[:, order], counts[order], first[order], ref


def read_pcd(path: str) -> np.ndarray:
    """binary PCD v0.7 with x y z float32 -> (3,M) fp32"""
    with open(path, "rb") as f:
        head = {}
        while True:
            line = f.readline().decode("ascii").strip()
            if line.startswith("#"):
                continue
            k, v = line.split(" ", 1)
            head[k] = v
            if k == "DATA":
                break
        data = f.read()
    assert head["VERSION"] == "0.7" and head["FIELDS"] == "x y z" and head["SIZE"] == "4 4 4" and head["TYPE"] == "F F F"
    assert head["DATA"] == "binary" and head["WIDTH"] == head["POINTS"] and head["HEIGHT"] == "1"
    M = int(head["POINTS"])
    assert len(data) == 12 * M
    return np.frombuffer(data, dtype="<f4").reshape(M, 3).T.copy()


def test_pcd_writer_round_trip(tmp_path):
    from deeppointmap_amd.globalmap import write_pcd
    rng = np.random.default_rng(3)
    xyz = rng.normal(size=(3, 1001)).astype(np.float32) * 100
    xyz[:, 7] = [np.float32(1e-30), -0.0, np.float32(3.4e38)]
    write_pcd(str(tmp_path / "a.pcd"), xyz)
    back = read_pcd(str(tmp_path / "a.pcd"))
    assert back.dtype == np.float32 and np.array_equal(back.view(np.uint32), xyz.view(np.uint32))
    write_pcd(str(tmp_path / "empty.pcd"), np.zeros((3, 0), np.float32))
    assert read_pcd(str(tmp_path / "empty.pcd")).shape == (3, 0)
    with pytest.raises(ValueError):
        write_pcd(str(tmp_path / "bad.pcd"), np.zeros((4, 2), np.float32))


def test_restatement_hand_worked():
    """min = (0, 0, 0) -> min_b = -0.25: x = 0, 0.2 fall in voxel 0 ((x + 0.25) / 0.5 = 0.5, 0.9), x = 0.6 in voxel 1 (1.7),
    x = 0.24 in voxel 0 again (0.98); y = 1.0 is voxel 2 of y (2.5).  Order of first appearance: the first point's voxel,
    then x = 0.6, then (0, 1, 0)."""
    pts = np.array([[0.0, 0.2, 0.6, 0.0, 0.24],
                    [0.0, 0.0, 0.0, 1.0, 0.0],
                    [0.0, 0.0, 0.0, 0.0, 0.0]], dtype=np.float32)
    c, n, first, ref = voxel_down_sample_ref(pts, 0.5)
    assert n.tolist() == [3, 1, 1] and first.tolist() == [0, 2, 3]
    np.testing.assert_allclose(c[:, 0], [(float(np.float32(0.2)) + float(np.float32(0.24))) / 3, 0, 0], rtol=0, atol=1e-15)
    np.testing.assert_allclose(c[:, 1], [np.float32(0.6), 0, 0], rtol=0, atol=0)
    np.testing.assert_allclose(c[:, 2], [0, 1, 0], rtol=0, atol=0)
    np.testing.assert_allclose(ref[:, 0], [0.5, 0.5, 0.5])
    # the anchor is the minimum over ALL points: one point far below moves every boundary
    pts2 = np.concatenate([pts, np.array([[-0.3], [0.0], [0.0]], np.float32)], axis=1)
    c2, n2, first2, _ = voxel_down_sample_ref(pts2, 0.5)
    # min_b.x = -0.55: 0 -> 1.1, 0.2 -> 1.5, 0.6 -> 2.3, 0.24 -> 1.58, -0.3 -> 0.5
    assert n2.tolist() == [3, 1, 1, 1] and first2.tolist() == [0, 2, 3, 5]
    # empty input, one point
    assert voxel_down_sample_ref(np.zeros((3, 0), np.float32), 0.5)[0].shape == (3, 0)
    c1, n1, _, _ = voxel_down_sample_ref(np.array([[1.5], [2.5], [-3.5]], np.float32), 0.5)
    assert n1.tolist() == [1] and c1[:, 0].tolist() == [1.5, 2.5, -3.5]


def test_fp32_rounding_of_exact_sums():
    """the halfway cases a plain fp64 -> fp32 cast gets wrong: 1 + 2^-24 is halfway between 1 and 1 + 2^-23 (ties to even:
    1); with 2^-60 more, the exact sum is above halfway (1 + 2^-23), with 2^-60 less below (1)"""
    one, h, tiny = np.array([1.0]), np.array([2.0 ** -24]), 2.0 ** -60
    assert _sum32(one, h)[0] == np.float32(1.0)
    assert _sum32(one + h, np.array([tiny]))[0] == np.float32(1.0 + 2.0 ** -23)
    assert _sum32(one + h, np.array([-tiny]))[0] == np.float32(1.0)
    assert _sum32(-(one + h), np.array([-tiny]))[0] == np.float32(-(1.0 + 2.0 ** -23))
    rng = np.random.default_rng(4)
    a, b = rng.normal(size=10000) * 1e3, rng.normal(size=10000)
    assert np.array_equal(_sum32(a, b), (a + b).astype(np.float32))   # no halfway case: the plain cast


def test_transform_restatement_matches_torch_on_exact_cases():
    """identity and a pure translation are exact in any arithmetic; a 90-degree rotation permutes coordinates exactly"""
    rng = np.random.default_rng(1)
    xyz = rng.normal(size=(3, 100)).astype(np.float32)
    assert np.array_equal(transform_fp32(xyz, np.eye(4)), xyz)
    T = np.eye(4)
    T[:3, 3] = [0.5, -2.0, 8.0]
    assert np.array_equal(transform_fp32(xyz, T), (xyz + np.array([[0.5], [-2.0], [8.0]], np.float32)).astype(np.float32))
    Rz = np.array([[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
    assert np.array_equal(transform_fp32(xyz, Rz), np.stack([-xyz[1], xyz[0], xyz[2]]))


def test_result_maps_is_off_by_default():
    """no key: the back end retains no map clouds and records no ground truth, and the logger's map calls write nothing"""
    from deeppointmap_amd.consumer import Rank0Consumer, default_slam_args
    from deeppointmap_amd.system import ResultLogger
    assert "result_maps" not in default_slam_args()
    b = Rank0Consumer(None, "cpu")
    assert b.result_maps is False and b.map_clouds is None and b.gt == {}
    on = Rank0Consumer(None, "cpu", slam_args=dict(result_maps=True))
    assert on.result_maps is True and on.map_clouds is not None and len(on.map_clouds) == 0
    assert Rank0Consumer(None, "cpu", slam_args=dict(result_maps=False)).map_clouds is None
    import tempfile
    import os
    with tempfile.TemporaryDirectory() as d:
        rl = ResultLogger(b, d)
        rl.draw_trajectory("t", draft=False), rl.draw_trajectory("t", draft=True), rl.export_map("t"), rl.save_map("t")
        assert os.listdir(d) == []


def test_plot_data_layers_without_a_gpu(tmp_path):
    """draft plot_data needs no device: scans by timestep, ground truth, edges by insertion order; the renderer writes a jpg"""
    import torch
    from deeppointmap_amd.consumer import Rank0Consumer
    from deeppointmap_amd.system import ResultLogger
    b = Rank0Consumer(None, "cpu", slam_args=dict(result_maps=True))
    for i, (tok, kind) in enumerate([(0, "full"), (2, "non-keyframe"), (1, "full")]):
        b.type[tok] = kind
        b.poses[tok] = torch.eye(4)
        b.poses[tok][:3, 3] = torch.tensor([float(tok), 2.0 * tok, 0.0])
    b.gt[0] = torch.eye(4)
    b.edges[(0, 1)] = dict(type="odom")
    b.edges[(1, 2)] = dict(type="locz")
    b.edges[(0, 2)] = dict(type="other")
    rl = ResultLogger(b, str(tmp_path))
    d = rl.plot_data(draft=True)
    assert d["scan_token"].tolist() == [0, 1, 2] and d["scan_key"].tolist() == [True, True, False]
    assert d["scan_xy"].tolist() == [[0, 0], [1, 2], [2, 4]]
    assert d["gt_xy"][0].tolist() == [0, 0] and np.isnan(d["gt_xy"][1:]).all()
    assert d["edge_type"].tolist() == ["odom", "locz"] and d["edge_xy"][1].tolist() == [[1, 2], [2, 4]]
    assert d["full_map"] is None and d["key_map"] is None
    rl.draw_trajectory("t", draft=True)
    assert (tmp_path / "t.map.jpg").stat().st_size > 1000
