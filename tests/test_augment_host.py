"""CPU: tests/augment_restated.py and the draw source of deeppointmap_amd.augment against the reference's own outputs
(tests/golden/augment_*.npz, made by tests/golden/make_golden_augment.py from dataloader/transforms.py)."""
import json
import random

import numpy as np
import pytest
import torch

import augment_restated as A
from conftest import load_golden


@pytest.fixture(scope="module")
def gold():
    g = load_golden("augment_ref.npz")
    g.update(load_golden("augment_scan.npz"))
    return g


def _ground_params(g, name):
    L, W, gw, gh = g[name + ".params"]
    return int(L), int(W), float(gw), float(gh)


def test_ground_filter(gold):
    for name, key in (("ground", "scan"), ("ground_edge", "ground_edge.in")):
        L, W, gw, gh = _ground_params(gold, name)
        r = A.ground_filter(gold[key], L, W, gw, gh)
        A.check_ground(gold, name, gold[key], r["keep"])
        assert np.array_equal(np.sort(r["nonground"]), np.sort(gold[name + ".idx"][:int(gold[name + ".n_nonground"])]))
    # the edge set really holds its cases: the 2-point cell is gone, the threshold cell is sparse, the strip survives
    xyz = gold["ground_edge.in"]
    keep = set(A.ground_filter(xyz, 16, 16, 1.0, 0.5)["keep"].tolist())
    assert not {0, 1} & keep and len({2, 3, 4} & keep) == 1 and {5, 6, 7} <= keep and keep & {8, 9, 10} == {8} and {11, 12, 13} <= keep
    strip = [i for i in range(xyz.shape[0]) if -9.0 < xyz[i, 0] < -8.0 or -9.0 < xyz[i, 1] < -8.0]
    assert len(strip) == 12 and set(strip) <= keep
    outside = [i for i in range(xyz.shape[0]) if max(xyz[i, 0], xyz[i, 1]) >= 8.0 or min(xyz[i, 0], xyz[i, 1]) <= -9.0]
    assert len(outside) == 18 and not set(outside) & keep
    assert np.array_equal(A.ground_filter(xyz, 16, 16, 1.0, 0.0)["keep"], np.arange(xyz.shape[0]))


def test_voxel_sample(gold):
    for name, key in (("voxel", "scan"), ("voxel_one", "voxel_one.in"), ("voxel_each", "voxel_each.in")):
        for ret in ("first", "center"):
            assert np.array_equal(A.voxel_sample(gold[key], float(gold[name + ".voxel_size"]), ret), gold[f"{name}.{ret}"]), (name, ret)
    assert not np.array_equal(gold["voxel.first"], gold["voxel.center"])


def test_mask_selections(gold):
    scan = gold["scan"]
    assert np.array_equal(A.distance_sample(scan, *gold["distance.params"]), gold["distance.idx"])
    assert np.array_equal(A.random_drop(gold["drop.u"], float(gold["drop.ratio"])), gold["drop.idx"])
    w = gold["shield.wedges"]
    assert w.shape == (4, 4) and 0 < w[:, 2].sum() < 4                     # max_num wedges, one of them wraps past 180
    assert np.array_equal(A.random_shield(scan, w), gold["shield.idx"])
    assert A.shield_band(scan, w).mean() <= 1e-3


def test_wedges_from_the_recorded_draws(gold):
    """the library's wedge arithmetic on the reference's recorded torch.rand(3) draws gives the fixture's wedges"""
    from deeppointmap_amd.augment import shield_wedges

    class Src:
        vals = [torch.from_numpy(r) for r in gold["shield.rand3"]]
        def randint(self, a, b): return len(gold["shield.rand3"])
        def rand3(self): return self.vals.pop(0)
    assert np.array_equal(shield_wedges(Src(), [20.0, 90.0], [5.0, 25.0], 4), gold["shield.wedges"])


def test_index_transforms(gold):
    assert np.array_equal(A.gather(gold["shuffle.perm"], 4097), gold["shuffle.idx"])
    assert np.array_equal(A.gather(gold["sample.perm"], 4097, 1000), gold["sample.idx"])
    assert np.array_equal(A.gather(gold["sample.perm"], 4097, 5000), np.arange(4097))


def test_pointwise_maps(gold):
    small = gold["scan"][:4097]
    assert np.array_equal(A.random_pos_jitter(small, gold["jitter.j"]), gold["jitter.out"])
    assert np.array_equal(A.coordinates_normalization(small, 60.0), gold["norm.out"])
    for k in (0, 1):
        val, bound = A.affine(small, gold[f"rt{k}.R_aug"], gold[f"rt{k}.T_aug"])
        assert np.all(np.abs(gold[f"rt{k}.out"] - val) <= bound)
        R_new, T_new, calib = A.random_rt_pose(gold["rt.R_in"], gold["rt.T_in"], np.eye(4), gold[f"rt{k}.R_aug"], gold[f"rt{k}.T_aug"])
        assert np.array_equal(R_new, gold[f"rt{k}.R_new"]) and np.array_equal(T_new, gold[f"rt{k}.T_new"])
        assert np.array_equal(calib, gold[f"rt{k}.calib"])
    val, bound = A.vertical_correct(small, float(gold["vc.angle"]))
    assert np.all(np.abs(gold["vc.out"] - val) <= bound)
    assert float(np.abs(gold["vc.out"] - small).max()) > 0.1                # the correction moves points


def test_paired_rt_matrices_from_the_recorded_draws(gold):
    """RandomRT's host arithmetic (euler_matrix, the pair / flag / random_R state) on the recorded torch.rand(3) draws
    gives the reference's R_aug bit for bit"""
    from deeppointmap_amd import augment

    class Src(augment.DrawSource):
        reference, record = True, False
        vals = [torch.from_numpy(gold[f"rt{k}.rand3"]) for k in (0, 1)]
        def __init__(self): pass
        def random(self): return 0.0
        def rand3(self): return self.vals.pop(0)
        def normal31(self, mean, std): return torch.zeros(3, 1)
        def note(self, *a, **k): pass
    got = []
    rt = augment.RandomRT(r_std=0.5, t_std=1.0, p=1.0, pair=True)
    orig = augment.random_rt
    augment.random_rt = lambda pcd, R_aug, T_aug: got.append(R_aug.numpy())
    try:
        with augment.draws(Src()):
            rt(None), rt(None)
    finally:
        augment.random_rt = orig
    assert np.array_equal(got[0], gold["rt0.R_aug"]) and np.array_equal(got[1], gold["rt1.R_aug"])


def test_pack():
    a, b = np.arange(12, dtype=np.float32).reshape(4, 3), np.ones((2, 3), np.float32)
    pts, pad = A.pack([a, b], -1)
    assert pts.shape == (2, 3, 4) and np.array_equal(pts[0], a.T) and np.array_equal(pad, [[0, 0, 0, 0], [0, 0, 1, 1]])
    assert np.array_equal(pts[1, :, 2:], np.zeros((3, 2)))
    with pytest.raises(RuntimeError, match="greater than `padding_to`"):
        A.pack([a, b], 3)


class _Stub:
    """a frame without a GPU: the draw source only asks for its length, capacity and device"""
    cap, device, count = 4097, torch.device("cpu"), None

    def __init__(self, n):
        self.nbr_point = n


@pytest.mark.parametrize("name", ["train", "choice"])
def test_reference_draw_source_issues_the_reference_call_log(name, monkeypatch):
    """the class layer in rng='reference' mode, driven with the fixture's recorded point counts (no kernels: the functional
    layer is stubbed out), issues the fixture's call log exactly and the fixture's random.* values exactly.  Torch-drawn
    values are not compared: whether torch's CPU streams are identical between hosts is unverified."""
    from deeppointmap_amd import augment
    case = json.loads(str(load_golden("augment_chains.npz")["chains"]))[name]
    log, values = [], []

    def wrap(mod, fn, label, is_py):
        orig = getattr(mod, fn)

        def f(*a, **k):
            v = orig(*a, **k)
            log.append(label if is_py else f"{label}:" + "x".join(str(s) for s in v.shape))
            if is_py:
                values.append(float(a[0].index(v[0])) if fn == "choices" else float(v))
            return v
        monkeypatch.setattr(mod, fn, f)
    for fn in ("random", "uniform", "randint", "choices"):
        wrap(random, fn, "random." + fn, True)
    for fn in ("rand", "normal", "randperm"):
        wrap(torch, fn, "torch." + fn, False)
    monkeypatch.setattr(augment, "_apply", lambda fname, pcd, **kw: pcd)
    random.seed(case["seed"])
    torch.manual_seed(case["seed"])
    chain = augment.get_transforms(case["spec"])
    for counts in case["counts"]:
        stub = _Stub(counts[0])
        for t, n_after in zip(chain.transforms, counts[1:]):
            assert t(stub) is stub
            stub.nbr_point = n_after
    assert log == case["log"]
    assert values == case["py_values"]


def test_dataloader_import_path_resolves_to_the_gpu_transforms():
    import os
    import subprocess
    import sys
    from conftest import ROOT
    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(1, %r)\n"
        "from dataloader.transforms import PointCloud, PointCloudTransforms, get_transforms, pointcloud_transforms, RandomOcclusion\n"
        "import deeppointmap_amd.augment as a\n"
        "assert get_transforms is a.get_transforms and PointCloud is a.PointCloud and len(pointcloud_transforms) == 17\n"
        "chain = get_transforms({'VoxelSample': {'voxel_size': 0.3, 'retention': 'first'}, 'ToGPU': {}, 'RandomChoice': {'transforms': "
        "{'RandomShield': {'angle_range': [1, 2], 'dis_range': [1, 2], 'max_num': 2}, 'RandomDrop': {'max_ratio': 0.1}}, 'p': [1, 1]}, "
        "'ToTensor': {'padding_to': 8, 'use_calib': True}})\n"
        "assert [type(t).__name__ for t in chain.transforms] == ['VoxelSample', 'ToGPU', 'RandomChoice', 'ToTensor']\n"
        "assert isinstance(chain.transforms[2].transforms[0], RandomOcclusion)\n"
        "print('ok')\n") % (os.path.join(ROOT, "deeppointmap_amd", "dropin"), ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]


def test_class_layer_names_and_refusals():
    from deeppointmap_amd import augment
    assert len(augment.pointcloud_transforms) == 17 and augment.pointcloud_transforms["RandomShield"] is augment.RandomOcclusion
    with pytest.raises(NotImplementedError):
        augment.ToTensor(use_norm=True)
    with pytest.raises(NotImplementedError):
        augment.voxel_sample(None, 0.3, "center", num=100)
    with pytest.raises(TypeError):
        augment.RandomChoice([], p=0.5)
    with pytest.raises(ValueError):
        augment.DrawSource("numpy")
