"""GPU: SceneLoader, the DataLoader of pipeline/infer.py (reference infer.py:85-98), on one agent directory of the tree of
tests/dataset_tree.py (KITTI/00/0: 25 npz frames of 2048 points) and on six .bin frames with a NaN record each.  The
yardstick is the synchronous per-frame path: agent.set_independent(PointCloudTransforms(Args, mode='infer'))[i]."""
import importlib.util
import os
import threading

import numpy as np
import pytest
import torch

import dataset_tree
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POINTS = 2048


class Args:
    transforms = {"VoxelSample": {"voxel_size": 0.3, "retention": "first"}, "ToGPU": {},
                  "DistanceSample": {"min_dis": 1.0, "max_dis": 60.0},
                  "OutlierFilter": {"nb_neighbors": 10, "std_ratio": 3.0},
                  "LowPassFilter": {"normals_radius": 0.5, "normals_num": 16, "filter_std": 2.0, "flux": 4, "max_remain": -1},
                  "CoordinatesNormalization": {"ratio": 60.0}, "ToCPU": {}, "ToTensor": {"padding_to": -1}}


class ArgsPadded:
    transforms = {**Args.transforms, "ToTensor": {"padding_to": 8192}}


class ArgsLattice:
    """for the tree's lattice scans: without LowPassFilter, which empties them (every normal of a 0.5 m lattice at radius
    0.5 is the (0,0,1) of a lone point, so every similarity equals the mean and none is above it)"""
    transforms = {k: v for k, v in Args.transforms.items() if k != "LowPassFilter"}


def raw_scan(n, seed):
    spec = importlib.util.spec_from_file_location("_raw_scan", os.path.join(GOLDEN, "raw_scan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.raw_scan(n=n, seed=seed)


def agent_of(root):
    from deeppointmap_amd.dataset import BasicAgent
    return BasicAgent(root, "auto")


def transform(args=Args):
    from deeppointmap_amd.augment import PointCloudTransforms
    return PointCloudTransforms(args, mode="infer")


def reference_items(root, args=Args):
    """what DataLoader(agent.set_independent(transforms), batch_size=1, shuffle=False) hands the reference's loop"""
    agent = agent_of(root)
    agent.set_independent(transform(args))
    return [[t.unsqueeze(0) for t in agent[i]] for i in range(len(agent))]


def same_item(got, want):
    assert len(got) == len(want) == 5
    for a, b in zip(got, want):
        assert a.is_cuda and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b.to(a.device))


def loader_threads():
    return [t for t in threading.enumerate() if t.name == "deeppointmap-loader"]


@pytest.fixture(scope="module")
def npz_scene(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("scene_tree"))
    dataset_tree.write_tree(root, POINTS)
    d = os.path.join(root, "KITTI", "00", "0")
    return d, reference_items(d, ArgsLattice)


def write_bin_scene(d, n=6):
    os.makedirs(d, exist_ok=True)
    for k in range(n):
        rec = torch.cat([raw_scan(6000, 40 + k), torch.ones(6000, 1)], dim=1).numpy().astype(np.float32)
        rec[100 + 7 * k, k % 3] = np.nan                    # one NaN record: BinReader drops it
        rec.tofile(os.path.join(d, f"{k}.bin"))
    return d


@pytest.fixture(scope="module")
def bin_scene(tmp_path_factory):
    d = write_bin_scene(str(tmp_path_factory.mktemp("scene_bin")))
    return d, reference_items(d)


@pytest.mark.parametrize("group,prefetch", [(1, 0), (1, 2), (4, 0), (4, 2)])
def test_items_equal_the_per_frame_path(npz_scene, bin_scene, group, prefetch):
    from deeppointmap_amd import augment
    from deeppointmap_amd.loader import SceneLoader
    res = {}
    for name, (d, want), frames, args in (("npz", npz_scene, 25, ArgsLattice), ("bin", bin_scene, 6, Args)):
        agent = agent_of(d)
        before = augment.host_syncs()
        with SceneLoader(agent, transform(args), group=group, prefetch=prefetch, device=DEV) as ld:
            assert len(ld) == len(agent) == frames
            got = res[name] = list(ld)
        assert augment.host_syncs() - before == -(-frames // group)      # one synchronisation per group, the short last one too
        assert len(got) == frames and not loader_threads()
        for g, w in zip(got, want):                                     # file order
            same_item(g, w)
            assert g[0].shape[:2] == (1, 3) and g[0].shape[2] > 0 and g[3].shape == (1, g[0].shape[2]) and not bool(g[3].any())
    # the reader's pose, and the frame as read
    files = agent_of(npz_scene[0]).file_list
    assert [os.path.basename(f) for f in files[:3]] == ["0.npz", "1.npz", "2.npz"]
    for i in (0, 7, 24):
        with np.load(files[i]) as z:
            assert torch.equal(res["npz"][i][1][0].cpu(), torch.from_numpy(z["ego_rotation"]).float())
            assert torch.equal(res["npz"][i][2][0].cpu(), torch.from_numpy(z["ego_translation"]).float())
            assert torch.equal(res["npz"][i][4][0].cpu(), torch.from_numpy(z["lidar_pcd"]).float())
    rec = np.fromfile(os.path.join(bin_scene[0], "3.bin"), dtype=np.float32).reshape(-1, 4)
    keep = ~np.isnan(rec[:, :3]).any(1)
    assert keep.sum() == 5999 and torch.equal(res["bin"][3][4][0].cpu(), torch.from_numpy(rec[keep, :3].copy()))


def test_frames_the_chain_empties(npz_scene):
    """the whole shipped chain empties the tree's lattice scans (ArgsLattice says why): items of no points, as the per-frame
    path gives them"""
    from deeppointmap_amd.loader import SceneLoader
    d, _ = npz_scene
    want = reference_items(d)[:6]
    with SceneLoader(agent_of(d), transform(), group=4, prefetch=2, device=DEV) as ld:
        it = iter(ld)
        got = [next(it) for _ in range(6)]
    for g, w in zip(got, want):
        same_item(g, w)
        assert g[0].shape == (1, 3, 0) and g[3].shape == (1, 0) and g[4].shape == (1, POINTS, 3)


def test_padding_to_and_a_compose(bin_scene):
    """ToTensor(padding_to=8192): every item is padded to it; a Compose is taken like a PointCloudTransforms"""
    from deeppointmap_amd import augment
    from deeppointmap_amd.loader import SceneLoader
    d, _ = bin_scene
    want = reference_items(d, ArgsPadded)
    with SceneLoader(agent_of(d), augment.get_transforms(ArgsPadded.transforms), group=4, prefetch=2, device=DEV) as ld:
        got = list(ld)
    assert len(got) == 6
    for g, w in zip(got, want):
        same_item(g, w)
        assert g[0].shape == (1, 3, 8192) and bool(g[3].any()) and not bool(g[3].all())


def test_failures_raise_and_never_hang(tmp_path, npz_scene):
    from deeppointmap_amd.loader import SceneLoader
    d = write_bin_scene(str(tmp_path / "bad"))
    path = os.path.join(d, "3.bin")
    with open(path, "r+b") as f:
        f.truncate(os.path.getsize(path) - 6)              # no longer whole records
    ld = SceneLoader(agent_of(d), transform(), group=2, prefetch=2, device=DEV, timeout=60.0)
    it = iter(ld)
    seen = 0
    with pytest.raises(RuntimeError, match="3.bin"):
        for _ in range(6):
            next(it)
            seen += 1
    assert seen == 2                                        # the group before the broken one was delivered
    ld.close()
    assert not loader_threads()
    # a fixed capacity smaller than a frame: refused, naming the file, before any launch
    d, want = npz_scene
    for prefetch in (0, 2):
        with SceneLoader(agent_of(d), transform(ArgsLattice), group=4, prefetch=prefetch, capacity=1000, device=DEV) as small:
            with pytest.raises(ValueError, match=r"0\.npz.*capacity"):
                next(iter(small))
    assert not loader_threads()
    # exhausted: StopIteration, again and again; then a second pass gives the same frames
    with SceneLoader(agent_of(d), transform(ArgsLattice), group=8, prefetch=2, capacity=POINTS, device=DEV) as ld:
        first = list(ld)
        with pytest.raises(StopIteration):
            next(ld)
        with pytest.raises(StopIteration):
            next(ld)
        second = list(ld)
    assert len(first) == len(second) == 25
    for a, b, w in zip(first, second, want):
        same_item(a, w), same_item(b, w)


def test_a_slam_system_fed_by_the_loader(bin_scene, cfg_full, tmp_path):
    """six frames into a SlamSystem, once from the loader and once from the per-frame path: equal exit codes and an equal
    saved trajectory"""
    from deeppointmap_amd.loader import SceneLoader
    from test_gpu_system import _system
    d, want = bin_scene

    def run(items, name):
        out = tmp_path / name
        out.mkdir()
        system = _system(cfg_full, logger_dir=str(out))
        codes = [system.step(list(item)) for item in items]
        system.result_logger.save_trajectory("trajectory")
        toks, poses = system.trajectory()
        return codes, toks, poses, open(out / "trajectory.allframes.txt").read()
    with SceneLoader(agent_of(d), transform(), group=4, prefetch=2, device=DEV) as ld:
        a = run(ld, "loader")
    b = run(want, "per_frame")
    assert len(a[0]) == 6 and a[0] == b[0] and a[1] == b[1] and torch.equal(a[2], b[2]) and a[3] == b[3]
