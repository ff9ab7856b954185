"""CPU: the dataset tree, the readers, the frame distances, the loader's index order and the per-thread draws() stack against
fixtures made by running the reference (tests/golden/make_golden_dataset.py) on the tree of tests/dataset_tree.py."""
import json
import os
import random
import shutil
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import dataset_tree
from conftest import GOLDEN, ROOT, load_golden

SCENES = {"KITTI_00": ("KITTI", "00"), "KITTI_01": ("KITTI", "01"), "Carla_Town_00": ("Carla_Town", "00")}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from deeppointmap_amd import dataset
    from deeppointmap_amd.config import Cfg
    root = str(tmp_path_factory.mktemp("tree"))
    files = dataset_tree.write_tree(root)
    ds = dataset.SlamDatasets(Cfg(dataset_tree.tree_config(root)))
    return root, files, ds


@pytest.fixture(scope="module")
def draws():
    with open(os.path.join(GOLDEN, "dataset_draws.json")) as f:
        return json.load(f)


def test_tree_shape_and_str(tree):
    root, files, ds = tree
    assert len(ds) == dataset_tree.N_FRAMES == len(files)
    assert ds.pcd_range.tolist() == [0, 43, 48]
    assert ds.dataset_list[0].pcd_range.tolist() == [0, 40, 43]
    assert ds.dataset_list[0].scene_list[0].pcd_range.tolist() == [0, 25, 40]
    assert ds.get_seq_range().tolist() == [0, 25, 40, 43, 48]
    assert ds.dataset_list[0].get_frame_order(41) == (1, 1)
    for gid in (0, 24, 25, 39, 40, 42, 43, 47):     # files sorted by the integer in the name, agents in order
        d = 0 if gid < 43 else 1
        assert ds.dataset_list[d].file_of(gid - int(ds.pcd_range[d])) == files[gid]
    text = str(ds)
    assert "SlamDatasets: num_datasets=2" in text and "|——kitti" in text and "num_scenes=2 | num_frames=43" in text
    assert ds.collate_fn == ds.map_collate_fn
    ds.loop_detection()
    assert ds.collate_fn is None
    ds.registration()


def test_agent_split_and_independent(tree):
    from deeppointmap_amd import dataset
    root, files, _ = tree
    agent_root = os.path.join(root, "KITTI", "00", "0")     # 25 files
    whole = dataset.BasicAgent(agent_root, reader="auto")
    assert isinstance(whole.reader, dataset.NPZReader) and whole.file_list == files[:25]
    parts = [dataset.BasicAgent(agent_root, reader="auto", split_num=3, split_index=k) for k in range(3)]
    # body.py:340-346: a third each, 5 % overlap on both sides, the bounds truncated
    bounds = [(int(25 * max(1 / 3 * k - 1 / 20, 0.0)), int(25 * min(1 / 3 * (k + 1) + 1 / 20, 1.0))) for k in range(3)]
    assert bounds == [(0, 9), (7, 17), (15, 25)]
    assert [p.file_list for p in parts] == [files[a:b] for a, b in bounds]
    seen = []
    whole.reader = lambda path: path
    whole.set_independent(lambda data: seen.append(data) or "transformed")
    assert whole[3] == "transformed" and seen == [files[3]]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_registration_plans_equal_the_reference_draws(tree, draws, seed):
    root, files, ds = tree
    gid = {f: k for k, f in enumerate(files)}
    want = draws["registration"][str(seed)]
    if seed == 1:
        random.seed(seed)      # the default rng is Python's global `random`, as in the reference
        rng = {}
    else:
        rng = {"rng": random.Random(seed)}
    ds.registration()
    for index in range(draws["n"]):
        plan = ds.plan_registration(index, **rng)
        w = want[index]
        assert (plan["S"], plan["num_map"]) == (w["S"], w["num_map"]), index
        assert [gid[f[3]] for f in plan["frames"]] == w["frames"], index
        assert [list(f[:3]) for f in plan["frames"]] == w["dsf_index"], index
        info = plan["info"]
        assert [list(t) for t in info["dsf_index"]] == w["dsf_index"] and info["num_map"] == w["num_map"]
        assert [os.path.relpath(p, root) if p else "" for p in info["refined_SE3_file"]] == w["refined_SE3_file"], index
    branches = {len(set(w["frames"][:w["S"]])) < w["S"] for w in want}      # a replicated map and a plain one were drawn
    assert branches == {True, False}


def test_getitem_executes_the_plan_it_draws(tree, draws):
    """__getitem__ (the reference's interleaved form) with a transform that returns the frame id"""
    from deeppointmap_amd import dataset
    from deeppointmap_amd.config import Cfg
    root, files, _ = tree
    ds = dataset.SlamDatasets(Cfg(dataset_tree.tree_config(root)), data_transforms=lambda frame: (frame,))
    for d in ds.dataset_list:
        for s in d.scene_list:
            for a in s.agent_list:
                a.reader = lambda path, _g={f: k for k, f in enumerate(files)}: _g[path]
    random.seed(2)
    want = draws["registration"]["2"]
    for index in range(draws["n"]):
        frames, info = ds[index]
        assert [f[0] for f in frames] == want[index]["frames"] and info["num_map"] == want[index]["num_map"]
    ds.loop_detection()
    random.seed(3)
    assert [list(ds[i]) for i in range(draws["n"])] == draws["loop_detection"]["3"]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_loop_detection_plans_equal_the_reference_draws(tree, draws, seed):
    root, files, ds = tree
    gid = {f: k for k, f in enumerate(files)}
    rng = random.Random(seed)
    got = [[gid[f] for f in ds.plan_loop_detection(i, rng=rng)["files"]] for i in range(draws["n"])]
    assert got == draws["loop_detection"][str(seed)]
    assert got[47][1] in (43, 44, 45, 46, 47)       # a pair never leaves its scene


def test_frame_dis_bits_cache_and_chunks(tree, tmp_path):
    from deeppointmap_amd import dataset
    from deeppointmap_amd.config import Cfg
    root, files, ds = tree
    ref = load_golden("dataset_ref.npz")
    for name, scene in SCENES.items():
        want = ref["frame_dis_" + name]
        saved = np.load(os.path.join(root, *scene, "frame_dis.npy"))
        assert saved.dtype == np.float32 and saved.tobytes() == want.tobytes(), name
    d, s = ds.frame_distance[0][0], torch.from_numpy(ref["frame_dis_KITTI_00"]).half()
    assert d.dtype == torch.float16 and torch.equal(d, s)
    # the chunked build is the one-shot build bit for bit
    poses = np.stack([np.asarray(p[4], np.float32) for p in dataset_tree.poses()[:40]])
    for chunk in (1, 7, 40):
        assert dataset.pairwise_frame_dis(poses, chunk).tobytes() == ref["frame_dis_KITTI_00"].tobytes(), chunk
    # a cache that fits is used as it is; one of another frame count is rebuilt
    copy = str(tmp_path / "tree")
    shutil.copytree(root, copy)
    cache = os.path.join(copy, "KITTI", "00", "frame_dis.npy")
    marked = ref["frame_dis_KITTI_00"].copy()
    marked[0, 20] = 1.0
    np.save(cache, marked)
    np.save(os.path.join(copy, "KITTI", "01", "frame_dis.npy"), np.zeros((5, 5), np.float32))
    ds2 = dataset.SlamDatasets(Cfg(dataset_tree.tree_config(copy)))
    assert float(ds2.frame_distance[0][0][0, 20]) == 1.0
    assert np.load(os.path.join(copy, "KITTI", "01", "frame_dis.npy")).tobytes() == ref["frame_dis_KITTI_01"].tobytes()
    assert torch.equal(ds2.frame_distance[0][1], torch.from_numpy(ref["frame_dis_KITTI_01"]).half())


def test_read_raw_against_the_reference_readers(tmp_path):
    from deeppointmap_amd import dataset
    ref = load_golden("dataset_ref.npz")
    files = dataset_tree.write_reader_files(str(tmp_path))
    for kind, reader, stride, drop in (("npz", dataset.NPZReader(), 3, False), ("npy", dataset.NPYReader(), 3, False),
                                       ("bin", dataset.BinReader(), 4, True)):
        rows, got_stride, R, T, drop_nan = reader.read_raw(files[kind])
        assert rows.dtype == np.float32 and rows.shape[1] == got_stride == stride and drop_nan is drop
        xyz = dataset.filter_rows(rows, drop_nan)[:, :3]
        assert xyz.tobytes() == ref[kind + "_xyz"].tobytes(), kind
        if kind == "npz":
            assert np.array_equal(np.asarray(R, np.float32), ref["npz_R"]) and np.array_equal(np.asarray(T, np.float32), ref["npz_T"])
        else:
            assert R is None and T is None
            assert np.array_equal(ref[kind + "_R"], np.eye(3)) and not ref[kind + "_T"].any()
    rows = dataset.BinReader().read_raw(files["bin"])[0]
    assert rows.shape == (12, 4) and np.isnan(rows[9, 3]) and ref["bin_xyz"].shape == (9, 3)   # the NaN intensity row stays
    # the suffix reader's .bin branch drops nothing (heads/auto.py), and a wrong suffix is refused
    assert dataset.PointCloudReader().read_raw(files["bin"])[4] is False
    with pytest.raises(AssertionError):
        dataset.NPZReader().read_raw(files["npy"])
    for key in ("lidar_norm", "lidar_seg", "image", "lidar_proj"):
        path = str(tmp_path / f"extra_{key}.npz")
        np.savez(path, lidar_pcd=np.zeros((4, 3), np.float32), **{key: np.zeros((4, 3), np.float32)})
        with pytest.raises(NotImplementedError):
            dataset.NPZReader().read_raw(path)
    assert set(dataset.READER) == {"auto", "npz", "npy", "bin", "pcd"}


def _write_pcd(path, xyz, kind, size):
    n = len(xyz)
    t = {4: "<f4", 8: "<f8"}[size]
    head = (f"# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS intensity x y z\nSIZE 4 {size} {size} {size}\n"
            f"TYPE F F F F\nCOUNT 1 1 1 1\nWIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA {kind}\n")
    with open(path, "wb") as f:
        f.write(head.encode())
        if kind == "ascii":
            for k, p in enumerate(xyz.astype(t)):
                f.write((f"{k * 0.5} " + " ".join("nan" if np.isnan(v) else repr(float(v)) for v in p) + "\n").encode())
        else:
            rec = np.zeros(n, dtype=[("i", "<f4"), ("x", t), ("y", t), ("z", t)])
            rec["i"] = np.arange(n) * 0.5
            rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
            f.write(rec.tobytes())


@pytest.mark.parametrize("kind,size", [("ascii", 4), ("ascii", 8), ("binary", 4), ("binary", 8)])
def test_pcd_parser_round_trip(tmp_path, kind, size):
    from deeppointmap_amd import dataset
    xyz = dataset_tree.scan(9, 20).astype(np.float64) + 0.125
    xyz[3, 1] = np.nan
    xyz[11, 2] = np.nan
    path = str(tmp_path / "0.pcd")
    _write_pcd(path, xyz, kind, size)
    rows, stride, R, T, drop_nan = dataset.PcdReader().read_raw(path)
    assert rows.dtype == np.float32 and stride == 3 and R is None and T is None and drop_nan is True
    assert np.array_equal(rows, xyz.astype(np.float32), equal_nan=True)
    kept = dataset.filter_rows(rows, drop_nan)
    assert kept.shape == (18, 3) and np.array_equal(kept, np.delete(xyz, [3, 11], axis=0).astype(np.float32))


def test_pcd_binary_compressed_is_refused(tmp_path):
    from deeppointmap_amd import dataset
    path = str(tmp_path / "0.pcd")
    with open(path, "wb") as f:
        f.write(b"VERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\nWIDTH 1\nHEIGHT 1\nPOINTS 1\nDATA binary_compressed\n\0\0\0\0")
    with pytest.raises(NotImplementedError):
        dataset.PcdReader().read_raw(path)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_loader_index_order_is_torchs_samplers(world):
    from torch.utils.data import BatchSampler
    from torch.utils.data.distributed import DistributedSampler
    from deeppointmap_amd import loader
    n, bs, seed = 47, 4, 11          # 47 frames over 2 or 3 ranks: the tail is padded with the first indices
    orders = {}
    for epoch in (1, 2):
        for rank in range(world):
            got = loader.epoch_indices(n, bs, epoch, seed=seed, rank=rank, world=world)
            sampler = DistributedSampler(range(n), num_replicas=world, rank=rank, seed=loader.sampler_seed(seed))
            sampler.set_epoch(epoch)
            assert got == [list(b) for b in BatchSampler(sampler, bs, drop_last=True)]
            assert len(got) == -(-n // world) // bs
            orders[epoch, rank] = got
        if world > 1:
            flat = sorted(i for r in range(world) for i in list(DistributedSampler(range(n), num_replicas=world, rank=r,
                                                                               seed=loader.sampler_seed(seed)).__iter__()))
            assert len(flat) == world * -(-n // world) and set(flat) == set(range(n))
    assert orders[1, 0] != orders[2, 0]                       # set_epoch changes the order
    assert loader.epoch_indices(n, bs, 1, seed=seed, rank=0, world=world) == orders[1, 0]
    assert loader.epoch_indices(48, 4, 1, seed=seed) and len(loader.epoch_indices(48, 4, 1, seed=seed)) == 48 // 4
    # the reference mode at world > 1 is the reference's DistributedSampler(dataset) after set_epoch
    if world > 1:
        sampler = DistributedSampler(range(n), num_replicas=world, rank=1)
        sampler.set_epoch(5)
        assert loader.epoch_indices(n, bs, 5, seed=None, rank=1, world=world) == [list(b) for b in BatchSampler(sampler, bs, drop_last=True)]
    else:
        torch.manual_seed(3)
        a = loader.epoch_indices(n, bs, 1, seed=None)
        torch.manual_seed(3)
        assert a == [list(b) for b in BatchSampler(torch.utils.data.RandomSampler(range(n)), bs, drop_last=True)]


def test_draws_stack_is_per_thread():
    from deeppointmap_amd import augment
    mine, theirs = augment.DrawSource("reference"), augment.DrawSource("reference")
    seen = {}
    entered, leave = threading.Event(), threading.Event()

    def other():
        seen["before"] = augment._source()
        with augment.draws(theirs):
            seen["inside"] = augment._source()
            entered.set()
            assert leave.wait(30)
        seen["after"] = augment._source()

    with augment.draws(mine):
        t = threading.Thread(target=other)
        t.start()
        assert entered.wait(30)
        assert augment._source() is mine          # the source pushed in the second thread is invisible here
        leave.set()
        t.join(30)
        assert not t.is_alive()
        assert augment._source() is mine
    assert seen["inside"] is theirs and seen["before"] is augment._DEFAULT and seen["after"] is augment._DEFAULT
    assert augment._source() is augment._DEFAULT


def test_dropin_import_paths_resolve_to_the_dataset_and_trainer():
    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(1, %r)\n"
        "from dataloader.body import SlamDatasets, BasicDataset, BasicScene, BasicAgent, get_frame_dis, READER\n"
        "from dataloader.heads.auto import PointCloudReader\n"
        "from dataloader.heads.npz import NPZReader\n"
        "from dataloader.heads.npy import NPYReader\n"
        "from dataloader.heads.bin import BinReader\n"
        "from dataloader.heads.pcd import PcdReader\n"
        "from pipeline.modules.trainer import Trainer\n"
        "import deeppointmap_amd.dataset as d, deeppointmap_amd.trainer as t\n"
        "assert SlamDatasets is d.SlamDatasets and BasicAgent is d.BasicAgent and get_frame_dis is d.get_frame_dis\n"
        "assert READER == {'auto': PointCloudReader, 'npz': NPZReader, 'npy': NPYReader, 'bin': BinReader, 'pcd': PcdReader}\n"
        "assert Trainer is t.Trainer and callable(Trainer.add_module) and callable(Trainer.remove_module)\n"
        "print('ok')\n") % (os.path.join(ROOT, "deeppointmap_amd", "dropin"), ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
