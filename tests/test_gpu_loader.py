"""GPU: EpochLoader on the tree of tests/dataset_tree.py (2048-point scans).  The chain is the shipped inference chain of
tests/test_gpu_augment.py's drop-in test with RandomRT and RandomDrop in it, without its ToTensor."""
import os
import random
import shutil
import threading

import pytest
import torch
from torch.utils.data import BatchSampler, RandomSampler

import dataset_tree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POINTS, CAP, PAD = 2048, 2048 + 64, 2048
CHAIN = {"VoxelSample": {"voxel_size": 0.3, "retention": "first"}, "ToGPU": {}, "DistanceSample": {"min_dis": 1.0, "max_dis": 60.0},
         "RandomRT": {}, "RandomDrop": {"max_ratio": 0.2}, "CoordinatesNormalization": {"ratio": 60.0}, "ToCPU": {}}


def chain():
    from deeppointmap_amd import augment
    return augment.get_transforms(CHAIN)       # a fresh one per run: RandomRT carries the state of its pairing


def open_tree(root):
    from deeppointmap_amd import dataset
    from deeppointmap_amd.config import Cfg
    return dataset.SlamDatasets(Cfg(dataset_tree.tree_config(root)))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("tree2048"))
    dataset_tree.write_tree(root, POINTS)
    return root, open_tree(root)


def loader(ds, stage, batch_size, rng, prefetch, **kw):
    from deeppointmap_amd.loader import EpochLoader
    return EpochLoader(ds, chain(), stage, batch_size, rng=rng, prefetch=prefetch, capacity=CAP, padding_to=PAD, device=DEV, **kw)


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, torch.Tensor):
            assert x.is_cuda and x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)
        else:
            assert x == y
    return True


def loader_threads():
    return [t for t in threading.enumerate() if t.name == "deeppointmap-loader"]


@pytest.mark.parametrize("stage,batch_size", [("registration", 4), ("loop_detection", 4)])
def test_reference_mode_equals_the_hand_written_loop(tree, stage, batch_size):
    from deeppointmap_amd import augment
    root, ds = tree
    random.seed(5), torch.manual_seed(5)
    with loader(ds, stage, batch_size, "reference", 0) as ld:
        assert len(ld) == len(ds) // batch_size
        got = list(ld)
    assert len(got) == len(ds) // batch_size
    # the parent's pieces, by hand, with the same seeding: plan -> reader -> transform_frames -> collate_frames
    random.seed(5), torch.manual_seed(5)
    torch.empty((), dtype=torch.int64).random_()            # DataLoader.__iter__'s base seed
    batches = [list(b) for b in BatchSampler(RandomSampler(range(len(ds))), batch_size, drop_last=True)]
    reader, tf = ds.dataset_list[0].scene_list[0].agent_list[0].reader, chain()
    getattr(ds, stage)()
    for k, indices in enumerate(batches):
        if stage == "registration":
            plan = ds.plan_registration(indices[0])
            files = [f[3] for f in plan["frames"]]
        else:
            files = [f for i in indices for f in ds.plan_loop_detection(i)["files"]]
        frames = augment.transform_frames([reader(f) for f in files], tf, rng="reference")
        pcd, R, T, pad, calib = augment.collate_frames(frames, PAD)
        if stage == "registration":
            assert len(got[k]) == 6 and got[k][5] == plan["info"]
            same(got[k][:5], (pcd, R, T, pad, calib))
            assert pcd.shape == (plan["S"] * plan["num_map"], 3, PAD)
        else:
            assert len(got[k]) == 10
            same(got[k], tuple(t[h::2] for h in (0, 1) for t in (pcd, R, T, pad, calib)))
            assert got[k][0].shape == (batch_size, 3, PAD) and all(t.is_contiguous() for t in got[k])
        assert 0 < int((~pad).sum(1).min()) <= POINTS


def test_reference_mode_refuses_prefetch(tree):
    with pytest.raises(ValueError):
        loader(tree[1], "registration", 4, "reference", 1)
    with pytest.raises(ValueError):
        loader(tree[1], "registration", 4, "other", 0)


@pytest.mark.parametrize("stage,batch_size", [("registration", 6), ("loop_detection", 6)])
def test_seeded_batches_do_not_depend_on_prefetch(tree, stage, batch_size):
    root, ds = tree
    random.seed(1), torch.manual_seed(1)
    state = random.getstate(), torch.get_rng_state()

    def epoch(prefetch, ep=1, **kw):
        with loader(ds, stage, batch_size, 7, prefetch, **kw) as ld:
            ld.set_epoch(ep)
            out = list(ld)
        assert not loader_threads()
        return out
    base = epoch(0)
    assert len(base) == len(ds) // batch_size
    if stage == "registration":
        assert all(len(b) == 7 and isinstance(b[6], int) and 1 <= b[6] < b[0].shape[0] // b[5]["num_map"] for b in base)
    for prefetch, kw in ((1, {}), (2, {}), (2, {"num_workers": 3}), (0, {})):          # and again on a second run
        again = epoch(prefetch, **kw)
        assert len(again) == len(base) and all(same(a, b) for a, b in zip(base, again)), prefetch
    # no global random state was consumed
    assert random.getstate() == state[0] and torch.equal(torch.get_rng_state(), state[1])
    # another epoch: another index order and other draws
    other = epoch(2, ep=2)
    if stage == "registration":
        first = lambda bs: [b[5]["dsf_index"][0] for b in bs]    # noqa: E731
        assert first(other) != first(base) and sorted(set(first(base))) == sorted(first(base))
    assert not all(torch.equal(a[0], b[0]) for a, b in zip(base, other))


def test_missing_file_raises_from_next_and_the_thread_ends(tmp_path):
    root = str(tmp_path / "tree")
    dataset_tree.write_tree(root, 256)
    ds = open_tree(root)
    os.remove(os.path.join(root, "KITTI", "01", "0", "1.npz"))
    ld = loader(ds, "registration", 1, 3, 2)        # batch_size 1: every frame heads a batch of the epoch
    it = iter(ld)
    thread = ld._thread
    with pytest.raises(FileNotFoundError):
        for _ in range(len(ld)):
            next(it)
    thread.join(30)
    assert not thread.is_alive() and not loader_threads()
    ld.close()
    shutil.rmtree(root)
    dataset_tree.write_tree(root, 256)
    with loader(open_tree(root), "registration", 1, 3, 2) as fresh:      # a fresh loader then works
        assert len(list(fresh)) == 48
    assert not loader_threads()


def test_break_and_close_leave_no_thread(tree):
    root, ds = tree
    ld = loader(ds, "loop_detection", 4, 9, 2)
    for k, batch in enumerate(ld):
        if k == 1:
            break
    assert loader_threads()
    ld.close()
    assert not loader_threads()
    with pytest.raises(RuntimeError):
        next(ld)
    # a frame with more records than the capacity is refused before anything is queued
    from deeppointmap_amd.loader import EpochLoader
    with EpochLoader(ds, chain(), "registration", 4, rng=1, prefetch=1, capacity=POINTS - 1, padding_to=PAD, device=DEV) as small:
        with pytest.raises(ValueError, match="capacity"):
            next(iter(small))
    assert not loader_threads()
