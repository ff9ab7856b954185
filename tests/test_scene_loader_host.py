"""CPU: the grouping plan and the constructor checks of loader.SceneLoader.  No device is touched."""
import os

import numpy as np
import pytest


def _agent(tmp_path, n):
    from deeppointmap_amd.dataset import BasicAgent
    for k in (list(range(n))[::-1]):                      # written in reverse: the order is the file NUMBER, not the directory's
        np.save(os.path.join(tmp_path, f"{k}.npy"), np.zeros((4, 3), np.float32))
    return BasicAgent(str(tmp_path), "auto")


def _chain(padding_to=-1, **extra):
    from deeppointmap_amd import augment
    spec = {"VoxelSample": {"voxel_size": 0.3, "retention": "first"}, "ToGPU": {},
            "DistanceSample": {"min_dis": 1.0, "max_dis": 60.0}, "CoordinatesNormalization": {"ratio": 60.0}, "ToCPU": {},
            "ToTensor": {"padding_to": padding_to, **extra}}
    return augment.get_transforms(spec)


def test_groups_are_consecutive_and_the_last_may_be_short():
    from deeppointmap_amd.loader import scene_groups
    assert scene_groups(25, 4) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15], [16, 17, 18, 19],
                                   [20, 21, 22, 23], [24]]
    assert scene_groups(6, 1) == [[k] for k in range(6)]
    assert scene_groups(6, 6) == [list(range(6))] and scene_groups(6, 100) == [list(range(6))]
    assert scene_groups(0, 4) == []
    for n in range(0, 40):
        for g in (1, 2, 3, 7, 16):
            flat = [i for grp in scene_groups(n, g) for i in grp]
            assert flat == list(range(n)) and all(1 <= len(grp) <= g for grp in scene_groups(n, g))
            assert len(scene_groups(n, g)) == -(-n // g)
    with pytest.raises(ValueError):
        scene_groups(5, 0)


def test_the_plan_follows_the_agent_s_file_list(tmp_path, monkeypatch):
    import torch
    from deeppointmap_amd.loader import SceneLoader
    monkeypatch.setattr(torch.cuda, "current_device", lambda: pytest.fail("the constructor touched the device"))
    agent = _agent(tmp_path, 11)
    assert [os.path.basename(f) for f in agent.file_list] == [f"{k}.npy" for k in range(11)]
    ld = SceneLoader(agent, _chain(), group=4, prefetch=2)
    assert len(ld) == len(agent) == 11 and ld.files == agent.file_list
    assert [[ld.files[i] for i in grp] for grp in ld.groups] == [agent.file_list[0:4], agent.file_list[4:8], agent.file_list[8:11]]
    assert ld.padding_to == -1 and [type(t).__name__ for t in ld.chain.transforms] == [
        "VoxelSample", "ToGPU", "DistanceSample", "CoordinatesNormalization", "ToCPU"]
    assert SceneLoader(agent, _chain(8192), group=4).padding_to == 8192
    with pytest.raises(RuntimeError):
        next(ld)                                           # not iterated yet
    ld.close()


def test_split_chain_takes_both_kinds_of_transform():
    from deeppointmap_amd import augment
    from deeppointmap_amd.loader import split_chain

    class A:
        transforms = {"ToGPU": {}, "CoordinatesNormalization": {"ratio": 60.0}, "ToTensor": {"padding_to": 4096}}
    for tf in (augment.PointCloudTransforms(A, mode="infer"), augment.get_transforms(A.transforms)):
        chain, pad = split_chain(tf)
        assert pad == 4096 and [type(t).__name__ for t in chain.transforms] == ["ToGPU", "CoordinatesNormalization"]
    chain, pad = split_chain(augment.Compose([augment.ToGPU()]))
    assert pad == -1 and len(chain.transforms) == 1
    with pytest.raises(ValueError):
        split_chain(augment.Compose([augment.ToTensor(), augment.ToGPU()]))      # ToTensor may only end the chain
    with pytest.raises(ValueError):
        split_chain(augment.Compose([augment.ToGPU(), augment.ToTensor(use_calib=True)]))
    with pytest.raises(ValueError):
        split_chain(lambda pcd: pcd)


@pytest.mark.parametrize("kw", [{"group": 0}, {"group": 2.5}, {"group": True}, {"prefetch": -1}, {"prefetch": 1.5},
                                {"streams": 0}, {"capacity": 0}, {"capacity": 10.5}, {"timeout": 0}])
def test_constructor_refuses(tmp_path, kw):
    from deeppointmap_amd.loader import SceneLoader
    agent = _agent(tmp_path, 3)
    with pytest.raises(ValueError):
        SceneLoader(agent, _chain(), **kw)


def test_constructor_refuses_what_is_no_agent(tmp_path):
    from deeppointmap_amd.loader import SceneLoader
    with pytest.raises(ValueError):
        SceneLoader([str(tmp_path / "0.npy")], _chain())
    with pytest.raises(ValueError):
        SceneLoader(_agent(tmp_path, 2), None)
