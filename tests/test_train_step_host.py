"""CPU: the host side of the training step against the reference's recorded run (tests/golden/train_step_<case>.npz, made by
tests/golden/make_golden_train_step.py from the reference's own _train_registration in fp32 and fp64).

  * the plain-torch restatement of the map assembly (tests/train_step_restated.py) in fp64: feature rows and masks exact,
    coordinates, gt and src_global to 1e-12 relative to the largest magnitude of the tensor (two fp64 evaluations of one
    function in different operation orders: 1.1e-16 per rounding, a dozen roundings, a calib condition number below 100; the
    fixture restores the fp64 run from fp32 parts to ~1e-13).  This pins the comparator the GPU tests take gradients through.
  * train_pipeline.refined_pose / icp_table against every lookup the reference made: which entries fall back, and the bytes
    of the fp32 pose.
  * train_pipeline.draw_s1 against the recorded `random` calls.
  * the optimiser / scheduler factories, the drop-in import paths, the binding table.
"""
import os
import pickle
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_step_cases as C  # noqa: E402
import train_step_restated as R  # noqa: E402

CASES = C.cases()
RUNS = [(name, seed) for name, inputs in CASES.items() for seed in inputs["seeds"]]
_FIX = {}


def fixture(name):
    if name not in _FIX:
        _FIX[name] = C.load_fixture(name, GOLDEN)
    return _FIX[name]


def host_lookup(inputs, S1):
    """-> (icp (F+B,16) float32, has_icp (F+B,) uint8) from the project's host lookup on the case's dictionary"""
    from deeppointmap_amd.train_pipeline import icp_table
    table = C.se3_dict(inputs)
    return icp_table(inputs["pcd_index"], [table if u else None for u in inputs["uses_dict"]], S1)


def restated(inputs, S1, dtype, device="cpu"):
    """the restatement's six outputs and (rel, gt) on the case's inputs, with the host lookup's answer"""
    icp, has = host_lookup(inputs, S1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)   # noqa: E731
    rel, gt = R.poses(t(inputs["R"]), t(inputs["T"]), t(inputs["calib"]), t(icp), torch.from_numpy(has).to(device), inputs["S"], S1)
    outs = R.assemble(t(inputs["coor"]), t(inputs["fea"]), torch.from_numpy(inputs["mask"]).to(device), rel, gt, inputs["S"], S1,
                      C.COOR_SCALE)
    return outs, rel, gt


@pytest.mark.parametrize("name,seed", RUNS)
def test_restatement_matches_the_reference_in_fp64(name, seed):
    inputs, fix = CASES[name], fixture(name)
    S1, Cc = int(fix[f"{seed}/S1"]), inputs["C"]
    (src_desc, dst_desc, src_mask, dst_mask, src_global, dst_global), rel, gt = restated(inputs, S1, torch.float64)
    got = {"src_desc": src_desc, "dst_desc": dst_desc, "gt": gt, "src_global": src_global, "dst_global": dst_global}
    assert np.array_equal(src_mask.numpy(), fix[f"{seed}/src_mask"]) and np.array_equal(dst_mask.numpy(), fix[f"{seed}/dst_mask"])
    for k in ("src_desc", "dst_desc"):
        assert np.array_equal(got[k][:, :Cc].numpy().astype(np.float32), fix[f"{seed}/{k}/32"][:, :Cc]), k   # inputs are fp32 values
    for k, v in got.items():
        want = fix[f"{seed}/{k}/64"]
        assert v.shape == want.shape, (k, v.shape, want.shape)
        err = np.abs(v.numpy() - want).max() / np.abs(want).max()
        assert err <= 1e-12, (k, err)
    # a map's first frame: coor * coor_scale and nothing else, in fp32 the reference's bytes
    (s32, d32, *_), _, _ = restated(inputs, S1, torch.float32)
    N = inputs["N"]
    assert np.array_equal(s32[:, Cc:, :N].numpy(), fix[f"{seed}/src_desc/32"][:, Cc:, :N])
    assert np.array_equal(d32[:, Cc:, :N].numpy(), fix[f"{seed}/dst_desc/32"][:, Cc:, :N])


@pytest.mark.parametrize("name,seed", RUNS)
def test_host_lookup_matches_every_reference_lookup(name, seed):
    """each top-level get_SE3_from_dict call of the reference's run -- (s, d, bridge), whether it raised, the `.float()` pose --
    against refined_pose; then icp_table's rows against the same record (the reference makes its calls in the order gt, source
    map, target map, each map by map)"""
    from deeppointmap_amd.train_pipeline import refined_pose
    inputs, fix = CASES[name], fixture(name)
    table = C.se3_dict(inputs)
    look, ok, want = fix[f"{seed}/lookups"], fix[f"{seed}/lookup_ok"], fix[f"{seed}/lookup_icp"]
    assert len(look) == len(ok) == len(want)
    for (s, d, bridge), good, pose in zip(look, ok, want):
        M = refined_pose(table, int(s), int(d), None if bridge < 0 else int(bridge))
        assert (M is not None) == bool(good), (s, d, bridge)
        if good:
            assert M.dtype == np.float64 and M.astype(np.float32).reshape(16).tobytes() == pose.tobytes(), (s, d, bridge)
    S1, B, S = int(fix[f"{seed}/S1"]), inputs["B"], inputs["S"]
    icp, has = host_lookup(inputs, S1)
    F = B * S
    recorded = {(int(s), int(d), int(b)): (bool(g), p) for (s, d, b), g, p in zip(look, ok, want)}
    idx = inputs["pcd_index"]
    seen = 0
    for b in range(B):
        entries = [(F + b, idx[b, 0], idx[b, S1], -1)] + [(b * S + s, idx[b, s], idx[b, 0], -1) for s in range(1, S1)] + \
                  [(b * S + s, idx[b, s], idx[b, S1], idx[b, 0]) for s in range(S1 + 1, S)]
        for e, s, d, bridge in entries:
            if not inputs["uses_dict"][b]:
                assert has[e] == 0
                continue
            good, pose = recorded[(int(s), int(d), int(bridge))]
            assert bool(has[e]) == good, (b, e)
            if good:
                assert icp[e].tobytes() == pose.tobytes()
            seen += 1
        for first in (b * S, b * S + S1):
            assert has[first] == 0
    assert seen == len(look)
    if name == "b":
        assert (~ok).any(), "case (b) must reach the fallback"


class _Replay:
    """a `random` that answers with the recorded values and checks the calls"""

    def __init__(self, log):
        self.log, self.at = log, 0

    def random(self):
        kind, _, _, v = self.log[self.at]
        assert kind == 0
        self.at += 1
        return float(v)

    def randint(self, a, b):
        kind, ra, rb, v = self.log[self.at]
        assert kind == 1 and (a, b) == (int(ra), int(rb)), (a, b, ra, rb)
        self.at += 1
        return int(v)


@pytest.mark.parametrize("name,seed", RUNS)
def test_s1_draw_follows_the_recorded_random_calls(name, seed):
    import random
    from deeppointmap_amd.train_pipeline import draw_s1
    inputs, fix = CASES[name], fixture(name)
    replay = _Replay(fix[f"{seed}/rand_log"])
    assert draw_s1(inputs["S"], inputs["map_size_max"], replay) == int(fix[f"{seed}/S1"])
    assert replay.at == len(replay.log), "the reference made more calls"
    random.seed(seed)   # and a seeded run picks the reference's S1
    assert draw_s1(inputs["S"], inputs["map_size_max"]) == int(fix[f"{seed}/S1"])


def test_fixture_covers_both_s1_branches_the_bridge_and_the_fallback():
    fix = fixture("b")
    s1 = [int(fix[f"{seed}/S1"]) for seed in CASES["b"]["seeds"]]
    assert 1 in s1 and max(s1) > 1
    look = np.concatenate([fix[f"{seed}/lookups"] for seed in CASES["b"]["seeds"]])
    ok = np.concatenate([fix[f"{seed}/lookup_ok"] for seed in CASES["b"]["seeds"]])
    keys = {tuple(k) for k in CASES["b"]["dict_keys"].tolist()}
    direct = lambda s, d: (min(s, d), max(s, d)) in keys   # noqa: E731
    assert any(g and s == d for (s, d, b), g in zip(look, ok)), "a repeated frame"
    assert any(g and s > d and direct(s, d) for (s, d, b), g in zip(look, ok)), "a direct key"
    assert any(g and s < d and direct(s, d) for (s, d, b), g in zip(look, ok)), "a reversed key"
    assert any(g and s != d and not direct(s, d) and b >= 0 for (s, d, b), g in zip(look, ok)), "a pose over the bridge"
    assert any(not g and b >= 0 for (s, d, b), g in zip(look, ok)) and any(not g and b < 0 for (s, d, b), g in zip(look, ok))
    assert int(fixture("c")["0/S1"]) in (3, 4) and CASES["c"]["S"] > CASES["c"]["map_size_max"]
    for inputs in CASES.values():
        assert np.linalg.cond(inputs["calib"]).max() < 100


def test_pipeline_caches_pickles_per_file(tmp_path):
    from deeppointmap_amd.train_pipeline import DeepPointModelPipeline
    path = str(tmp_path / "refined.pkl")
    with open(path, "wb") as f:
        pickle.dump(C.se3_dict(CASES["b"]), f)
    me = SimpleNamespace(refined_SE3_cache={})
    first = DeepPointModelPipeline._load_refined_SE3(me, path)
    os.remove(path)
    assert DeepPointModelPipeline._load_refined_SE3(me, path) is first and sorted(first) == sorted(C.se3_dict(CASES["b"]))
    assert DeepPointModelPipeline._load_refined_SE3(me, "") is None and set(me.refined_SE3_cache) == {path, ""}


def test_factories():
    from deeppointmap_amd import optim as O
    cfg = lambda type, **kw: SimpleNamespace(type=type, kwargs=kw)   # noqa: E731
    p = [torch.nn.Parameter(torch.zeros(3))]
    for name, cls in (("AdamW", O.AdamW), ("adam", O.Adam), ("SGD", O.SGD)):
        opt = O.Optimizer(cfg(name, lr=0.25))(p)
        assert type(opt) is cls and isinstance(opt, torch.optim.Optimizer) and opt.param_groups[0]["lr"] == 0.25
    with pytest.raises(NotImplementedError):
        O.Optimizer(cfg("rmsprop"))
    opt = O.Optimizer(cfg("adamw", lr=1.0, weight_decay=0.5))(p)
    assert opt.param_groups[0]["weight_decay"] == 0.5 and opt.param_groups[0]["decoupled_weight_decay"] is True
    for name, kw, cls in (("identity", {}, O.IdentityScheduler), ("cosine", dict(T_max=4), torch.optim.lr_scheduler.CosineAnnealingLR),
                          ("cosine_restart", dict(T_0=2), torch.optim.lr_scheduler.CosineAnnealingWarmRestarts)):
        sch = O.Scheduler(cfg(name, **kw))(opt)
        assert type(sch) is cls
        sch.step()
    with pytest.raises(NotImplementedError):
        O.Scheduler(cfg("step"))
    for bad in (dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(ValueError):
            O.AdamW(p, **bad)
    with pytest.raises(ValueError):
        O.Adam([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))])
    with pytest.raises(ValueError):
        O.SGD(p, maximize=True)
    # the state dict's param_groups carry torch's keys, so torch's classes load it (and ours load torch's)
    for ours, theirs, kw in ((O.AdamW, torch.optim.AdamW, {}), (O.Adam, torch.optim.Adam, {}), (O.SGD, torch.optim.SGD, dict(momentum=0.5))):
        a, b = ours(p, lr=0.1, **kw), theirs(p, lr=0.1, **kw)
        assert sorted(a.state_dict()["param_groups"][0]) == sorted(b.state_dict()["param_groups"][0])
        b.load_state_dict(a.state_dict()), a.load_state_dict(b.state_dict())
    rec = O.Recorder()
    rec.add_dict({"loss": 3.0}), rec.add_dict({"loss": 1.0}), rec.add_item("acc", 0.5), rec.add_item("acc", 0.75)
    assert rec.best() == {"loss": 1.0, "acc": 0.75} and rec.mean() == {"loss": 2.0, "acc": 0.625} and "loss" in rec.tostring()
    lin = torch.nn.Linear(2, 2)
    O.try_load_state_dict(lin, {"weight": torch.ones(2, 2)}, log=False)   # a missing key: loaded non-strictly, no exception
    assert float(lin.weight.sum()) == 4.0


def test_dropin_paths_resolve_without_open3d_or_colorlog():
    code = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(1, %r)\n"
        "from pipeline.modules.model_pipeline import DeepPointModelPipeline\n"
        "from pipeline.modules.utils import Optimizer, Scheduler, Recorder, try_load_state_dict, fakecast\n"
        "import deeppointmap_amd.train_pipeline as t, deeppointmap_amd.optim as o\n"
        "assert DeepPointModelPipeline is t.DeepPointModelPipeline and Optimizer is o.Optimizer and Scheduler is o.Scheduler\n"
        "assert 'open3d' not in sys.modules and 'colorlog' not in sys.modules\n"
        "with fakecast(): pass\n"
        "print('ok')\n") % (os.path.join(ROOT, "deeppointmap_amd", "dropin"), ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]


def test_binding_table_carries_the_new_entry_points():
    from deeppointmap_amd import _lib
    from deeppointmap_amd.csrc import build
    for name in ("dpm_map_poses", "dpm_map_assemble_fwd", "dpm_map_assemble_bwd", "dpm_optim_step", "dpm_optim_chunk"):
        assert name in _lib.SIGNATURES, name
    assert "map_assemble.hip" in build.SOURCES and "optim.hip" in build.SOURCES
    header = open(os.path.join(ROOT, "include", "dpm_hip.h")).read()
    assert "model_pipeline.py" in header.split("int dpm_map_poses(")[0][-3000:]
