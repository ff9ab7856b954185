"""GPU: the one-launch optimisers (deeppointmap_amd/optim.py over csrc/optim.hip) against torch.optim on the CPU.

Comparison targets: torch.optim.AdamW / Adam / SGD on the CPU in fp64 (`ref64`) and in fp32 (`ref32`) on the same parameters,
gradients and learning-rate schedule -- torch, not the code under test.  Bound, per tensor, for the parameters and for every
state tensor:  max |hip - ref64| <= max(3 max |ref32 - ref64|, steps 2^-23 max |ref64|): the project's three-way rule
(profiles/r06_margin_three_way.md) with a floor of one fp32 rounding of the largest value per step taken.  Every observed error
goes to profiles/train_step_accuracy.md through test_logs/train_step_errors.log (scripts/train_step_bench.py collects it).
"""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = (1, 3, 63, 64, 65, 4097, 0)   # + one tensor without a gradient and one view at a 4-byte offset (make_params)
STEPS = 6
ALGOS = {
    "adamw": ("AdamW", dict(lr=1e-2, weight_decay=0.05)),
    "adamw_nodecay": ("AdamW", dict(lr=1e-2, weight_decay=0.0, betas=(0.8, 0.99))),
    "adam": ("Adam", dict(lr=1e-2)),
    "adam_decay": ("Adam", dict(lr=1e-2, weight_decay=0.05, eps=1e-6)),
    "sgd": ("SGD", dict(lr=1e-2)),
    "sgd_decay": ("SGD", dict(lr=1e-2, weight_decay=0.05)),
    "sgd_momentum": ("SGD", dict(lr=1e-2, momentum=0.9, dampening=0.1, weight_decay=0.05)),
    "sgd_nesterov": ("SGD", dict(lr=1e-2, momentum=0.9, nesterov=True)),
}


def log(line):
    print(line)
    try:
        os.makedirs(os.path.join(ROOT, "test_logs"), exist_ok=True)
        with open(os.path.join(ROOT, "test_logs", "train_step_errors.log"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def values(seed=7):
    """per tensor its initial value and STEPS gradients (numpy float32): gradients hold exact zeros and a 1e4 outlier"""
    rng = np.random.default_rng(seed)
    out = []
    for n in SIZES + (5, 130):   # the last two: the tensor without a gradient, the misaligned view
        p = rng.standard_normal(n).astype(np.float32)
        g = rng.standard_normal((STEPS, n)).astype(np.float32)
        g[:, ::3] = 0.0
        if n:
            g[1, n // 2] = 1e4
        out.append((p, g))
    return out


def make_params(vals, device, dtype, misalign=True):
    """leaf parameters of the values; the last one is a view one element into a larger buffer (4-byte offset, not 16-byte
    aligned) when `misalign`"""
    params = []
    for i, (p, _) in enumerate(vals):
        t = torch.from_numpy(p).clone().to(device=device, dtype=dtype)   # a copy: steps on the CPU must not reach `vals`
        if misalign and i == len(vals) - 1:
            buf = torch.zeros(t.numel() + 8, device=device, dtype=dtype)
            buf[1:1 + t.numel()] = t
            t = buf[1:1 + t.numel()]
            assert device == "cpu" or t.data_ptr() % 16 == 4
        params.append(torch.nn.Parameter(t))
    return params


NO_GRAD = len(SIZES)   # index of the tensor that never gets a gradient


def run(opt_cls, kw, vals, device, dtype, steps=range(STEPS), state=None, noncontiguous=False, misalign=True, params=None,
        no_grad=NO_GRAD):
    """`steps` optimiser steps with a CosineAnnealingLR stepped after every step (the lr changes under the optimiser)"""
    params = make_params(vals, device, dtype, misalign) if params is None else params
    opt = opt_cls(params, **kw)
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=STEPS)
    if state is not None:
        opt.load_state_dict(state[0]), sch.load_state_dict(state[1])
    for k in steps:
        for i, (p, (_, g)) in enumerate(zip(params, vals)):
            if i == no_grad:
                continue
            gk = torch.from_numpy(g[k]).clone().to(device=device, dtype=dtype)
            if noncontiguous and gk.numel() > 1:
                gk = torch.stack([gk, gk], dim=1)[:, 0]
                assert not gk.is_contiguous()
            p.grad = gk
        opt.step()
        sch.step()
    return params, opt, sch


def state_arrays(params, opt):
    out = {}
    for i, p in enumerate(params):
        out[f"p{i}"] = p.detach().cpu().double().numpy()
        for k, v in opt.state.get(p, {}).items():
            if torch.is_tensor(v) and k != "step":
                out[f"{k}{i}"] = v.detach().cpu().double().numpy()
    return out


def three_way(what, hip, ref32, ref64, steps):
    assert sorted(hip) == sorted(ref64) == sorted(ref32), (sorted(hip), sorted(ref64))
    worst = 0.0
    for k, want in ref64.items():
        if want.size == 0:
            assert hip[k].size == 0
            continue
        err, e = np.abs(hip[k] - want).max(), np.abs(ref32[k] - want).max()
        bound = max(3 * e, steps * 2.0 ** -23 * np.abs(want).max())
        worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
        log(f"optim {what} {k}: max|hip-ref64| {err:.3e}, max|ref32-ref64| {e:.3e}, bound {bound:.3e}")
        assert err <= bound, (what, k, err, bound)
    return worst


@pytest.mark.parametrize("name", sorted(ALGOS))
def test_six_steps_against_torch_on_the_cpu(name):
    from deeppointmap_amd import optim as O
    cls, kw = ALGOS[name]
    vals = values()
    hp, hopt, _ = run(getattr(O, cls), kw, vals, DEV, torch.float32)
    p32, o32, _ = run(getattr(torch.optim, cls), kw, vals, "cpu", torch.float32)
    p64, o64, _ = run(getattr(torch.optim, cls), kw, vals, "cpu", torch.float64)
    three_way(name, state_arrays(hp, hopt), state_arrays(p32, o32), state_arrays(p64, o64), STEPS)
    # the tensor without a gradient: unchanged, no state, and the step counters of the others are torch's
    assert torch.equal(hp[NO_GRAD].detach().cpu(), torch.from_numpy(vals[NO_GRAD][0])) and hp[NO_GRAD] not in hopt.state
    for a, b in zip(hp, p32):
        sa, sb = hopt.state.get(a, {}), o32.state.get(b, {})
        assert sorted(sa) == sorted(sb)
        if "step" in sb:
            assert not sa["step"].is_cuda and float(sa["step"]) == float(sb["step"]) == STEPS
    assert all(p._version >= STEPS for i, p in enumerate(hp) if i != NO_GRAD)   # in-place updates are announced to autograd


def test_identical_bytes_twice_and_any_chunking():
    """the update is element-wise: two runs agree byte for byte, and the same values laid out as ONE tensor (aligned, many
    chunks) or as many (odd lengths, scalar tails, a misaligned view) give the same bytes; a non-contiguous gradient too"""
    from deeppointmap_amd import optim as O
    vals = values()
    with_grad = [v for i, v in enumerate(vals) if i != NO_GRAD]
    for name in ("adamw", "adam_decay", "sgd_momentum"):
        cls, kw = ALGOS[name]
        a, oa, _ = run(getattr(O, cls), kw, vals, DEV, torch.float32)
        b, ob, _ = run(getattr(O, cls), kw, vals, DEV, torch.float32, noncontiguous=True)
        sa, sb = state_arrays(a, oa), state_arrays(b, ob)
        assert sorted(sa) == sorted(sb) and all(sa[k].tobytes() == sb[k].tobytes() for k in sa), name
        one = [(np.concatenate([p for p, _ in with_grad]), np.concatenate([g for _, g in with_grad], axis=1))]
        c, oc, _ = run(getattr(O, cls), kw, one, DEV, torch.float32, misalign=False, no_grad=-1)
        many = np.concatenate([sa[f"p{i}"] for i in range(len(vals)) if i != NO_GRAD])
        assert state_arrays(c, oc)["p0"].tobytes() == many.tobytes(), name
        for key in ("exp_avg", "exp_avg_sq", "momentum_buffer"):
            if f"{key}0" in sa:
                many = np.concatenate([sa[f"{key}{i}"] for i in range(len(vals)) if i != NO_GRAD])
                assert state_arrays(c, oc)[f"{key}0"].tobytes() == many.tobytes(), (name, key)


def test_state_dict_round_trip_with_torch_adamw():
    """three steps here, three more in torch.optim.AdamW from our state dict -- and the other way round -- against six
    uninterrupted steps of torch on the CPU in fp64 / fp32, with the same bound"""
    from deeppointmap_amd import optim as O
    cls, kw = ALGOS["adamw"]
    vals = values()
    p32, o32, _ = run(torch.optim.AdamW, kw, vals, "cpu", torch.float32)
    p64, o64, _ = run(torch.optim.AdamW, kw, vals, "cpu", torch.float64)
    r32, r64 = state_arrays(p32, o32), state_arrays(p64, o64)
    first, rest = range(3), range(3, STEPS)

    def detached(params):
        return [torch.nn.Parameter(p.detach().clone()) for p in params]
    # ours -> torch (on the GPU: torch.optim.AdamW loads our dict, the parameters continue where ours stopped)
    hp, hopt, hsch = run(O.AdamW, kw, vals, DEV, torch.float32, steps=first, misalign=False)
    tp, topt, _ = run(torch.optim.AdamW, kw, vals, DEV, torch.float32, steps=rest, state=(hopt.state_dict(), hsch.state_dict()),
                      params=detached(hp))
    three_way("ours->torch", state_arrays(tp, topt), r32, r64, STEPS)
    # torch -> ours
    tp, topt, tsch = run(torch.optim.AdamW, kw, vals, DEV, torch.float32, steps=first, misalign=False)
    hp, hopt, _ = run(O.AdamW, kw, vals, DEV, torch.float32, steps=rest, state=(topt.state_dict(), tsch.state_dict()),
                      params=detached(tp))
    three_way("torch->ours", state_arrays(hp, hopt), r32, r64, STEPS)
    assert all(float(st["step"]) == STEPS for st in hopt.state.values())


def test_tables_are_rebuilt_only_when_an_address_changes_and_step_does_not_synchronise():
    from deeppointmap_amd import optim as O
    params = [torch.nn.Parameter(torch.randn(n, device=DEV)) for n in (5, 4097, 64)]
    for p in params:
        p.grad = torch.randn_like(p)
    opt = O.AdamW(params, lr=1e-3)
    opt.step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")   # any synchronising torch call inside step() raises
    try:
        for _ in range(3):
            for p in params:
                p.grad.mul_(0.5)              # same gradient storage
            opt.step()
        assert opt.plan_builds == 1
        old = params[1].grad
        params[1].grad = torch.ones_like(old)  # a new address (the old tensor is still alive): one rebuild, also without a sync
        opt.step()
        assert opt.plan_builds == 2
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(torch.isfinite(p).all() for p in params)


def test_refusals():
    from deeppointmap_amd import _lib, optim as O
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    with pytest.raises(_lib.DpmError):
        O.AdamW([p]).step()   # CPU tensors: no fallback
