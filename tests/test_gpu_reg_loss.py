"""GPU: the fused RegistrationLoss (deeppointmap_amd/loss.py, csrc/reg_loss.hip) against the reference's recorded answers
(tests/golden/reg_loss*.npz) and against the plain-torch restatement on the device (tests/reg_loss_restated.py)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reg_loss_cases  # noqa: E402
import reg_loss_restated as R  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = reg_loss_cases.cases()
KEYS = ("xs", "xd", "ps", "pd", "fs", "fd", "cs", "cd", "os", "od")
DEV = "cuda"


def _inputs(name, dtype=torch.float32):
    inputs, cfg, _ = CASES[name]
    t = {k: torch.from_numpy(v).to(DEV) if v.dtype == bool else torch.from_numpy(v).to(DEV, dtype) for k, v in inputs.items()}
    return t, cfg


def _fused(t, cfg, grads=False):
    from deeppointmap_amd.loss import RegistrationLoss
    feats = [t[k].detach().requires_grad_(grads) for k in ("fs", "fd", "cs", "cd")]
    with torch.enable_grad():
        out = RegistrationLoss(cfg)(t["xs"], t["xd"], t["ps"], t["pd"], *feats, t["os"], t["od"])
        g = torch.autograd.grad(out[0], feats) if grads else None
    return out, g


def _vals(out):
    return np.array([float(o) for o in out])


@pytest.mark.parametrize("name", sorted(CASES))
def test_pairs_and_values_equal_reference(name):
    from deeppointmap_amd import ops
    from deeppointmap_amd.loss import RegistrationLoss
    fx = load_golden("reg_loss.npz")
    t, cfg = _inputs(name)
    eps = cfg.loss.eps_positive
    nn_s, nn_d, ne_s, ne_d = ops.reg_loss_pairs(t["xs"].contiguous(), t["xd"].contiguous(), eps, neutral_counts=True)
    for k, v in (("nn_s", nn_s), ("nn_d", nn_d), ("neutral_s", ne_s), ("neutral_d", ne_d)):
        assert np.array_equal(v.cpu().numpy(), fx[f"{name}/{k}"]), k
    ids, mask, neutral = RegistrationLoss.make_pairs(t["xs"].transpose(1, 2), t["xd"].transpose(1, 2), eps)
    assert np.array_equal(ids.cpu().numpy(), fx[f"{name}/nn_s"]) and ids.dtype == torch.int64
    assert torch.equal(mask, ids >= 0)
    assert np.array_equal(neutral.sum(2).cpu().numpy(), fx[f"{name}/neutral_s"])
    out, _ = _fused(t, cfg)
    got = _vals(out)
    ref = fx[f"{name}/out64"] if fx[f"{name}/masks64_equal"] else fx[f"{name}/out32"]
    err = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-6)
    print(f"{name}: relative error of (loss, acc, loss_p, loss_c, loss_o) {np.array2string(err, precision=2)}")
    # top-1 accuracy: equal unless a row's fp64 top-2 gap is below 1e-6 (such rows may flip in fp32)
    fs32, fd32 = t["fs"].float().contiguous(), t["fd"].float().contiguous()
    _, _, _, am_s, am_d = ops.reg_loss_forward(fs32, fd32, None, None, t["ps"].contiguous(), t["pd"].contiguous(), nn_s, nn_d,
                                               cfg.loss.tau, eps, False, argmax=True)
    close = 0
    for side, am in (("s", am_s), ("d", am_d)):
        diff = am.cpu().numpy() != fx[f"{name}/am_{side}"]
        close += int((fx[f"{name}/gap_{side}"] < 1e-6).sum())
        assert not (diff & (fx[f"{name}/gap_{side}"] >= 1e-6)).any(), side
    print(f"{name}: rows with an fp64 top-2 gap below 1e-6: {close}")
    if close == 0:
        assert got[1] == ref[1] or abs(got[1] - ref[1]) < 1e-6
    np.testing.assert_allclose(np.delete(got, 1), np.delete(ref, 1), rtol=1e-5, atol=1e-6)
    assert isinstance(out[1], float) and out[2].dim() == 0 and out[3].dim() == 0


@pytest.mark.parametrize("name", [k for k, v in CASES.items() if v[2]])
def test_gradients_equal_reference(name):
    fg = load_golden("reg_loss_grads.npz")
    t, cfg = _inputs(name)
    _, g = _fused(t, cfg, grads=True)
    for k, gi in zip(("fs", "fd", "cs", "cd"), g):
        want = fg[f"{name}/{k}"]
        err = np.abs(gi.cpu().numpy() - want).max() / np.abs(want).max()
        print(f"{name}/{k}: max |g - g64| / max |g64| = {err:.2e}")
        assert err < 1e-5
    # fine features reach only loss_p and coarse only loss_c: their gradients through those terms alone are the same
    from deeppointmap_amd.loss import RegistrationLoss
    L = cfg.loss
    feats = [t[k].detach().requires_grad_(True) for k in ("fs", "fd", "cs", "cd")]
    with torch.enable_grad():
        out = RegistrationLoss(cfg)(t["xs"], t["xd"], t["ps"], t["pd"], *feats, t["os"], t["od"])
        gp = torch.autograd.grad(out[2], feats[:2])
        gc = torch.autograd.grad(out[3], feats[2:])
    for k, gi, lam in zip(("fs", "fd", "cs", "cd"), gp + gc, (L.lambda_p, L.lambda_p, L.lambda_c, L.lambda_c)):
        want = fg[f"{name}/{k}"] / lam
        assert np.abs(gi.cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max(), k


@pytest.mark.parametrize("name", sorted(CASES))
def test_eval_pairing_acc_equals_reference_top1(name):
    """the static method with the reference's arguments: (B,S,C) features, ~padding, make_pairs' ids and mask"""
    from deeppointmap_amd.loss import RegistrationLoss
    fx = load_golden("reg_loss.npz")
    t, cfg = _inputs(name)
    ids, mask, _ = RegistrationLoss.make_pairs(t["xs"].transpose(1, 2), t["xd"].transpose(1, 2), cfg.loss.eps_positive)
    acc = RegistrationLoss.eval_pairing_acc(t["fs"].transpose(1, 2), t["fd"].transpose(1, 2), ~t["ps"], ids, mask)
    nn, am, gap, pad = fx[f"{name}/nn_s"], fx[f"{name}/am_s"], fx[f"{name}/gap_s"], CASES[name][0]["ps"]
    rows = (nn >= 0) & ~pad
    want = float(np.float32(((am == nn) & rows).sum()) / np.float32(max(rows.sum(), 1.0)))
    assert isinstance(acc, float)
    if (gap[rows] >= 1e-6).all():
        assert acc == want, (acc, want)
    else:
        assert abs(acc - want) <= (gap[rows] < 1e-6).sum() / max(rows.sum(), 1)


def test_bitwise_repeatable():
    t, cfg = _inputs("multi_tile")
    o1, g1 = _fused(t, cfg, grads=True)
    o2, g2 = _fused(t, cfg, grads=True)
    assert all(torch.equal(a, b) if torch.is_tensor(a) else a == b for a, b in zip(o1, o2))
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))


def _large(B, S, D, seed, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    side = (S / 6.0) ** (1 / 3)
    xs = torch.rand(B, 3, S, generator=g) * side
    idx = torch.randint(0, S, (B, D), generator=g)
    xd = torch.gather(xs, 2, idx.unsqueeze(1).expand(B, 3, D)) + (torch.rand(B, 3, D, generator=g) - 0.5) * 0.3
    f = lambda C, N: torch.randn(B, C, N, generator=g)
    fs, cs = f(256, S), f(128, S)
    fd = torch.gather(fs, 2, idx.unsqueeze(1).expand(B, 256, D)) + 0.8 * f(256, D)
    cd = torch.gather(cs, 2, idx.unsqueeze(1).expand(B, 128, D)) + 0.8 * f(128, D)
    ps = torch.zeros(B, S, dtype=torch.bool)
    pd = torch.zeros(B, D, dtype=torch.bool)
    ps[:, S - S // 16:] = True
    pd[:, D - D // 20:] = True
    t = dict(xs=xs, xd=xd, ps=ps, pd=pd, fs=fs, fd=fd, cs=cs, cd=cd, os=torch.randn(50, 3, 1, generator=g),
             od=torch.randn(60, 3, 1, generator=g))
    return {k: v.to(DEV) if v.dtype == torch.bool else v.to(DEV, dtype) for k, v in t.items()}


@pytest.mark.parametrize("S", [2048, 4096])
def test_against_restatement_on_device(S):
    from deeppointmap_amd import ops
    t = _large(4, S, S, S)
    cfg = reg_loss_cases.cfg("euclidean", lambda_p=0.8, lambda_c=1.3, lambda_o=0.5)
    out, g = _fused(t, cfg, grads=S == 2048)
    feats = [t[k].detach().requires_grad_(S == 2048) for k in ("fs", "fd", "cs", "cd")]
    with torch.enable_grad():
        want, extra = R.registration_loss(t["xs"], t["xd"], t["ps"], t["pd"], *feats, t["os"], t["od"], cfg)
        gw = torch.autograd.grad(want[0], feats) if S == 2048 else None
    nn_s, nn_d, ne_s, ne_d = ops.reg_loss_pairs(t["xs"], t["xd"], cfg.loss.eps_positive, neutral_counts=True)
    for k, v in (("nn_s", nn_s), ("nn_d", nn_d), ("neutral_s", ne_s), ("neutral_d", ne_d)):
        assert torch.equal(v.long(), extra[k]), k
    got, ref = _vals(out), _vals(want)
    print(f"S=D={S}: fused {got}, restated {ref}, relative error {np.abs(got - ref) / np.abs(ref)}")
    np.testing.assert_allclose(np.delete(got, 1), np.delete(ref, 1), rtol=1e-5)
    # top-1 row by row against the fp64 argmax: only rows whose fp64 top-2 gap is below 1e-6 may differ
    _, _, _, am_s, am_d = ops.reg_loss_forward(t["fs"], t["fd"], None, None, t["ps"], t["pd"], nn_s, nn_d, cfg.loss.tau,
                                               cfg.loss.eps_positive, False, argmax=True)
    unit = lambda f: f.double() / f.double().norm(dim=1, keepdim=True).clamp_min(1e-12)
    sim = torch.einsum("bcm,bcn->bmn", unit(t["fs"]), unit(t["fd"]))
    near_ties, hits, ref_hits = 0, [], []
    top1 = lambda am, nn, rows: float(np.float32(int(((am == nn) & rows).sum())) / np.float32(max(int(rows.sum()), 1)))
    for am, am_r, s64, nn, pad in ((am_s, extra["argmax_s"], sim, nn_s, t["ps"]),
                                   (am_d, extra["argmax_d"], sim.transpose(1, 2), nn_d, t["pd"])):
        top2 = torch.topk(s64, 2, dim=2)
        close = (top2.values[..., 0] - top2.values[..., 1]) < 1e-6
        near_ties += int(close.sum())
        assert not ((am.long() != top2.indices[..., 0]) & ~close).any()
        assert not ((am.long() != am_r) & ~close).any()
        rows = (nn >= 0) & ~pad
        hits.append(top1(am, nn, rows)), ref_hits.append(top1(am_r, nn, rows))
        del s64, top2
    del sim
    print(f"S=D={S}: rows with an fp64 top-2 gap below 1e-6: {near_ties}")
    assert got[1] == (hits[0] + hits[1]) / 2
    if near_ties == 0:
        assert hits == ref_hits
    # the restatement divides hits / rows on the device, which may round the quotient one fp32 ulp differently
    assert abs(got[1] - ref[1]) <= 2e-7 + near_ties / (4 * S)
    if g is not None:
        for a, b in zip(g, gw):
            err = float((a - b).abs().max() / b.abs().max())
            print(f"  gradient: max |g - g_restated| / max |g_restated| = {err:.2e}")
            assert err < 1e-5


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_inputs_and_transposed_views(dtype):
    t, cfg = _inputs("padding_both")
    want, gw = _fused({k: v.clone() for k, v in t.items()}, cfg, grads=True)
    # transposed views: the same values laid out (B,S,C) and viewed as (B,C,S)
    tv = dict(t)
    for k in ("fs", "fd", "cs", "cd"):
        tv[k] = t[k].transpose(1, 2).contiguous().transpose(1, 2)
        assert not tv[k].is_contiguous()
    got, gg = _fused(tv, cfg, grads=True)
    assert all((torch.equal(a, b) if torch.is_tensor(a) else a == b) for a, b in zip(got, want))
    assert all(torch.equal(a, b) for a, b in zip(gg, gw))
    th = dict(t)
    for k in ("fs", "fd", "cs", "cd"):
        th[k] = t[k].to(dtype)
    oh, gh = _fused(th, cfg, grads=True)
    assert all(g.dtype == dtype for g in gh)
    up = dict(t)
    for k in ("fs", "fd", "cs", "cd"):
        up[k] = th[k].float()
    ou, gu = _fused(up, cfg, grads=True)   # the fp32 computation on the rounded inputs
    assert float(oh[0]) == float(ou[0])
    assert all(torch.equal(a, b.to(dtype)) for a, b in zip(gh, gu))


def test_refusals():
    from deeppointmap_amd import _lib
    from deeppointmap_amd.loss import RegistrationLoss
    t, cfg = _inputs("s_ne_d_lambda")
    m = RegistrationLoss(cfg)
    with pytest.raises(_lib.DpmError):
        m(*(t[k].cpu() for k in KEYS))
    bad = dict(t, fs=t["fs"][:, :100], fd=t["fd"][:, :100])
    with pytest.raises(ValueError):
        m(*(bad[k] for k in KEYS))
    with pytest.raises(ValueError):
        RegistrationLoss(reg_loss_cases.cfg("chebyshev"))(*(t[k] for k in KEYS))
    # coordinates, masks and features that disagree in B or point count: refused before any kernel indexes them together
    for k, v in (("ps", t["ps"][:, :-1]), ("pd", t["pd"][:1]), ("xd", t["xd"][:, :, :-1]), ("xs", t["xs"][:1]),
                 ("cs", t["cs"][:, :, :-2]), ("fd", t["fd"][:1])):
        with pytest.raises(ValueError):
            m(*(dict(t, **{k: v})[k2] for k2 in KEYS))
    from deeppointmap_amd import ops
    xs, xd = t["xs"].contiguous(), t["xd"].contiguous()
    with pytest.raises(ValueError):
        ops.reg_loss_pairs(xs, xd[:1].contiguous(), 0.5)
    nn_s, nn_d = ops.reg_loss_pairs(xs, xd, 0.5)
    fs, fd, ps, pd = t["fs"].contiguous(), t["fd"].contiguous(), t["ps"].contiguous(), t["pd"].contiguous()
    for args in ((fs, fd, xs, xd, ps[:, :-1].contiguous(), pd, nn_s, nn_d), (fs, fd, xs, xd, ps, pd, nn_s, nn_d[:, 1:].contiguous()),
                 (fs, fd, xs[:, :, 1:].contiguous(), xd, ps, pd, nn_s, nn_d)):
        with pytest.raises(ValueError):
            ops.reg_loss_forward(*args, 0.1, 0.5, True)


def test_no_positives_gives_zero_tensor_and_zero_gradient():
    t, cfg = _inputs("no_pos_both")
    out, g = _fused(t, cfg, grads=True)
    assert torch.is_tensor(out[2]) and out[2].dim() == 0 and float(out[2]) == 0.0 and float(out[3]) == 0.0
    assert all(float(x.abs().max()) == 0.0 for x in g)


def test_sgd_step_matches_restatement():
    """one SGD step of a small head (two Conv1d, as the pairing heads) through the fused loss and through the restatement"""
    from deeppointmap_amd.loss import RegistrationLoss
    t = _large(2, 700, 650, 7)
    cfg = reg_loss_cases.cfg("manhattan", lambda_p=1.0, lambda_c=0.6, lambda_o=1.0)
    torch.manual_seed(0)
    heads = []
    for _ in range(2):
        h = torch.nn.ModuleDict(dict(fine=torch.nn.Sequential(torch.nn.Conv1d(256, 256, 1), torch.nn.ReLU(), torch.nn.Conv1d(256, 256, 1)),
                                     coarse=torch.nn.Conv1d(128, 128, 1))).to(DEV)
        heads.append(h)
    heads[1].load_state_dict(heads[0].state_dict())
    for h, fn in ((heads[0], lambda *a: RegistrationLoss(cfg)(*a)), (heads[1], lambda *a: R.registration_loss(*a, cfg)[0])):
        opt = torch.optim.SGD(h.parameters(), lr=0.5)
        with torch.enable_grad():
            out = fn(t["xs"], t["xd"], t["ps"], t["pd"], h["fine"](t["fs"]), h["fine"](t["fd"]), h["coarse"](t["cs"]),
                     h["coarse"](t["cd"]), t["os"], t["od"])
            opt.zero_grad()
            out[0].backward()
        opt.step()
    for (k, a), b in zip(heads[0].state_dict().items(), heads[1].state_dict().values()):
        err = float((a - b).abs().max())
        assert err < 1e-5, (k, err)


def test_memory_stays_linear():
    """B = 2, S = D = 16384: one dense (B,S,D) fp32 matrix alone would be 2 GiB"""
    B, S = 2, 16384
    t = _large(B, S, S, 3)
    cfg = reg_loss_cases.cfg("manhattan")
    feats = [t[k].requires_grad_(True) for k in ("fs", "fd", "cs", "cd")]
    inputs = sum(f.numel() * 4 for f in feats)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    from deeppointmap_amd.loss import RegistrationLoss
    with torch.enable_grad():
        out = RegistrationLoss(cfg)(*(t[k] for k in KEYS))
        g = torch.autograd.grad(out[0], feats)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak above baseline {peak / 2**20:.1f} MiB, feature inputs {inputs / 2**20:.1f} MiB")
    assert peak < 3 * inputs + 64 * 2**20
    assert all(torch.isfinite(x).all() for x in g) and np.isfinite(float(out[0]))
