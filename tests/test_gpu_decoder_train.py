"""GPU: the decoder's training forward (Decoder.forward in .train() mode), its attention kernels (csrc/attention_train.hip) and
offset pairing (csrc/offset_pairs.hip), alone and through RegistrationLoss and backward().

References: the reference's recorded answers (tests/golden/decoder_train_<case>.partNN.npz, fp32 and fp64 runs) and, for what
the fixture only samples, the plain-torch restatement run in fp64 on the device (tests/decoder_train_restated.py, pinned to
the fixture by tests/test_decoder_train_host.py).

Bounds.  Forward features: the project's rule (conftest.assert_features_close, 1e-5 x scale).  Loss and every gradient, per
tensor in the maximum norm relative to max |fp64|: max(3 e, FLOOR) with e = |reference fp32 - reference fp64| of that tensor
(recorded by the fixture; for the attention operator alone: dense fp32 torch autograd on the device against the same in fp64)
-- factor 3 is the margin the project grants over the reference's own fp32 error (tests/test_gpu_margin.py) -- and FLOOR
twice the worst error of the dense fp32 torch restatement on the device against the fp64 one, measured once on the first GPU
run (profiles/decoder_train_accuracy.md has the figures): an independent fp32 evaluation of the same function.  That run gave
6.95e-6 as the worst of four cases and 1.1e-2 on `no_pairs`, where torch's default fp32 GEMM backend (hipBLASLt) returns
gradients that far from fp64 and its rocBLAS backend 5.1e-6: a defect of that evaluation, not its rounding error, so it is left
out and FLOOR is the smaller figure, 1.4e-5 (the HIP path sits at 8.2e-6 on that case).
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, assert_features_close

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_train_cases as C  # noqa: E402
import decoder_train_restated as R  # noqa: E402
from test_decoder_train_host import rel_err, run_restated  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = C.cases()
DEV = "cuda"
FLOOR = 1.4e-5   # 2 x 6.95e-6 (plain_256, d/d similarity_head.2.bias): see the docstring and profiles/decoder_train_accuracy.md


def check(what, got, want64, e):
    """max |got - want64| / max |want64| <= max(3 e, FLOOR); asserted and logged by conftest's observed-error log (both sides
    divided by max |want64|, so that its scale is 1 and its tolerance the relative bound)"""
    got, want64 = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    m = float(np.abs(want64).max()) if want64.size else 0.0
    m = m if m > 0.0 else 1.0
    bound = max(3 * e, FLOOR)
    assert_features_close(got / m, want64 / m, f"{what} (e {e:.2e})", tol=bound)
    return rel_err(got, want64)


# ---- the attention operator ------------------------------------------------------------------------------------------------

def _qkv(B, M, N, seed, mask):
    gen = torch.Generator().manual_seed(seed)
    q, k, v, do = (torch.randn(B * n, 256, generator=gen).to(DEV) for n in (M, N, N, M))
    km = None
    if mask:
        km = torch.zeros(B, N, dtype=torch.uint8)
        for b in range(B):   # ragged tails plus a few keys inside
            km[b, N - 1 - (37 * (b + 1)) % (N // 2):] = 1
            km[b, torch.randint(0, N // 2, (5,), generator=gen)] = 1
        km = km.to(DEV)
    return q, k, v, do, km


def _dense(q, k, v, B, M, N, km, dtype):
    """the dense formula under autograd in `dtype` -> (out (B*M,256), lse (B,8,M))"""
    h = lambda t, n: t.to(dtype).view(B, n, 8, 32).transpose(1, 2)   # noqa: E731
    s = h(q, M) @ h(k, N).transpose(-1, -2) / 32 ** 0.5
    if km is not None:
        s = s.masked_fill(km.bool()[:, None, None, :], float("-inf"))
    return (torch.softmax(s, -1) @ h(v, N)).transpose(1, 2).reshape(B * M, 256), torch.logsumexp(s, -1)


SHAPES = [(256, 256), (4096, 256), (256, 4096), (1000, 777)]


@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("M,N", SHAPES)
def test_attention_train_forward(M, N, mask):
    from deeppointmap_amd import ops
    B = 2
    q, k, v, _, km = _qkv(B, M, N, 5, mask)
    out, lse = ops.attention_train_forward(q, k, v, B, M, N, 8, km)
    want = ops.attention(q, k, v, B, M, N, 8, key_mask=km)
    torch.testing.assert_close(out, want, rtol=1e-4, atol=2e-5)       # the tolerance of test_attention_core_vs_torch
    o64, l64 = _dense(q, k, v, B, M, N, km, torch.float64)
    torch.testing.assert_close(out.cpu(), o64.float().cpu(), rtol=1e-4, atol=2e-5)
    assert_features_close(lse.cpu().numpy(), l64.cpu().numpy(), f"attention_train lse M={M} N={N} mask={mask}")
    # strided operands: column slices of one (rows, 768) buffer, as the module calls it
    if M == N:
        qkv = torch.cat([q, k, v], dim=1)
        o2, l2 = ops.attention_train_forward(qkv[:, :256], qkv[:, 256:512], qkv[:, 512:], B, M, N, 8, km)
        assert torch.equal(o2, out) and torch.equal(l2, lse)


@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("M,N", SHAPES)
def test_attention_train_backward(M, N, mask):
    from deeppointmap_amd import ops
    B = 2
    q, k, v, do, km = _qkv(B, M, N, 7, mask)
    runs = []
    for _ in range(2):
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
        with torch.enable_grad():
            out = ops.attention_train(*leaves, B, M, N, 8, km)
            runs.append(torch.autograd.grad(out, leaves, do))
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two runs differ"
    ref = {}
    for dtype in (torch.float32, torch.float64):
        leaves = [t.clone().to(dtype).requires_grad_(True) for t in (q, k, v)]
        with torch.enable_grad():
            out, _ = _dense(*leaves, B, M, N, km, dtype)
            ref[dtype] = [g.cpu().numpy() for g in torch.autograd.grad(out, leaves, do.to(dtype))]
    for name, got, r32, r64 in zip(("dq", "dk", "dv"), runs[0], ref[torch.float32], ref[torch.float64]):
        check(f"attention_train {name} M={M} N={N} mask={mask}", got.cpu().numpy(), r64, rel_err(r32, r64))
    if mask:
        dead = km.bool().reshape(-1)
        assert dead.any()
        assert not runs[0][1][dead].any() and not runs[0][2][dead].any(), "masked keys must get exactly zero dK and dV"
        assert runs[0][1][~dead].any()


def test_attention_train_errors():
    from deeppointmap_amd import ops
    q = torch.randn(64, 128, device=DEV)
    with pytest.raises(ValueError, match="32"):     # head width 16
        ops.attention_train(q, q, q, 1, 64, 64, 8)
    q = torch.randn(64, 256, device=DEV)
    with pytest.raises(ValueError):
        ops.attention_train(q, q[:32], q, 1, 64, 64, 8)
    with pytest.raises(ValueError):
        ops.attention_train(q, q, q, 1, 64, 64, 8, torch.zeros(1, 63, dtype=torch.uint8, device=DEV))
    with pytest.raises(TypeError):
        ops.attention_train(q, q, q, 1, 64, 64, 8, torch.zeros(1, 64, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError):
        ops.attention_train(q.double(), q.double(), q.double(), 1, 64, 64, 8)


# ---- Decoder.forward ---------------------------------------------------------------------------------------------------------

def _decoder(cfg):
    from deeppointmap_amd.decoder import Decoder
    dec = Decoder(cfg)
    dec.load_state_dict(C.state_dict(cfg), strict=True)
    return dec.to(DEV)


def _tensors(name):
    inputs, cfg = CASES[name]
    t = lambda a: None if a is None else torch.from_numpy(a).to(DEV) if a.dtype == bool else torch.from_numpy(a).to(DEV, torch.float32)   # noqa: E731
    return {k: t(v) for k, v in inputs.items()}, cfg


def hip_step(name, dec=None):
    """Decoder.forward -> RegistrationLoss -> backward() -> (outs, loss values, grad_src, grad_dst, {param: grad}, decoder)"""
    from deeppointmap_amd.loss import RegistrationLoss
    t, cfg = _tensors(name)
    dec = (dec or _decoder(cfg)).train()
    dec.zero_grad(set_to_none=True)
    src, dst = t["src"].clone().requires_grad_(True), t["dst"].clone().requires_grad_(True)
    ps, pd = (torch.from_numpy(m).to(DEV) for m in C.masks(CASES[name][0]))
    with torch.enable_grad():
        outs = dec(src, dst, t["ps"], t["pd"], (t["R"], t["T"]))
        xs_global = (t["R"] @ src[:, -3:] + t["T"]).detach()
        vals = RegistrationLoss(cfg)(xs_global, dst[:, -3:].detach(), ps, pd, *outs)
        vals[0].backward()
    return outs, vals, src.grad, dst.grad, {k: p.grad for k, p in dec.flat().items()}, dec


@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_outputs(name):
    from deeppointmap_amd import ops
    fx = C.load_fixture(name, GOLDEN)
    t, cfg = _tensors(name)
    dec = _decoder(cfg).train()
    with torch.enable_grad():
        outs = dec(t["src"], t["dst"], t["ps"], t["pd"], (t["R"], t["T"]))
    B, _, M = t["src"].shape
    N = t["dst"].shape[2]
    K = fx["pairs"].shape[0]
    E, Cc = C.MODEL_CHANNEL, C.IN_CHANNEL
    assert [tuple(o.shape) for o in outs] == [(B, E, M), (B, E, N), (B, Cc, M), (B, Cc, N), (K, 3, 1), (K, 3, 1)]
    assert all(o.requires_grad for o in outs)
    for k, o in zip(C.OUT_KEYS, outs):
        assert_features_close(o.detach().cpu().numpy(), fx[k + "/64"], f"decoder_train {name} {k}")
    # the pair list: exactly the reference's, every case
    ps, pd = (torch.from_numpy(m).to(DEV) for m in C.masks(CASES[name][0]))
    src_gt = (t["R"] @ t["src"][:, -3:] + t["T"]).contiguous()
    triples, off_a, off_b, perm_b = ops.offset_pairs(src_gt, t["dst"][:, -3:].contiguous(), ps, pd, cfg.loss.eps_offset)
    assert triples.dtype == torch.int32 and np.array_equal(triples.cpu().numpy(), fx["pairs"])
    tr = triples.long().cpu().numpy()
    assert np.array_equal(np.diff(off_a.cpu().numpy()), np.bincount(tr[:, 0] * M + tr[:, 1], minlength=B * M))
    assert np.array_equal(np.diff(off_b.cpu().numpy()), np.bincount(tr[:, 0] * N + tr[:, 2], minlength=B * N))
    key = (tr[:, 0] * N + tr[:, 2])[perm_b.cpu().numpy()]
    assert np.all(np.diff(key) >= 0) and np.all(np.diff(perm_b.cpu().numpy())[np.diff(key) == 0] > 0)   # sorted by target row, stable
    # the pairing features are the inference path's similarity-head features of the same descriptors
    dec.eval()
    x, _, y, _, _, _, _ = dec._descriptor_attention_forward(t["src"], t["dst"], t["ps"], t["pd"])
    for side, rows, o, n in (("src", x, outs[0], M), ("dst", y, outs[1], N)):
        a = dec._lin("similarity_head.2", dec._lin("similarity_head.0", rows, ops.ACT_RELU))
        assert_features_close(o.detach().transpose(1, 2).reshape(B * n, E).cpu().numpy(), a.cpu().numpy(),
                              f"decoder_train {name} {side}_pairing against the inference path")


@pytest.mark.parametrize("name", sorted(CASES))
def test_end_to_end_gradients(name):
    fx = C.load_fixture(name, GOLDEN)
    outs, vals, gs, gd, pg, dec = hip_step(name)
    outs2, vals2, gs2, gd2, pg2, _ = hip_step(name, dec)
    # bitwise repeatability of the loss and of every gradient
    assert torch.equal(vals[0], vals2[0]) and torch.equal(gs, gs2) and torch.equal(gd, gd2)
    for k in pg:
        if "loop" in k:
            assert pg[k] is None and pg2[k] is None, k
        else:
            assert pg[k] is not None and torch.equal(pg[k], pg2[k]), k
    nc = C.IN_CHANNEL
    l64, l32 = fx["loss/64"], fx["loss/32"]
    for i, what in ((0, "loss"), (2, "loss_p"), (3, "loss_c"), (4, "loss_o")):
        if l64[i] != 0:
            check(f"decoder_train {name} {what}", np.array([float(vals[i])]), l64[i:i + 1], abs(l32[i] - l64[i]) / abs(l64[i]))
        else:
            assert float(vals[i]) == 0.0, what
    for what, g in (("grad_src", gs), ("grad_dst", gd)):
        g = g.cpu().numpy()
        assert not g[:, nc:].any(), "the xyz rows get no gradient"
        check(f"decoder_train {name} {what}", g[:, :nc], fx[what + "/64"][:, :nc], rel_err(fx[what + "/32"][:, :nc], fx[what + "/64"][:, :nc]))
    # parameter gradients: the fixture's samples, maxima and norms, and the whole tensors against the fp64 restatement
    _, _, loss_r, gs_r, gd_r, pg_r = run_restated(name, torch.float64, DEV)
    assert abs(loss_r - l64[0]) <= 1e-9 * abs(l64[0])
    worst = 0.0
    for k, g in pg.items():
        if "loop" in k:
            continue
        key = f"pgrad/{k}"
        mx = float(fx[key + "/max"][1])
        if mx == 0.0:
            assert not g.any() and (pg_r[k] is None or not pg_r[k].any()), k
            continue
        g = g.cpu().numpy()
        e = float(np.asarray(fx[key + "/e"]).reshape(-1)[0])
        off = C.sample_offset(k)
        s_err = float(np.abs(g.reshape(-1)[off::C.SAMPLE_STRIDE] - fx[key + "/64"]).max()) / mx
        assert s_err <= max(3 * e, FLOOR), f"{k} (fixture sample): {s_err:.3e} (e {e:.2e})"
        worst = max(worst, check(f"decoder_train {name} d/d {k}", g, pg_r[k], e))
        norm = float(np.linalg.norm(g.astype(np.float64)))
        # a maximum-norm error of b x max moves the 2-norm by at most b x max x sqrt(size)
        assert abs(norm - fx[key + "/norm"][1]) <= max(3 * e, FLOOR) * mx * g.size ** 0.5, k
    print(f"decoder_train {name}: worst parameter gradient error {worst:.3e}")


def test_sgd_step_reaches_inference():
    """after an optimiser step the inference path (derived-weight caches, captured graphs) serves the new weights"""
    from deeppointmap_amd.decoder import Decoder
    from deeppointmap_amd.loss import RegistrationLoss
    name = "plain_256"
    t, cfg = _tensors(name)
    dec = _decoder(cfg)
    s, d = t["src"][0], t["dst"][0]
    assert not any(p.requires_grad for p in dec.parameters())
    before = [dec.registration_forward(s, d) for _ in range(4)][-1]     # derived tensors made, the shape's graph captured
    dec.train()
    assert all(p.requires_grad == ("loop" not in k) for k, p in dec.flat().items())
    opt = torch.optim.SGD([p for p in dec.parameters() if p.requires_grad], lr=1e-4)
    with torch.enable_grad():
        outs = dec(t["src"], t["dst"], None, None, (t["R"], t["T"]))
        ps, pd = (torch.from_numpy(m).to(DEV) for m in C.masks(CASES[name][0]))
        loss = RegistrationLoss(cfg)((t["R"] @ t["src"][:, -3:] + t["T"]), t["dst"][:, -3:], ps, pd, *outs)[0]
        loss.backward()
    opt.step()
    dec.eval()
    assert not any(p.requires_grad for p in dec.parameters())
    after = [dec.registration_forward(s, d) for _ in range(4)]
    fresh = Decoder(cfg)
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in dec.state_dict().items()}, strict=True)
    want = fresh.to(DEV).registration_forward(s, d)
    for got in after:
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]) and got[3] == want[3]
    assert all(torch.isfinite(x).all() for x in want[:3]) and all(torch.isfinite(x).all() for x in before[:3])
    assert not torch.equal(before[1], want[1]), "the step must have changed the weights"


def test_forward_argument_errors():
    from deeppointmap_amd.decoder import Decoder
    t, cfg = _tensors("three_layers")
    dec = _decoder(cfg)
    Rt = (t["R"], t["T"])
    with pytest.raises(AssertionError):   # eval mode, as the reference
        dec(t["src"], t["dst"], t["ps"], t["pd"], Rt)
    dec.train()
    with pytest.raises(AssertionError):
        dec(t["src"], t["dst"], t["ps"], t["pd"], None)
    with pytest.raises(ValueError):
        dec(t["src"][:, :130], t["dst"], t["ps"], t["pd"], Rt)
    with pytest.raises(ValueError):
        dec(t["src"], t["dst"].repeat(2, 1, 1), t["ps"], t["pd"], Rt)
    with pytest.raises(ValueError):
        dec(t["src"], t["dst"], t["ps"][:, :-1], t["pd"], Rt)
    with pytest.raises(ValueError):
        dec(t["src"], t["dst"], t["ps"].to(torch.uint8), t["pd"], Rt)
    with pytest.raises(ValueError):
        dec(t["src"], t["dst"], t["ps"], t["pd"], (t["R"][0], t["T"]))
    narrow = C.cfg()
    narrow.decoder.model_channel = 128
    small = Decoder(narrow).to(DEV).train()
    with pytest.raises(ValueError, match="32"):
        small(t["src"], t["dst"], t["ps"], t["pd"], Rt)


def test_peak_memory_below_one_probability_tensor():
    """forward + loss + backward at B = 2, M = N = 4096, three layers: the peak stays below what ONE (B, 8, M, N) fp32 tensor takes
    (1 GiB); autograd over the dense formulation keeps one per attention block."""
    import gc
    from deeppointmap_amd.loss import RegistrationLoss
    B, M, N = 2, 4096, 4096
    gc.collect()
    torch.cuda.synchronize()
    # what earlier tests of the same process still hold (session fixtures, captured graphs) is not this step's: everything
    # from here on is counted -- weights, inputs, BLAS workspaces -- which in a fresh process is max_memory_allocated itself
    base = torch.cuda.memory_allocated()
    cfg = C.cfg(layers=3)
    inputs = C._make(99, B, M, N, side=60.0)
    dec = _decoder(cfg).train()
    t = lambda a: torch.from_numpy(a).to(DEV, torch.float32)   # noqa: E731
    src, dst, Rg, Tg = t(inputs["src"]).requires_grad_(True), t(inputs["dst"]).requires_grad_(True), t(inputs["R"]), t(inputs["T"])
    ps, pd = (torch.from_numpy(m).to(DEV) for m in C.masks(inputs))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    with torch.enable_grad():
        outs = dec(src, dst, ps, pd, (Rg, Tg))
        loss = RegistrationLoss(cfg)((Rg @ src[:, -3:] + Tg).detach(), dst[:, -3:].detach(), ps, pd, *outs)[0]
        loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"decoder_train memory B={B} M={M} N={N} layers=3: peak {peak / 2 ** 20:.0f} MiB above {base / 2 ** 20:.0f} MiB held before, K {outs[4].shape[0]}, loss {float(loss):.4f}")
    assert torch.isfinite(loss) and outs[4].shape[0] > 0
    assert peak < B * 8 * M * N * 4
