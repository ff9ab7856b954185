"""GPU: the loop-detection training stage -- ops.loop_pool and ops.loop_bce (csrc/loop_head_train.hip), the stage switch of
Decoder / Encoder, Decoder.loop_detection_forward under autograd and LoopDetectionLoss, alone and through backward() and an
optimiser step.

References: the reference's recorded answers (tests/golden/loop_train_<case>.partNN.npz, fp32 and fp64 runs) and, for what the
fixture only samples, the plain-torch restatement run in fp64 on the device (tests/loop_train_restated.py, pinned to the
fixture by tests/test_loop_train_host.py).

Bounds.  Forward features: the project's rule (conftest.assert_features_close, 1e-5 x scale); probabilities: atol 2e-5, the
tolerance of test_gpu_decoder.py::test_loop_detection_vs_reference.  Every gradient, per tensor in the maximum norm relative
to max |fp64|: max(3 e, FLOOR), e = |reference fp32 - reference fp64| of that tensor (recorded by the fixture; for the
operator alone: dense fp32 torch autograd on the device against the same in fp64), factor 3 the margin the project grants over
the reference's own fp32 error (tests/test_gpu_margin.py, tests/test_gpu_decoder_train.py).  The floors were measured once on
the first GPU run by scripts/loop_train_accuracy.py, which uses nothing of the code under test (profiles/loop_train_accuracy.md
has the figures):
  FLOOR_OP   twice the worst error of the dense fp32 torch formulation of loop_pool against its fp64 run on the same x, over
             the shapes of test 1;
  FLOOR_E2E  twice the worst error, against the fixture's fp64 gradients, of the dense fp32 torch head fed with the features
             the eval-mode trunk returns (the inference kernels, pinned by the existing suites): it carries the trunk's
             bf16x3 arithmetic, which the fixture's fp32 reference run does not have.
ops.loop_bce: loss and dpred 1e-6 relative (fp32 elementwise formulas and a B-term sum); metrics equal.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, assert_features_close

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_train_cases as C  # noqa: E402
import loop_train_restated as R  # noqa: E402
from test_loop_train_host import fixture_checks, rel_err, run_restated  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = C.cases()
DEV = "cuda"
E = 256
FLOOR_OP = 7.6e-6    # 2 x 3.80e-6 (dense fp32 torch dW1 at B=2, L=4096): profiles/loop_train_accuracy.md
FLOOR_E2E = 2.9e-6   # 2 x 1.45e-6 (pairs_256, d/d loop_head.mlp.0.weight): profiles/loop_train_accuracy.md


def check(what, got, want64, e, floor):
    """max |got - want64| / max |want64| <= max(3 e, floor); asserted and logged by conftest's observed-error log"""
    got, want64 = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    m = float(np.abs(want64).max()) if want64.size else 0.0
    m = m if m > 0.0 else 1.0
    err = rel_err(got, want64)
    print(f"{what}: err {err:.3e}, e {e:.2e}, bound {max(3 * e, floor):.2e}")
    assert_features_close(got / m, want64 / m, f"{what} (e {e:.2e})", tol=max(3 * e, floor))
    return err


# ---- 1. the operator ----------------------------------------------------------------------------------------------------------

def pool_inputs(B, L, seed=3):
    """x (B*L, E), W1, b1, g; a few rows of x are zero and a few biases are zero: pre == 0 exactly there"""
    gen = torch.Generator().manual_seed(seed + 131 * L + B)
    x = torch.randn(B * L, E, generator=gen)
    W1 = torch.randn(E, E, generator=gen) / E ** 0.5
    b1 = 0.3 * torch.randn(E, generator=gen)
    g = torch.randn(B, E, generator=gen)
    b1[[5, 77, 200]] = 0.0
    x[:: max(1, (B * L) // 3)] = 0.0
    return [t.to(DEV) for t in (x, W1, b1, g)]


def dense_pool(x, W1, b1, g, B, L, dtype):
    """relu(x W1^T + b1).view(B, L, E).mean(1) under autograd in `dtype` -> (m, dW1, db1)"""
    x, g = x.to(dtype), g.to(dtype)
    W1, b1 = W1.to(dtype).requires_grad_(True), b1.to(dtype).requires_grad_(True)
    with torch.enable_grad():
        m = R.loop_pool(x.view(B, L, E), W1, b1)
        dW1, db1 = torch.autograd.grad(m, (W1, b1), g)
    return m.detach(), dW1, db1


def hip_pool(x, W1, b1, g, B, L):
    W1, b1 = W1.clone().requires_grad_(True), b1.clone().requires_grad_(True)
    from deeppointmap_amd import ops
    with torch.enable_grad():
        m = ops.loop_pool(x, B, L, W1, b1)
        dW1, db1 = torch.autograd.grad(m, (W1, b1), g)
    return m.detach(), dW1, db1


POOL_SHAPES = [(1, 1), (3, 17), (3, 250), (2, 1024), (2, 4096)]


@pytest.mark.parametrize("B,L", POOL_SHAPES)
def test_loop_pool_forward_and_backward(B, L):
    x, W1, b1, g = pool_inputs(B, L)
    m, dW1, db1 = hip_pool(x, W1, b1, g, B, L)
    m64, dW64, db64 = dense_pool(x, W1, b1, g, B, L, torch.float64)
    _, dW32, db32 = dense_pool(x, W1, b1, g, B, L, torch.float32)
    assert_features_close(m.cpu().numpy(), m64.cpu().numpy(), f"loop_pool forward B={B} L={L}")
    n = lambda t: t.cpu().numpy()   # noqa: E731
    check(f"loop_pool dW1 B={B} L={L}", n(dW1), n(dW64), rel_err(n(dW32), n(dW64)), FLOOR_OP)
    check(f"loop_pool db1 B={B} L={L}", n(db1), n(db64), rel_err(n(db32), n(db64)), FLOOR_OP)
    # the zero rows of x meet the zero biases at pre == 0 exactly: no contribution, as torch's relu has none there
    pre = F.linear(x.double(), W1.double(), b1.double())
    assert (pre == 0).sum() >= 3
    # a second run, and x as a column slice of a wider buffer: identical bytes
    m2, dW2, db2 = hip_pool(x, W1, b1, g, B, L)
    assert torch.equal(m, m2) and torch.equal(dW1, dW2) and torch.equal(db1, db2), "two runs differ"
    wide = torch.full((B * L, E + 8), 7.0, device=DEV)
    wide[:, 4:4 + E] = x
    m3, dW3, db3 = hip_pool(wide[:, 4:4 + E], W1, b1, g, B, L)
    assert torch.equal(m, m3) and torch.equal(dW1, dW3) and torch.equal(db1, db3), "strided x differs"


def test_loop_pool_pre_exactly_zero():
    """x = 0: pre = b1; the channels with b1 == 0 sit exactly on the ReLU's corner and must get nothing"""
    from deeppointmap_amd import ops
    B, L = 2, 70
    x = torch.zeros(B * L, E, device=DEV)
    W1 = torch.randn(E, E, device=DEV)
    b1 = torch.randn(E, device=DEV)
    b1[::4] = 0.0
    g = torch.randn(B, E, device=DEV).abs() + 0.1
    m = ops.loop_pool_forward(x, B, L, W1, b1)
    dW1, db1 = ops.loop_pool_backward(x, B, L, W1, b1, g)
    torch.testing.assert_close(m, torch.relu(b1).expand(B, E), rtol=1e-6, atol=0)
    assert not dW1.any()
    assert not db1[b1 <= 0].any() and (db1[b1 > 0] > 0).all()
    torch.testing.assert_close(db1[b1 > 0], g.sum(0)[b1 > 0], rtol=1e-5, atol=0)


def test_loop_pool_errors():
    from deeppointmap_amd import ops
    x = torch.randn(64, 128, device=DEV)
    with pytest.raises(ValueError, match="256"):     # E = 128
        ops.loop_pool(x, 1, 64, torch.randn(128, 128, device=DEV), torch.randn(128, device=DEV))
    x, W1, b1 = torch.randn(64, E, device=DEV), torch.randn(E, E, device=DEV), torch.randn(E, device=DEV)
    with pytest.raises(ValueError, match="rows"):
        ops.loop_pool(x, 2, 64, W1, b1)
    with pytest.raises(ValueError, match="B >= 1"):
        ops.loop_pool(x[:0], 0, 64, W1, b1)
    with pytest.raises(ValueError, match="W1"):
        ops.loop_pool(x, 1, 64, W1[:, :128], b1)
    with pytest.raises(ValueError, match="shape"):
        ops.loop_pool_backward(x, 1, 64, W1, b1, torch.randn(2, E, device=DEV))


# ---- 2. memory (derived, not measured) ------------------------------------------------------------------------------------------

def test_loop_pool_memory_does_not_grow_with_tokens():
    """Forward + backward at L = 8192 may take at most a quarter of ONE fp32 (B * 7168, E) tensor more than at L = 1024: a
    stored pre-activation or ReLU output, or a workspace proportional to the rows, would take a whole one or more.  What does
    grow is the forward's per-tile column sums: B * (7168 / 64) * E floats, 1/64 of that tensor."""
    B, Lmax = 2, 8192
    x, W1, b1, g = pool_inputs(B, Lmax)
    peak = {}
    for L in (1024, 1024, 8192):           # the first round warms up (library, allocator pools)
        xs = x[:B * L]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        m, dW1, db1 = hip_pool(xs, W1, b1, g, B, L)
        torch.cuda.synchronize()
        peak[L] = torch.cuda.max_memory_allocated() - base
        del m, dW1, db1
    growth, limit = peak[8192] - peak[1024], 0.25 * 4 * B * 7168 * E
    print(f"loop_pool peak: L=1024 {peak[1024]} B, L=8192 {peak[8192]} B, growth {growth} B, limit {limit:.0f} B")
    assert growth < limit


# ---- 3. the loss --------------------------------------------------------------------------------------------------------------

BATCHES = {
    "mixed": ([0.2, 0.7, 0.55, 0.4, 0.9], [0, 1, 0, 1, 1]),
    "saturated": ([0.0, 1.0, 0.0, 1.0, 0.3], [0, 1, 1, 0, 1]),      # the -100 clamp and the 1e-12 guard
    "no_positive": ([0.2, 0.7, 0.6], [0, 0, 0]),
    "no_negative": ([0.2, 0.7, 0.6], [1, 1, 1]),
    "one": ([0.8], [1]),
    "half": ([0.5, 0.5, 0.6], [1, 0, 1]),                            # exactly 0.5 is not a positive prediction
}


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_loop_bce_and_loss_module(name):
    from deeppointmap_amd import ops
    from deeppointmap_amd.loss import LoopDetectionLoss
    p, y = (torch.tensor(v, dtype=torch.float32, device=DEV) for v in BATCHES[name])
    grad = torch.tensor(1.7, device=DEV)
    with torch.enable_grad():
        pr = p.clone().requires_grad_(True)
        want = F.binary_cross_entropy(pr, y)
        dwant, = torch.autograd.grad(want, pr, grad)
        ph = p.clone().requires_grad_(True)
        loss, stats = ops.loop_bce(ph, y)
        assert not stats.requires_grad and loss.dim() == 0
        dgot, = torch.autograd.grad(loss, ph, grad)
    torch.testing.assert_close(loss, want.detach(), rtol=1e-6, atol=0)
    torch.testing.assert_close(dgot, dwant, rtol=1e-6, atol=0)
    gt = y.bool()
    _, mwant = R.loop_loss(p, gt)
    hit = p > 0.5
    counts = [float(gt.sum()), float((~gt).sum()), float((hit == gt).sum()), float((hit & gt).sum()), float((hit & ~gt).sum()), 0.0, 0.0]
    assert stats.tolist()[1:] == counts and stats[0] == loss
    # the module: labels from the frame positions, the reference's metric keys
    cfg = C.cfg()
    src_T = torch.zeros(len(y), 3, 1, device=DEV)
    dst_T = torch.zeros(len(y), 3, 1, device=DEV)
    dst_T[:, 1, 0] = torch.where(gt, 3.0, 30.0)
    with torch.enable_grad():
        ph = p.clone().requires_grad_(True)
        l2, metrics = LoopDetectionLoss(cfg)(ph, src_T, dst_T)
        l2.backward()
    assert torch.equal(l2.detach(), loss.detach())
    torch.testing.assert_close(ph.grad * 1.7, dgot, rtol=1e-6, atol=0)
    assert sorted(metrics) == sorted(C.METRIC_KEYS)
    assert [metrics[k] for k in C.METRIC_KEYS[1:]] == [mwant[k] for k in C.METRIC_KEYS[1:]], (metrics, mwant)
    assert metrics["loss_loop"] == float(loss)
    with pytest.raises(ValueError):
        LoopDetectionLoss(cfg)(ph, src_T[:, :, 0], dst_T)


# ---- 4. the module ------------------------------------------------------------------------------------------------------------

def make_decoder(cfg, sd=None):
    from deeppointmap_amd.decoder import Decoder
    dec = Decoder(cfg)
    dec.load_state_dict(C.state_dict(cfg) if sd is None else sd, strict=True)
    return dec.to(DEV)


def hip_step(name, dec):
    """one stage-two step -> (prob, loss, metrics, {param: grad or None})"""
    from deeppointmap_amd.loss import LoopDetectionLoss
    inputs, cfg = CASES[name]
    t = lambda a: torch.from_numpy(a).float().to(DEV)   # noqa: E731
    ps, pd = (None, None) if inputs["ps"] is None else (torch.from_numpy(m).to(DEV) for m in C.masks(inputs))
    dec.zero_grad(set_to_none=True)
    with torch.enable_grad():
        prob = dec.loop_detection_forward(t(inputs["src"]), t(inputs["dst"]), ps, pd)
        loss, metrics = LoopDetectionLoss(cfg)(prob, t(inputs["src_T"]), t(inputs["dst_T"]))
        loss.backward()
    return prob.detach(), loss.detach(), metrics, {k: (None if p.grad is None else p.grad.clone()) for k, p in dec.flat().items()}


@pytest.fixture(scope="module")
def restated64():
    """the fp64 restatement on the device, once per case"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = run_restated(name, torch.float64, device=DEV)
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(CASES))
def test_stage_two_step(name, restated64):
    inputs, cfg = CASES[name]
    fx = C.load_fixture(name, GOLDEN)
    dec = make_decoder(cfg)
    t = lambda a: torch.from_numpy(a).float().to(DEV)   # noqa: E731
    ps, pd = (None, None) if inputs["ps"] is None else (torch.from_numpy(m).to(DEV) for m in C.masks(inputs))
    p_eval = dec.loop_detection_forward(t(inputs["src"]), t(inputs["dst"]), ps, pd)
    assert dec.set_train_stage("loop_detection") is dec and not dec.training
    dec.train()
    assert sorted(k for k, p in dec.flat().items() if p.requires_grad) == sorted(C.HEAD)
    prob, loss, metrics, grads = hip_step(name, dec)
    assert tuple(prob.shape) == (inputs["src"].shape[0],)
    np.testing.assert_allclose(prob.cpu().numpy(), fx["prob/64"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(prob.cpu().numpy(), p_eval.cpu().numpy(), atol=2e-5, rtol=0)
    # grad mode off in .train(): today's inference path, identical bytes
    assert torch.equal(dec.loop_detection_forward(t(inputs["src"]), t(inputs["dst"]), ps, pd), p_eval)
    assert [metrics[k] for k in C.METRIC_KEYS[1:]] == list(fx["metrics/64"][1:])
    for k, g in grads.items():
        assert (g is not None) == ("loop" in k), k
    pg = {k: g.cpu().numpy() for k, g in grads.items() if g is not None}
    e_loss = abs(fx["loss/32"][0] - fx["loss/64"][0]) / abs(fx["loss/64"][0])
    check(f"{name} loss", [float(loss)], fx["loss/64"], e_loss, FLOOR_E2E)
    assert abs(metrics["loss_loop"] - float(loss)) == 0.0
    dprob = np.zeros_like(fx["grad/dprob/64"])   # not a parameter: checked through the eight that follow from it
    for k, got, want, e in fixture_checks(fx, "64", prob.cpu().numpy(), dprob, pg):
        if k in ("prob", "grad/dprob"):
            continue
        check(f"{name} {k}", got.reshape(want.shape), want, e, FLOOR_E2E)
    # the whole tensors against the fp64 restatement on the device
    _, _, _, _, pg64 = restated64(name)
    for k in C.HEAD:
        e = float(fx[f"pgrad/{k}/e"].reshape(-1)[0]) if k in C.SAMPLED else rel_err(fx[f"grad/{k}/32"], fx[f"grad/{k}/64"])
        check(f"{name} {k} (restated fp64)", pg[k], pg64[k].reshape(pg[k].shape), e, FLOOR_E2E)
    prob2, loss2, _, grads2 = hip_step(name, dec)
    assert torch.equal(prob, prob2) and torch.equal(loss, loss2)
    assert all(torch.equal(grads[k], grads2[k]) for k in C.HEAD), "two runs differ"


# ---- 5. one optimiser step ----------------------------------------------------------------------------------------------------

def test_sgd_step_is_seen_by_inference():
    name = "ragged"
    inputs, cfg = CASES[name]
    dec = make_decoder(cfg)
    t = lambda a: torch.from_numpy(a).float().to(DEV)   # noqa: E731
    ps, pd = (torch.from_numpy(m).to(DEV) for m in C.masks(inputs))
    before = dec.loop_detection_forward(t(inputs["src"]), t(inputs["dst"]), ps, pd)
    dec.set_train_stage("loop_detection").train()
    hip_step(name, dec)
    frozen = {k: p.detach().clone() for k, p in dec.flat().items() if "loop" not in k}
    torch.optim.SGD([p for p in dec.parameters() if p.requires_grad], lr=0.05).step()
    dec.eval()
    assert not any(p.requires_grad for p in dec.parameters()) and dec.train_stage == "loop_detection"
    assert all(torch.equal(frozen[k], dec.flat()[k]) for k in frozen)
    after = dec.loop_detection_forward(t(inputs["src"]), t(inputs["dst"]), ps, pd)
    assert float((after - before).abs().max()) > 1e-3, "the step must move the probabilities"
    sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    want = run_restated(name, torch.float64, device=DEV, sd=sd)[0]
    np.testing.assert_allclose(after.cpu().numpy(), want, atol=2e-5, rtol=0)


# ---- 6. the stage switch ------------------------------------------------------------------------------------------------------

def test_stage_switch():
    from deeppointmap_amd import synthetic
    from deeppointmap_amd.config import reduced_args
    from deeppointmap_amd.encoder import Encoder
    from deeppointmap_amd.weights import init_procedural
    dec = make_decoder(C.cfg())
    assert dec.train_stage == "registration"
    dec.train()
    assert all(p.requires_grad == ("loop" not in k) for k, p in dec.flat().items())      # the default stage: as before
    dec.set_train_stage("loop_detection")                                                # applied at once while training
    assert all(p.requires_grad == ("loop" in k) for k, p in dec.flat().items())
    dec.eval().train()                                                                   # sticky
    assert all(p.requires_grad == ("loop" in k) for k, p in dec.flat().items())
    dec.set_train_stage("registration")
    assert all(p.requires_grad == ("loop" not in k) for k, p in dec.flat().items())
    with pytest.raises(ValueError, match="stage"):
        dec.set_train_stage("loop")
    enc = init_procedural(Encoder(reduced_args())).to(DEV)
    with pytest.raises(ValueError, match="stage"):
        enc.set_train_stage("loops")
    N = 2048
    base = synthetic.base_cloud(N, seed=6)
    pts = torch.stack([synthetic.frame(f, N, base) for f in (0, 3)]).float()
    pad = torch.zeros(2, N, dtype=torch.bool)
    want = enc(pts, pad)
    assert enc.train_stage == "registration"
    enc.train()
    assert all(p.requires_grad for p in enc.parameters())                                # the default stage: as before
    assert enc.set_train_stage("loop_detection") is enc
    assert enc.training and not any(p.requires_grad for p in enc.parameters())
    with torch.enable_grad():
        got = enc(pts, pad)
        samp = enc.presample(pts, pad)
        again = enc(pts, pad, presampled=samp)                                           # inference-only arguments are accepted
    assert not got[1].requires_grad
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and all(torch.equal(a, b) for a, b in zip(again, want))
    enc.set_train_stage("registration")
    assert all(p.requires_grad for p in enc.parameters())
    fea = enc(pts, pad)[1]
    assert fea.requires_grad, "back in the registration stage .train() runs the training forward"
    enc.eval()
    assert all(torch.equal(a, b) for a, b in zip(enc(pts, pad), want))
