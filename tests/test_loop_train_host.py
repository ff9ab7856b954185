"""CPU: the plain-torch restatement of one loop-detection training step (tests/loop_train_restated.py) against the reference's
recorded answers (tests/golden/loop_train_<case>.partNN.npz): probabilities, loss, metrics, the gradient of the loss with
respect to the probabilities and the eight loop_head gradients (five whole, three sampled), fp64 against fp64 and fp32 against
fp32.  This pins the comparator the GPU tests use where the reference does not exist.

Bounds, per tensor in the maximum norm relative to max |reference fp64|:
  fp64 against fp64: 1e-9 on every stored quantity.  Both are fp64 evaluations of one function in different operation orders:
    rounding 1.1e-16 amplified by sums of up to 512 terms and the LayerNorm / softmax stages of the trunk stays below 1e-12,
    and the fixture restores the fp64 run from fp32 parts to ~1e-13.
  fp32 against fp32: 4 e + E, as tests/test_decoder_train_host.py derives it (e the tensor's recorded
    |reference fp32 - reference fp64|, E the largest e of the case).
Metric values: equal.
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_train_cases as C  # noqa: E402
import loop_train_restated as R  # noqa: E402

CASES = C.cases()


def run_restated(name, dtype, device="cpu", sd=None):
    """-> (prob, loss, metrics, dprob, {param: grad or None}) of the restatement, as numpy"""
    inputs, cfg = CASES[name]
    if sd is None:
        sd = C.state_dict(cfg)
    sd = {k: v.detach().to(device=device, dtype=dtype).requires_grad_("loop" in k) for k, v in sd.items()}
    t = lambda a: torch.from_numpy(a).to(device=device, dtype=dtype)   # noqa: E731
    ps, pd = (torch.from_numpy(m).to(device) for m in C.masks(inputs))
    with torch.enable_grad():
        loss, prob, metrics = R.training_step(sd, cfg, t(inputs["src"]), t(inputs["dst"]), ps, pd, t(inputs["src_T"]),
                                              t(inputs["dst_T"]))
        prob.retain_grad()
        loss.backward()
    n = lambda x: x.detach().cpu().numpy()   # noqa: E731
    return n(prob), float(loss.detach()), metrics, n(prob.grad), {k: (n(v.grad) if v.grad is not None else None) for k, v in sd.items()}


def rel_err(got, want):
    m = float(np.abs(want).max()) if want.size else 0.0
    if m == 0.0:
        return float(np.abs(got).max()) if got.size else 0.0
    return float(np.abs(got.astype(np.float64) - want).max()) / m


def e_of(fx, key):
    return rel_err(fx[key + "/32"], fx[key + "/64"])


def fixture_checks(fx, prec, prob, dprob, pg):
    """[(key, got, want, e)] of everything the fixture stores about the gradients and the probabilities; sampled tensors are
    compared relative to the whole tensor's maximum, as their e is"""
    checks = [("prob", prob, fx[f"prob/{prec}"], e_of(fx, "prob")), ("grad/dprob", dprob, fx[f"grad/dprob/{prec}"], e_of(fx, "grad/dprob"))]
    for k in C.WHOLE:
        checks.append(("grad/" + k, pg[k], fx[f"grad/{k}/{prec}"], e_of(fx, "grad/" + k)))
    for k in C.SAMPLED:
        key, mx = f"pgrad/{k}", fx[f"pgrad/{k}/max"][1]
        checks.append((key, pg[k].reshape(-1)[C.sample_offset(k)::C.SAMPLE_STRIDE] / mx, fx[f"{key}/{prec}"] / mx, float(fx[key + "/e"].reshape(-1)[0])))
    return checks


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("prec", ["64", "32"])
def test_restatement_equals_reference(name, prec):
    fx = C.load_fixture(name, GOLDEN)
    prob, loss, metrics, dprob, pg = run_restated(name, torch.float64 if prec == "64" else torch.float32)
    for k, g in pg.items():
        assert (g is not None) == ("loop" in k), k
    want = fx[f"metrics/{prec}"]
    assert [metrics[k] for k in C.METRIC_KEYS[1:]] == list(want[1:]), (metrics, want)
    lw = fx[f"loss/{prec}"][0]
    assert abs(loss - lw) <= (1e-9 if prec == "64" else 4e-6) * abs(lw), (loss, lw)
    assert abs(metrics["loss_loop"] - want[0]) <= (1e-9 if prec == "64" else 4e-6) * abs(want[0])
    for k in C.SAMPLED:
        norm, nw = float(np.linalg.norm(pg[k].astype(np.float64))), fx[f"pgrad/{k}/norm"][0 if prec == "32" else 1]
        assert abs(norm - nw) <= (1e-9 if prec == "64" else 1e-5) * nw, (k, norm, nw)
        mx, mw = float(np.abs(pg[k]).max()), fx[f"pgrad/{k}/max"][0 if prec == "32" else 1]
        assert abs(mx - mw) <= (1e-9 if prec == "64" else 1e-5) * mw, (k, mx, mw)
    checks = fixture_checks(fx, prec, prob, dprob, pg)
    e_case = max(c[3] for c in checks)
    worst = ("", 0.0, 0.0)
    for k, got, w, e in checks:
        got = got.reshape(w.shape) if got.size == w.size else got
        assert got.shape == w.shape, (k, got.shape, w.shape)
        err = rel_err(got, w.astype(np.float64))
        bound = 1e-9 if prec == "64" else 4 * e + e_case
        if err / bound > worst[1]:
            worst = (k, err / bound, err)
        assert err <= bound, f"{k}: {err:.3e} > {bound:.3e} (e {e:.2e})"
    print(f"{name} fp{prec}: worst {worst[0]} at {worst[2]:.2e} = {worst[1]:.2f} of its bound")


def test_fixture_requirements():
    """what keeps the GPU tests meaningful: probabilities away from 0 and 1 (a saturated sigmoid has no gradient to check),
    labels that no rounding can flip, and the label mixes of the case table"""
    for name, (inputs, cfg) in CASES.items():
        assert C.gap(inputs) > 1e-4, name
        fx = C.load_fixture(name, GOLDEN)
        for k in ("prob/32", "prob/64"):
            assert (fx[k] > 0.05).all() and (fx[k] < 0.95).all(), (name, fx[k])
        assert np.array_equal(fx["labels"], inputs["labels"]), name
        for f in C.fixture_parts(name, GOLDEN):
            assert os.path.getsize(f) < (1 << 20), f
    lab = {n: CASES[n][0]["labels"] for n in CASES}
    assert lab["pairs_256"].sum() == 2 and (~lab["pairs_256"]).sum() == 2
    assert 0 < lab["ragged"].sum() < lab["ragged"].size
    assert not lab["all_negative"].any() and lab["all_positive"].all()
