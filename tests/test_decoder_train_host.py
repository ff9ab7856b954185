"""CPU: the plain-torch restatement of the decoder's training step (tests/decoder_train_restated.py) against the reference's
recorded answers (tests/golden/decoder_train_<case>.partNN.npz): outputs, pair lists, loss, descriptor gradients and the
sampled parameter gradients, fp64 against fp64 and fp32 against fp32.  This pins the comparator the GPU tests use where the
reference does not exist.

Bounds, per tensor in the maximum norm relative to max |reference fp64|:
  fp64 against fp64: 1e-9.  Both are fp64 evaluations of one function in different operation orders (F.linear on rows against
    Conv1d on channels): rounding 1.1e-16 amplified by the sums (up to 512 terms) and three LayerNorm / softmax stages stays
    below 1e-12; the fixture restores the fp64 run from fp32 parts to ~1e-13.  1e-9 leaves three orders and still catches any
    wrong term (the smallest loss term weighs 1e-3 of a gradient).
  fp32 against fp32: 4 e + E.  e = max |reference fp32 - reference fp64| / max |reference fp64| of that tensor and E the
    largest e of the case's tensors (both recorded by the fixture): two fp32 evaluations in different orders each sit about e
    from the exact value, so they differ by up to ~2 e, and factor 2 on that for the tensors where the reference's own order
    happens to be the lucky one.  The per-tensor e of a small tensor is a poor estimate (offset_head.head.weight is sampled
    at 12 elements: its e is 1.2e-7, one ulp, where the gradients that feed it carry 3e-6), so no tensor is held tighter
    than the error the reference itself shows somewhere in the same step.
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_train_cases as C  # noqa: E402
import decoder_train_restated as R  # noqa: E402

CASES = C.cases()


def run_restated(name, dtype, device="cpu"):
    """-> (outs, pairs, loss, grad_src, grad_dst, {param: grad}) of the restatement, as numpy"""
    inputs, cfg = CASES[name]
    sd = {k: v.to(device=device, dtype=dtype).requires_grad_("loop" not in k) for k, v in C.state_dict(cfg).items()}
    t = lambda a: torch.from_numpy(a).to(device=device, dtype=dtype)   # noqa: E731
    src, dst = t(inputs["src"]).requires_grad_(True), t(inputs["dst"]).requires_grad_(True)
    ps, pd = (torch.from_numpy(m).to(device) for m in C.masks(inputs))
    with torch.enable_grad():
        loss, outs, pairs = R.training_step(sd, cfg, src, dst, ps, pd, t(inputs["R"]), t(inputs["T"]))
        loss.backward()
    n = lambda x: x.detach().cpu().numpy()   # noqa: E731
    return ([n(o) for o in outs], n(pairs), float(loss), n(src.grad), n(dst.grad),
            {k: (n(v.grad) if v.grad is not None else None) for k, v in sd.items()})


def rel_err(got, want):
    m = float(np.abs(want).max()) if want.size else 0.0
    if m == 0.0:
        return float(np.abs(got).max()) if got.size else 0.0
    return float(np.abs(got.astype(np.float64) - want).max()) / m


def e_of(fx, key):
    return rel_err(fx[key + "/32"], fx[key + "/64"])


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("prec", ["64", "32"])
def test_restatement_equals_reference(name, prec):
    fx = C.load_fixture(name, GOLDEN)
    dtype = torch.float64 if prec == "64" else torch.float32
    outs, pairs, loss, gs, gd, pg = run_restated(name, dtype)
    assert np.array_equal(pairs, fx["pairs"]), "pair list"
    nc = C.IN_CHANNEL
    checks = [(k, o, fx[f"{k}/{prec}"], e_of(fx, k)) for k, o in zip(C.OUT_KEYS, outs)]
    checks.append(("grad_src", gs[:, :nc], fx[f"grad_src/{prec}"][:, :nc], rel_err(fx["grad_src/32"][:, :nc], fx["grad_src/64"][:, :nc])))
    checks.append(("grad_dst", gd[:, :nc], fx[f"grad_dst/{prec}"][:, :nc], rel_err(fx["grad_dst/32"][:, :nc], fx["grad_dst/64"][:, :nc])))
    for k, g in pg.items():
        if "loop" in k:
            assert g is None, k
            continue
        off = C.sample_offset(k)
        key = f"pgrad/{k}"
        if fx[key + "/max"][1] == 0.0:   # the reference's gradient is exactly zero (the offset head when no pair exists)
            assert g is None or not g.any(), k
            continue
        s32, s64 = fx[key + "/32"], fx[key + "/64"]
        # sampled: errors relative to the whole tensor's maximum, as e is
        mx = fx[key + "/max"][1]
        checks.append((key, g.reshape(-1)[off::C.SAMPLE_STRIDE] / mx, fx[f"{key}/{prec}"] / mx, float(np.abs(s32 - s64).max() / mx)))
        norm = float(np.linalg.norm(g.astype(np.float64)))
        want = fx[key + "/norm"][0 if prec == "32" else 1]
        assert abs(norm - want) <= (1e-9 if prec == "64" else 1e-5) * want, (k, norm, want)
    lw = fx[f"loss/{prec}"]
    assert abs(loss - lw[0]) <= (1e-9 if prec == "64" else 4e-6) * abs(lw[0]), (loss, lw[0])
    worst = ("", 0.0, 0.0)
    e_case = max(c[3] for c in checks)
    for k, got, want, e in checks:
        assert got.shape == want.shape, (k, got.shape, want.shape)
        err = rel_err(got, want.astype(np.float64))
        bound = 1e-9 if prec == "64" else 4 * e + e_case
        if err / bound > worst[1]:
            worst = (k, err / bound, err)
        assert err <= bound, f"{k}: {err:.3e} > {bound:.3e} (e {e:.2e})"
    print(f"{name} fp{prec}: worst {worst[0]} at {worst[2]:.2e} = {worst[1]:.2f} of its bound")


def test_fixture_requirements():
    """what the fixture must provide: an unambiguous pair list in every case, one case with K >= 1000, a case with K = 0, one
    with a source token in many pairs and a target token in many pairs"""
    ks = {}
    for name, (inputs, cfg) in CASES.items():
        assert C.gap(inputs) > 1e-4, name
        fx = C.load_fixture(name, GOLDEN)
        ks[name] = fx["pairs"]
        for f in C.fixture_parts(name, GOLDEN):
            assert os.path.getsize(f) < (1 << 20), f
    assert max(p.shape[0] for p in ks.values()) >= 1000
    assert ks["no_pairs"].shape == (0, 3)
    hubs = ks["hubs"]
    assert np.bincount(hubs[:, 1]).max() >= 40 and np.bincount(hubs[:, 2]).max() >= 40
