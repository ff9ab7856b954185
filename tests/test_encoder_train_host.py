"""CPU: the plain-torch restatement of the encoder's training forward (tests/encoder_train_restated.py) against the reference's
recorded answers (tests/golden/encoder_train_<case>.partNN.npz: fp32 and fp64 runs of the reference Encoder in .train() mode).
This pins the restatement, which the GPU tests then run in fp64 on the device with the module's routes forced.

Bound, per tensor in the maximum norm relative to max |fp64 run|: max(3 e, FLOOR), e = |reference fp32 - reference fp64| of that
tensor (recorded by the fixture), FLOOR as derived in tests/test_gpu_encoder_train.py.  The routes (which neighbour point wins
each max) must equal the fixture's wherever the fixture's two runs agree."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_train_cases as C  # noqa: E402
import encoder_train_restated as R  # noqa: E402

# Twice the worst error, over the fixture cases, of the dense fp32 torch restatement on the MI355X against the fp64 one with
# equal routes: an independent fp32 evaluation of the same function.  Measured 1.666e-6 (reduced_padded), 1.657e-6
# (default_8192), 1.651e-6 (reduced_short), each the worst of the 110 gradients (profiles/encoder_train_accuracy.md).
FLOOR = 3.4e-6


def rel_err(got, want64):
    got, want64 = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    m = float(np.abs(want64).max()) if want64.size else 0.0
    return float(np.abs(got - want64).max() / m) if m > 0 else float(np.abs(got).max() if got.size else 0.0)


def fixture_geometry(fix, cfg, device):
    n = len(cfg.encoder.npoint)
    level_xyz = [torch.from_numpy(fix[f"level_xyz/{i}"]).to(device) for i in range(n)]
    level_len = [torch.from_numpy(fix[f"level_len/{i}"]).to(device) for i in range(n)]
    idx = {name: torch.from_numpy(fix[f"idx/{name}"].astype(np.int64)).to(device) for name, *_ in R.layer_names(cfg)}
    return level_xyz, level_len, idx


def run_restated(name, dtype, device="cpu", geometry=None, winners=None, fix=None):
    """the restatement on a fixture case -> (fea (B,C,S) ndarray, {param: gradient ndarray}, {layer: winning points ndarray});
    geometry = (level_xyz, level_len, idx) on `device` (default: the fixture's), winners {layer: (B,S,C) tensor} forces routes"""
    cfg = C.cfg(name)
    pts, pad, G = C.inputs(name)
    if geometry is None:
        geometry = fixture_geometry(fix if fix is not None else C.load_fixture(name, GOLDEN), cfg, device)
    level_xyz, level_len, idx = geometry
    sd = {k: v.to(device=device, dtype=dtype).requires_grad_(True) for k, v in C.state_dict(cfg).items()}
    xyz = torch.from_numpy(pts).to(device).transpose(1, 2).contiguous()
    n_up = cfg.encoder.upsample_layers
    out_len = level_len[len(level_len) - n_up - 1]
    with torch.enable_grad():
        fea, routes = R.encoder_train_restated(cfg, sd, xyz, level_xyz, level_len, idx, winners)
        live = (torch.arange(fea.shape[1], device=device).unsqueeze(0) < out_len.unsqueeze(1)).unsqueeze(2)
        g = torch.from_numpy(G).to(device=device, dtype=dtype).transpose(1, 2)
        (fea * g * live).sum().backward()
    grads = {k: v.grad.detach().cpu().numpy() for k, v in sd.items()}
    return (fea.detach().transpose(1, 2).cpu().numpy(), grads, {k: v.cpu().numpy() for k, v in routes.items()})


def grad_bound_check(name, fix, grads, what, floor=FLOOR):
    """every parameter gradient (the fixture's whole tensor or strided sample) against the fp64 run -> worst error / bound"""
    worst = 0.0
    for key, g in grads.items():
        want = fix[f"pgrad/{key}/64"]
        got = C.grad_sample(key, g)
        m = float(fix[f"pgrad/{key}/max"][1])
        err = float(np.abs(got.astype(np.float64) - want).max() / m)
        bound = max(3 * float(np.ravel(fix[f"pgrad/{key}/e"])[0]), floor)
        assert err <= bound, f"{name} {what} d/d {key}: {err:.3e} > {bound:.3e}"
        worst = max(worst, err / bound)
    return worst


@pytest.mark.parametrize("name", list(C.CASES))
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_restatement_matches_the_reference(name, dtype):
    fix = C.load_fixture(name, GOLDEN)
    fea, grads, routes = run_restated(name, dtype, fix=fix)
    assert len(grads) == 110
    e = rel_err(fix["fea/32"], fix["fea/64"])
    err = rel_err(fea, fix["fea/64"])
    assert err <= max(3 * e, FLOOR), f"{name} fea: {err:.3e} > max(3 x {e:.2e}, {FLOOR:.1e})"
    tag = "64" if dtype == torch.float64 else "32"
    for layer, pts in routes.items():
        agree = fix[f"win/{layer}/32"] == fix[f"win/{layer}/64"]
        assert np.array_equal(pts[agree], fix[f"win/{layer}/{tag}"].astype(np.int64)[agree]), f"{name} {layer}: routes differ"
    grad_bound_check(name, fix, grads, f"restated fp{tag}")


def test_forced_routes_reproduce_the_free_run():
    """the gather at given winners is the max wherever the winners are the argmax: same outputs, same gradients"""
    name = "reduced_padded"
    fix = C.load_fixture(name, GOLDEN)
    fea, grads, routes = run_restated(name, torch.float64, fix=fix)
    forced = {k: torch.from_numpy(v) for k, v in routes.items()}
    fea2, grads2, _ = run_restated(name, torch.float64, winners=forced, fix=fix)
    assert np.array_equal(fea, fea2)
    for k in grads:
        assert rel_err(grads2[k], grads[k]) <= 1e-12, k
