"""GPU: Encoder / Decoder with set_train_dense("hip"): the training forwards with every dense layer in csrc/dense_train.hip.

The fixture cases run through the machinery of tests/test_gpu_decoder_train.py and tests/test_gpu_encoder_train.py (their helpers
are imported, their bounds apply: 1e-5 x scale for the features, max(3 e, FLOOR) with the fixtures' recorded e for loss and
gradients, the encoder's routes forced to the module's).  Then: no torch dense node is left in the graph, the switch goes back
to today's bytes, recomputation changes no byte, two steps give identical bytes, deepcopy keeps the mode and the loop-detection
stage still serves the inference bytes.
"""
import copy
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, assert_features_close

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_decoder_train as TD  # noqa: E402
import test_gpu_encoder_train as TE  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DENSE_NODES = ("AddmmBackward0", "MmBackward0", "NativeLayerNormBackward0")


def hip_decoder(name):
    return TD._decoder(TD.CASES[name][1]).set_train_dense("hip")


def hip_encoder(name):
    return TE._encoder(TE.C.cfg(name)).set_train_dense("hip")


def enc_step(name, enc):
    """Encoder.train().forward WITHOUT a trace (tracing turns the recomputation off) -> (fea, {param: grad}, the graph's root)"""
    pts, pad, G = TE.C.inputs(name)
    enc.train()
    enc.zero_grad(set_to_none=True)
    coor, fea, padding = enc(torch.from_numpy(pts), torch.from_numpy(pad))
    with torch.enable_grad():
        root = (fea * torch.from_numpy(G).to(DEV) * (~padding).unsqueeze(1)).sum()
        root.backward(retain_graph=True)
    return fea.detach(), {k: p.grad.clone() for k, p in enc.flat().items()}, root


def graph_nodes(root):
    """name -> count over every autograd node reachable from root.grad_fn"""
    seen, stack, names = set(), [root.grad_fn], {}
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names[type(fn).__name__] = names.get(type(fn).__name__, 0) + 1
        stack.extend(f for f, _ in fn.next_functions)
    return names


# ---- the fixture cases ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["plain_256", "no_pairs", "masks_ragged"])
def test_decoder_fixture_cases_in_hip_mode(name):
    C = TD.C
    fx = C.load_fixture(name, GOLDEN)
    outs, vals, gs, gd, pg, dec = TD.hip_step(name, hip_decoder(name))
    assert dec.train_dense == "hip"
    for k, o in zip(C.OUT_KEYS, outs):
        assert_features_close(o.detach().cpu().numpy(), fx[k + "/64"], f"dense_train decoder {name} {k}")
    l64, l32 = fx["loss/64"], fx["loss/32"]
    for i, what in ((0, "loss"), (2, "loss_p"), (3, "loss_c"), (4, "loss_o")):
        if l64[i] != 0:
            TD.check(f"dense_train decoder {name} {what}", np.array([float(vals[i])]), l64[i:i + 1], abs(l32[i] - l64[i]) / abs(l64[i]))
        else:
            assert float(vals[i]) == 0.0, what
    nc = C.IN_CHANNEL
    for what, g in (("grad_src", gs), ("grad_dst", gd)):
        g = g.cpu().numpy()
        assert not g[:, nc:].any(), "the xyz rows get no gradient"
        TD.check(f"dense_train decoder {name} {what}", g[:, :nc], fx[what + "/64"][:, :nc],
                 TD.rel_err(fx[what + "/32"][:, :nc], fx[what + "/64"][:, :nc]))
    _, _, _, _, _, pg_r = TD.run_restated(name, torch.float64, DEV)
    worst = 0.0
    for k, g in pg.items():
        if "loop" in k:
            assert g is None, k
            continue
        mx = float(fx[f"pgrad/{k}/max"][1])
        if mx == 0.0:
            assert not g.any(), k
            continue
        e = float(np.asarray(fx[f"pgrad/{k}/e"]).reshape(-1)[0])
        worst = max(worst, TD.check(f"dense_train decoder {name} d/d {k}", g.cpu().numpy(), pg_r[k], e))
    print(f"dense_train decoder {name}: worst parameter gradient error {worst:.3e}")
    # a second step from the same state: identical bytes
    _, vals2, gs2, gd2, pg2, _ = TD.hip_step(name, dec)
    assert torch.equal(vals[0], vals2[0]) and torch.equal(gs, gs2) and torch.equal(gd, gd2)
    assert all(torch.equal(pg[k], pg2[k]) for k in pg if pg[k] is not None)


@pytest.mark.parametrize("name", ["reduced_padded", "reduced_short"])
def test_encoder_fixture_cases_in_hip_mode(name):
    C = TE.C
    cfg = C.cfg(name)
    fix = C.load_fixture(name, GOLDEN)
    coor, fea, padding, grads, trace, enc = TE.hip_step(name, hip_encoder(name))
    assert enc.train_dense == "hip"
    valid = ~fix["padding"]
    assert np.array_equal(padding.cpu().numpy(), fix["padding"])
    assert_features_close(fea.cpu().numpy().transpose(0, 2, 1)[valid], fix["fea/64"].transpose(0, 2, 1)[valid],
                          f"dense_train encoder {name} fea vs fixture fp64")
    assert len(grads) == 110 and all(g is not None and torch.isfinite(g).all() for g in grads.values())
    geometry, winners = TE._module_geometry(cfg, trace)
    _, g64, _ = TE.run_restated(name, torch.float64, DEV, geometry, winners)
    worst = 0.0
    for k in g64:
        worst = max(worst, TE.check(f"dense_train encoder {name} d/d {k}", grads[k].cpu().numpy(), g64[k],
                                    float(np.ravel(fix[f"pgrad/{k}/e"])[0])))
    print(f"dense_train encoder {name}: worst parameter gradient error {worst:.3e}")
    _, fea2, _, grads2, _, _ = TE.hip_step(name, enc)
    assert torch.equal(fea, fea2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


# ---- no torch dense node left -------------------------------------------------------------------------------------------------

def test_graph_has_no_torch_dense_node():
    seen = {}
    for mode in ("torch", "hip"):
        outs, vals, *_ = TD.hip_step("plain_256", TD._decoder(TD.CASES["plain_256"][1]).set_train_dense(mode))
        seen["decoder", mode] = graph_nodes(vals[0])
        _, _, root = enc_step("reduced_padded", TE._encoder(TE.C.cfg("reduced_padded")).set_train_dense(mode))
        seen["encoder", mode] = graph_nodes(root)
    for module in ("decoder", "encoder"):
        t, h = seen[module, "torch"], seen[module, "hip"]
        # the walk sees the dense layers where they are torch's ...
        assert t.get("AddmmBackward0", 0) + t.get("MmBackward0", 0) > 0 and t.get("NativeLayerNormBackward0", 0) > 0, (module, t)
        assert not any("_DenseLinear" in k for k in t), (module, t)
        # ... and none where they are not
        assert not any(h.get(k, 0) for k in DENSE_NODES), (module, h)
        assert any("_DenseLinearBackward" in k for k in h) and any("_DenseLinearLNBackward" in k for k in h), (module, h)
    assert seen["decoder", "hip"].get("BmmBackward0", 0) == 0
    ups = TE.C.cfg("reduced_padded").encoder.upsample_layers
    assert seen["encoder", "hip"].get("BmmBackward0", 0) == seen["encoder", "torch"].get("BmmBackward0", 0) <= ups   # the interpolations


# ---- bytes -------------------------------------------------------------------------------------------------------------------

def test_switching_back_gives_todays_bytes():
    name = "plain_256"
    dec = hip_decoder(name)
    TD.hip_step(name, dec)
    outs, vals, gs, gd, pg, _ = TD.hip_step(name, dec.set_train_dense("torch"))
    outs0, vals0, gs0, gd0, pg0, _ = TD.hip_step(name)
    assert all(torch.equal(a, b) for a, b in zip(outs, outs0)) and torch.equal(vals[0], vals0[0])
    assert torch.equal(gs, gs0) and torch.equal(gd, gd0)
    assert all(torch.equal(pg[k], pg0[k]) for k in pg if pg0[k] is not None)
    name = "reduced_padded"
    enc = hip_encoder(name)
    enc_step(name, enc)
    fea, grads, _ = enc_step(name, enc.set_train_dense("torch"))
    fea0, grads0, _ = enc_step(name, TE._encoder(TE.C.cfg(name)))
    assert torch.equal(fea, fea0) and all(torch.equal(grads[k], grads0[k]) for k in grads)


def test_recomputation_changes_no_byte():
    name = "plain_256"
    outs0, vals0, gs0, gd0, pg0, _ = TD.hip_step(name, hip_decoder(name))
    dec = hip_decoder(name)
    dec.train_checkpoint_rows = 1
    outs, vals, gs, gd, pg, _ = TD.hip_step(name, dec)
    assert all(torch.equal(a, b) for a, b in zip(outs, outs0)) and torch.equal(vals[0], vals0[0])
    assert torch.equal(gs, gs0) and torch.equal(gd, gd0)
    assert all(torch.equal(pg[k], pg0[k]) for k in pg if pg0[k] is not None)
    name = "reduced_padded"
    enc = hip_encoder(name)
    fea0, grads0, _ = enc_step(name, enc)
    fea1, grads1, _ = enc_step(name, enc)                          # two steps from the same state
    assert torch.equal(fea0, fea1) and all(torch.equal(grads0[k], grads1[k]) for k in grads0)
    enc.train_checkpoint_rows = 1
    fea, grads, _ = enc_step(name, enc)
    assert torch.equal(fea, fea0) and all(torch.equal(grads[k], grads0[k]) for k in grads)


# ---- deepcopy and the stage switch -----------------------------------------------------------------------------------------------

def test_deepcopy_and_loop_detection_stage():
    name = "plain_256"
    t, cfg = TD._tensors(name)
    dec = hip_decoder(name)
    twin = copy.deepcopy(dec)
    assert twin.train_dense == "hip" and twin is not dec
    outs, vals, gs, gd, pg, _ = TD.hip_step(name, dec)
    outs2, vals2, gs2, gd2, pg2, _ = TD.hip_step(name, twin)
    assert torch.equal(vals[0], vals2[0]) and all(torch.equal(pg[k], pg2[k]) for k in pg if pg[k] is not None)
    # the frozen trunk of the loop-detection stage: the inference bytes, whatever the dense mode
    want = TD._decoder(cfg).loop_detection_forward(t["src"], t["dst"])
    dec.set_train_stage("loop_detection").train()
    assert torch.equal(dec.loop_detection_forward(t["src"], t["dst"]), want)
    with torch.enable_grad():
        prob = dec.loop_detection_forward(t["src"], t["dst"])
    assert prob.requires_grad
    np.testing.assert_allclose(prob.detach().cpu().numpy(), want.cpu().numpy(), atol=2e-5, rtol=0)   # the tolerance of test_gpu_loop_train
    ename = "reduced_padded"
    pts, pad, _ = (torch.from_numpy(a) for a in TE.C.inputs(ename))
    enc = hip_encoder(ename)
    assert copy.deepcopy(enc).train_dense == "hip"
    want = TE._encoder(TE.C.cfg(ename))(pts, pad)
    enc.set_train_stage("loop_detection").train()
    with torch.enable_grad():
        got = enc(pts, pad)
    assert not got[1].requires_grad and all(torch.equal(a, b) for a, b in zip(got, want))
