"""GPU: the encoder's training forward (Encoder.forward in .train() mode) and its grouping operator (csrc/group_train.hip), alone
and through Decoder.forward, RegistrationLoss and backward().

References: the reference's recorded answers (tests/golden/encoder_train_<case>.partNN.npz, fp32 and fp64 runs) and the
plain-torch restatement run in fp64 on the device (tests/encoder_train_restated.py, pinned to the fixture by
tests/test_encoder_train_host.py) with the routes -- which neighbour point wins each max -- forced to the kernel's, so that two
implementations are compared on the same piecewise-smooth branch.

Bounds.  Forward features: the project's rule (conftest.assert_features_close, 1e-5 x scale).  Routes: the fp64 value at the
chosen neighbour within FEATURE_TOL x max(1, |max|) of the fp64 maximum, and at most 1e-3 of the live maxima won by another
point than the fp64 argmax (the reference's own fp32 run: 0 to 5.8e-5 on the fixture inputs).  Every gradient, per tensor in the
maximum norm relative to max |fp64|: max(3 e, FLOOR), e = the error of an independent fp32 evaluation of that tensor (operator:
the dense fp32 restatement on the device against the same fp64 run; module: |reference fp32 - reference fp64| recorded by the
fixture), factor 3 the margin the project grants over the reference's own fp32 error (tests/test_gpu_margin.py), and FLOOR
(tests/test_encoder_train_host.py) twice the worst error of the dense fp32 restatement on the device against the fp64 one with
equal routes over the fixture cases, measured on the first GPU run (profiles/encoder_train_accuracy.md has every figure; each
run prints what it observes and appends it to bench_out/encoder_train_accuracy.log).
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import FEATURE_TOL, GOLDEN, ROOT, assert_features_close

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_train_cases as C  # noqa: E402
import encoder_train_restated as R  # noqa: E402
from test_encoder_train_host import FLOOR, rel_err, run_restated  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX_ROUTE_SHARE = 1e-3


def note(line):
    print(line)
    try:
        os.makedirs(os.path.join(ROOT, "bench_out"), exist_ok=True)
        with open(os.path.join(ROOT, "bench_out", "encoder_train_accuracy.log"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def check(what, got, want64, e):
    got, want64 = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    m = float(np.abs(want64).max()) if want64.size else 0.0
    m = m if m > 0.0 else 1.0
    err = float(np.abs(got - want64).max() / m)
    bound = max(3 * e, FLOOR)
    note(f"{what}: err {err:.3e}, e {e:.3e}, bound {bound:.3e}")
    assert err <= bound, f"{what}: {err:.3e} > max(3 x {e:.2e}, {FLOOR:.1e})"
    return err


# ---- the grouping operator -------------------------------------------------------------------------------------------------

def _layer_inputs(Cout, K, seed=3, B=2, N=2048, S=512, lens=(2048, 1400), radius=0.1):
    """ragged frames, FPS centres (the second frame runs out of points: padded centre rows), a hybrid neighbour query"""
    from deeppointmap_amd import ops, synthetic
    gen = torch.Generator().manual_seed(seed + Cout + K)
    base = synthetic.base_cloud(N, seed=seed)
    pts = torch.stack([synthetic.frame(2 * b, N, base) for b in range(B)]).float()
    pad = torch.zeros(B, N, dtype=torch.bool)
    for b, n in enumerate(lens):
        pad[b, n:] = True
        pts[b][:, n:] = 0.0
    xyz, lengths = ops.prepare_points(pts.to(DEV).contiguous(), pad.to(DEV))
    _, centers, _ = ops.fps(xyz, lengths, S)
    idx = ops.knn_hybrid(xyz, lengths, centers, K, radius)
    Cin = Cout // 2
    fea = torch.randn(B, N, Cin, generator=gen).to(DEV)
    W = (torch.randn(Cout, Cin + 3, generator=gen) / (Cin + 3) ** 0.5).to(DEV)
    bias = (0.1 * torch.randn(Cout, generator=gen)).to(DEV)
    gamma = (1 + 0.2 * torch.randn(Cout, generator=gen)).to(DEV)
    gamma[::7] *= -1                                   # both signs
    beta = (0.2 * torch.randn(Cout, generator=gen)).to(DEV)
    dout = torch.randn(B, S, Cout, generator=gen).to(DEV)
    return dict(xyz=xyz, lengths=lengths, centers=centers, idx=idx, fea=fea, W=W, bias=bias, gamma=gamma, beta=beta, dout=dout,
                radius=radius, Cin=Cin)


SHIPPED = [(32, 32), (64, 32), (128, 32), (256, 32), (512, 16), (32, 16), (512, 32)]


@pytest.mark.parametrize("Cout,K", SHIPPED)
def test_group_train_forward(Cout, K):
    from deeppointmap_amd import ops
    t = _layer_inputs(Cout, K)
    Cin = t["Cin"]
    P = torch.nn.functional.linear(t["fea"], t["W"][:, :Cin].contiguous(), t["bias"]).contiguous()
    out, slots = ops.group_train_forward(P, t["xyz"], t["centers"], t["idx"], t["W"][:, Cin:].contiguous(), t["gamma"], t["beta"],
                                         t["radius"])
    want = ops.group_mlp_max(t["xyz"], t["fea"], t["centers"], t["idx"], t["W"], t["bias"], t["gamma"], t["beta"], t["radius"],
                             generic=True)
    assert_features_close(out.cpu().numpy(), want.cpu().numpy(), f"group_train forward Cout={Cout} K={K}")
    # routes against the dense fp64 restatement
    d = lambda x: x.double()   # noqa: E731
    max64, pts64, y64 = R.group_layer(d(t["xyz"]), d(t["fea"]), d(t["centers"]), t["idx"], d(t["W"]), d(t["bias"]), d(t["gamma"]),
                                      d(t["beta"]), t["radius"])
    live_k = slots != ops.GROUP_TRAIN_NO_WINNER
    at = torch.gather(y64, 2, slots.long().clamp(max=K - 1).unsqueeze(2)).squeeze(2)
    at = torch.where(live_k, at, torch.zeros_like(at))
    gap = ((max64 - at) / max64.abs().clamp(min=1.0)).max().item()
    assert gap <= FEATURE_TOL, f"a chosen neighbour is {gap:.2e} below the fp64 maximum"
    win = ops.group_train_winners(t["idx"], slots)
    live = max64 > 0
    share = ((win != pts64) & live).sum().item() / max(live.sum().item(), 1)
    note(f"group_train forward Cout={Cout} K={K}: routes differing from the fp64 argmax {share:.2e} of {int(live.sum())} live maxima, "
         f"largest gap to the fp64 maximum {gap:.2e}")
    assert share <= MAX_ROUTE_SHARE


@pytest.mark.parametrize("Cout,K", SHIPPED)
def test_group_train_backward(Cout, K):
    from deeppointmap_amd import ops
    t = _layer_inputs(Cout, K, seed=5)
    Cin = t["Cin"]
    P0 = torch.nn.functional.linear(t["fea"], t["W"][:, :Cin].contiguous(), t["bias"]).contiguous()
    Wr0 = t["W"][:, Cin:].contiguous()
    runs = []
    for _ in range(2):
        leaves = [x.clone().requires_grad_(True) for x in (P0, Wr0, t["gamma"], t["beta"])]
        keep = []
        with torch.enable_grad():
            out = ops.group_train(leaves[0], t["xyz"], t["centers"], t["idx"], leaves[1], leaves[2], leaves[3], t["radius"],
                                  layer="test", keep_slots=keep)
            runs.append(torch.autograd.grad(out, leaves, t["dout"]) + (out.detach(), keep[0]))
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two runs differ"
    dP, dWr, dg, db, out, slots = runs[0]
    win = ops.group_train_winners(t["idx"], slots)
    # the dense restatement with the kernel's routes: features = P itself through [I | W_rel], so that d/d fea is dP
    ref = {}
    for dt in (torch.float64, torch.float32):
        leaves = [x.detach().to(dt).requires_grad_(True) for x in (P0, Wr0, t["gamma"], t["beta"])]
        with torch.enable_grad():
            W = torch.cat([torch.eye(Cout, device=DEV, dtype=dt), leaves[1]], dim=1)
            o, _, _ = R.group_layer(t["xyz"].to(dt), leaves[0], t["centers"].to(dt), t["idx"], W, torch.zeros(Cout, device=DEV, dtype=dt),
                                    leaves[2], leaves[3], t["radius"], winners=win)
            ref[dt] = [g.cpu().numpy() for g in torch.autograd.grad(o, leaves, t["dout"].to(dt))] + [o.detach().cpu().numpy()]
    assert_features_close(out.cpu().numpy(), ref[torch.float64][4], f"group_train out vs forced fp64 Cout={Cout} K={K}")
    for name, got, w64, w32 in zip(("dP", "dW_rel", "dgamma", "dbeta"), (dP, dWr, dg, db), ref[torch.float64], ref[torch.float32]):
        check(f"group_train backward Cout={Cout} K={K} {name}", got.cpu().numpy(), w64, rel_err(w32, w64))
    # rows of dP that no winning neighbour names -- padding points among them -- are exact zeros
    named = torch.zeros(dP.shape[0], dP.shape[1], dtype=torch.bool, device=DEV)
    rows = torch.arange(dP.shape[0], device=DEV).view(-1, 1, 1).expand_as(win)
    named[rows[win >= 0], win[win >= 0]] = True
    assert not named[torch.arange(dP.shape[1], device=DEV).unsqueeze(0) >= t["lengths"].unsqueeze(1)].any()
    assert (dP[~named] == 0).all() and int((~named).sum()) > 0
    assert bool((dP[named].abs().sum(-1) > 0).any())


def test_group_train_peak_memory():
    """forward + backward at B = 4, N = 16 384, S = 4096, K = 32, Cout = 32 stay below half of one (B,S,K,Cout) fp32 tensor
    (32 MiB) on top of the inputs"""
    from deeppointmap_amd import ops
    B, N, S, K, Cout = 4, 16384, 4096, 32, 32
    gen = torch.Generator().manual_seed(1)
    P = torch.randn(B, N, Cout, generator=gen).to(DEV).requires_grad_(True)
    xyz = torch.rand(B, N, 3, generator=gen).to(DEV)
    centers = xyz[:, :S].contiguous()
    idx = torch.randint(0, N, (B, S, K), generator=gen, dtype=torch.int32).to(DEV)
    Wr = torch.randn(Cout, 3, generator=gen).to(DEV).requires_grad_(True)
    gamma = torch.ones(Cout, device=DEV, requires_grad=True)
    beta = torch.zeros(Cout, device=DEV, requires_grad=True)
    dout = torch.randn(B, S, Cout, generator=gen).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.enable_grad():
        out = ops.group_train(P, xyz, centers, idx, Wr, gamma, beta, 0.3)
        grads = torch.autograd.grad(out, (P, Wr, gamma, beta), dout)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    note(f"group_train peak memory over the inputs at B={B} N={N} S={S} K={K} Cout={Cout}: {extra / 2 ** 20:.1f} MiB "
         f"(one (B,S,K,Cout) fp32 tensor: {B * S * K * Cout * 4 / 2 ** 20:.0f} MiB)")
    assert extra < B * S * K * Cout * 4 // 2
    assert all(torch.isfinite(g).all() for g in grads)


# ---- Encoder.train() -------------------------------------------------------------------------------------------------------

def _encoder(cfg):
    from deeppointmap_amd.encoder import Encoder
    enc = Encoder(cfg)
    enc.load_state_dict(C.state_dict(cfg), strict=True)
    return enc.to(DEV)


def hip_step(name, enc=None):
    """Encoder.train().forward -> backward of sum(fea * G * ~padding) -> (coor, fea, padding, {param: grad}, trace, encoder)"""
    cfg = C.cfg(name)
    pts, pad, G = C.inputs(name)
    enc = (enc or _encoder(cfg)).train()
    enc.zero_grad(set_to_none=True)
    trace = {}
    coor, fea, padding = enc(torch.from_numpy(pts), torch.from_numpy(pad), trace=trace)
    assert fea.requires_grad, "fea carries no graph"
    with torch.enable_grad():
        (fea * torch.from_numpy(G).to(DEV) * (~padding).unsqueeze(1)).sum().backward()
    return coor, fea.detach(), padding, {k: p.grad.clone() for k, p in enc.flat().items()}, trace, enc


def _module_geometry(cfg, trace):
    n = len(cfg.encoder.npoint)
    level_xyz = [trace[f"downsampler.{i}.fps.new"] for i in range(n)]
    level_len = [trace[f"downsampler.{i}.len"] for i in range(n)]
    idx = {name: trace[name + ".idx"].long() for name, *_ in R.layer_names(cfg)}
    winners = {name: trace[name + ".winners"] for name, *_ in R.layer_names(cfg)}
    return (level_xyz, level_len, idx), winners


@pytest.mark.parametrize("name", list(C.CASES))
def test_encoder_train_forward_and_gradients(name):
    cfg = C.cfg(name)
    fix = C.load_fixture(name, GOLDEN)
    pts, pad, _ = C.inputs(name)
    coor, fea, padding, grads, trace, enc = hip_step(name)
    # forward: the fixture, and the same module in eval mode
    valid = ~fix["padding"]
    assert np.array_equal(padding.cpu().numpy(), fix["padding"])
    L = len(cfg.encoder.npoint) - cfg.encoder.upsample_layers - 1
    assert np.array_equal(coor.cpu().numpy().transpose(0, 2, 1)[valid], fix[f"level_xyz/{L}"][valid])
    assert_features_close(fea.cpu().numpy().transpose(0, 2, 1)[valid], fix["fea/64"].transpose(0, 2, 1)[valid],
                          f"Encoder.train {name} fea vs fixture fp64")
    e_coor, e_fea, e_pad = _encoder(cfg)(torch.from_numpy(pts), torch.from_numpy(pad))
    assert torch.equal(e_coor, coor) and torch.equal(e_pad, padding)
    assert_features_close(fea.cpu().numpy(), e_fea.cpu().numpy(), f"Encoder.train {name} fea vs eval mode")
    # gradients: all 110, finite, against the fp64 restatement on the device with the module's routes
    assert len(grads) == 110 and all(g is not None and torch.isfinite(g).all() for g in grads.values())
    geometry, winners = _module_geometry(cfg, trace)
    _, g64, _ = run_restated(name, torch.float64, DEV, geometry, winners)
    _, g32, _ = run_restated(name, torch.float32, DEV, geometry, winners)
    dense = max(rel_err(g32[k], g64[k]) for k in g64)
    note(f"Encoder.train {name}: dense fp32 restatement on the device vs fp64, equal routes, worst of 110 tensors: {dense:.3e} "
         f"(FLOOR is twice the worst of these over the cases)")
    worst = 0.0
    for k in g64:
        worst = max(worst, check(f"Encoder.train {name} d/d {k}", grads[k].cpu().numpy(), g64[k], float(np.ravel(fix[f"pgrad/{k}/e"])[0])))
    # the fixture itself: routes on valid centre rows, then the gradients where none differs
    differing = 0
    for layer, stage, _, _ in R.layer_names(cfg):
        rows = torch.arange(winners[layer].shape[1], device=DEV).unsqueeze(0) < geometry[1][stage].unsqueeze(1)
        w64 = torch.from_numpy(fix[f"win/{layer}/64"].astype(np.int64)).to(DEV)
        differing += int(((winners[layer] != w64) & rows.unsqueeze(2)).sum())
    unforced = 0.0
    for k, g in grads.items():
        got = C.grad_sample(k, g.cpu().numpy()).astype(np.float64)
        err = float(np.abs(got - fix[f"pgrad/{k}/64"]).max() / float(fix[f"pgrad/{k}/max"][1]))
        unforced = max(unforced, err)
        if differing == 0:
            bound = max(3 * float(np.ravel(fix[f"pgrad/{k}/e"])[0]), FLOOR)
            assert err <= bound, f"{name} d/d {k} vs the fixture: {err:.3e} > {bound:.3e}"
    note(f"Encoder.train {name}: worst HIP gradient error vs forced fp64 {worst:.3e}; routes differing from the fixture's fp64 run "
         f"{differing}; worst error vs the unforced fixture {unforced:.3e}")
    # a second run: identical bytes
    _, fea2, _, grads2, _, _ = hip_step(name, enc)
    assert torch.equal(fea, fea2) and all(torch.equal(grads[k], grads2[k]) for k in grads)


def test_eval_after_train_and_sgd_step():
    name = "reduced_padded"
    cfg = C.cfg(name)
    pts, pad, _ = (torch.from_numpy(a) for a in C.inputs(name))
    before = _encoder(cfg)(pts, pad)
    _, _, _, grads, _, enc = hip_step(name)
    assert all(p.requires_grad for p in enc.parameters())
    enc.eval()
    assert not any(p.requires_grad for p in enc.parameters()) and not enc.training
    after = enc(pts, pad)
    assert not after[1].requires_grad and all(torch.equal(a, b) for a, b in zip(before, after))
    # an optimiser step, then inference: the new weights are read
    enc.train()
    opt = torch.optim.SGD(enc.parameters(), lr=1e-2)
    opt.step()
    enc.eval()
    stepped = enc(pts, pad)
    fresh = _encoder(cfg)
    fresh.load_state_dict(enc.state_dict(), strict=True)
    want = fresh(pts, pad)
    assert all(torch.equal(a, b) for a, b in zip(stepped, want))
    assert not torch.equal(stepped[1], before[1])


def test_training_chain_encoder_decoder_loss():
    """Encoder.train() -> descriptors -> Decoder.train().forward -> RegistrationLoss -> backward() on two frame pairs"""
    from deeppointmap_amd import synthetic
    from deeppointmap_amd.config import reduced_args
    from deeppointmap_amd.decoder import Decoder
    from deeppointmap_amd.loss import RegistrationLoss
    from deeppointmap_amd.weights import init_procedural
    cfg = reduced_args()
    cfg.loss = dict(tau=0.1, offset_value="manhattan", eps_positive=1.0, eps_offset=2.0, lambda_p=1.0, lambda_c=1.0, lambda_o=1.0)
    N, scale = 4096, float(cfg.slam_system.coor_scale)
    base = synthetic.base_cloud(N, seed=4)
    src_f, dst_f = (0, 5), (2, 8)
    src = torch.stack([synthetic.frame(f, N, base) for f in src_f]).float()
    dst = torch.stack([synthetic.frame(f, N, base) for f in dst_f]).float()
    pad = torch.zeros(2, N, dtype=torch.bool)
    Rt = torch.stack([synthetic.relative_pose(a, b) for a, b in zip(src_f, dst_f)]).float().to(DEV)
    gt = (Rt[:, :3, :3].contiguous(), Rt[:, :3, 3:].contiguous())
    enc, dec = _encoder(cfg), init_procedural(Decoder(cfg)).to(DEV)
    eval_before = enc(src, pad)

    def step():
        enc.train(), dec.train()
        enc.zero_grad(set_to_none=True), dec.zero_grad(set_to_none=True)
        cs, fs, ps = enc(src, pad)
        cd, fd, pd = enc(dst, pad)
        with torch.enable_grad():
            ds, dd = torch.cat([fs, cs * scale], dim=1), torch.cat([fd, cd * scale], dim=1)
            outs = dec(ds, dd, ps, pd, gt)
            loss = RegistrationLoss(cfg)((gt[0] @ ds[:, -3:] + gt[1]).detach(), dd[:, -3:].detach(), ps, pd, *outs)[0]
            loss.backward()
        return loss.detach().clone(), {"enc." + k: p.grad.clone() for k, p in enc.flat().items()}, \
            {"dec." + k: (None if p.grad is None else p.grad.clone()) for k, p in dec.flat().items()}
    loss, ge, gd = step()
    assert torch.isfinite(loss)
    assert len(ge) == 110
    for k, g in list(ge.items()) + [(k, g) for k, g in gd.items() if "loop" not in k]:
        assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0, k
    assert all(g is None for k, g in gd.items() if "loop" in k)
    loss2, ge2, gd2 = step()
    assert torch.equal(loss, loss2) and all(torch.equal(ge[k], ge2[k]) for k in ge)
    assert all(torch.equal(gd[k], gd2[k]) for k in gd if gd[k] is not None)
    enc.eval(), dec.eval()
    eval_after = enc(src, pad)
    assert_features_close(eval_after[1].cpu().numpy(), eval_before[1].cpu().numpy(), "eval after the training chain")
    assert torch.equal(eval_after[0], eval_before[0]) and torch.equal(eval_after[2], eval_before[2])


def test_refusals():
    from deeppointmap_amd import ops
    from deeppointmap_amd.config import reduced_args, reduced_voxel_args
    from deeppointmap_amd.encoder import Encoder
    name = "reduced_padded"
    pts, pad, _ = (torch.from_numpy(a) for a in C.inputs(name))
    with pytest.raises(ValueError, match="voxel"):
        _encoder(reduced_voxel_args()).train()(pts, pad)
    enc = _encoder(reduced_args())
    samp = enc.presample(pts, pad)
    enc.train()
    for kw in (dict(descriptor_scale=60.0), dict(presampled=samp), dict(stop_level=2), dict(resume={}), dict(spare_frames=1)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            enc(pts, pad, **kw)
    with pytest.raises(RuntimeError, match="GPU only"):
        Encoder(reduced_args()).train()(pts, pad)
    # a width the kernels do not cover: the message names the layer
    t = _layer_inputs(32, 32)
    P = torch.zeros(2, 2048, 48, device=DEV)
    with pytest.raises(ValueError, match="downsampler.9.sa.mlp"):
        ops.group_train(P, t["xyz"], t["centers"], t["idx"], torch.zeros(48, 3, device=DEV), torch.ones(48, device=DEV),
                        torch.zeros(48, device=DEV), 0.1, layer="downsampler.9.sa.mlp")
    wide = reduced_args()
    wide.encoder.width = 24
    wide_enc = Encoder(wide)
    from deeppointmap_amd.weights import init_procedural
    init_procedural(wide_enc).to(DEV).train()
    with pytest.raises(ValueError, match=r"downsampler\.0\.sa\.mlp"):
        wide_enc(pts, pad)
