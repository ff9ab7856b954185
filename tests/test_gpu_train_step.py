"""GPU: the training step -- ops.map_poses / ops.map_assemble (csrc/map_assemble.hip), DeepPointModelPipeline and TrainStep.

Assembly, against the reference's recorded run (tests/golden/train_step_<case>.npz, fp32 and fp64):
  feature rows, masks, the coordinates of a map's first frame and dst_global's copy of them: identical bytes to the fp32 run;
  the other coordinates, gt and src_global, per output and case:
      max |hip - ref64| <= max(3 max |ref32 - ref64|, 4 * 2^-24 * max |ref64|)
  the project's three-way rule (profiles/r06_margin_three_way.md); the floor is the four roundings of a 3-term product plus add.
Pipeline, against the INTEGRATION.md recipe written out here (the same modules with torch glue, tests/train_step_restated.py):
  per tensor (loss, metrics, every parameter gradient), relative to the largest magnitude of the fp64-glue value,
      |pipeline - recipe with fp64 glue| <= 3 |recipe with fp32 glue - recipe with fp64 glue|
  which is the coordinate bound above carried through the decoder, the loss and the backward by the recipe itself.
Every observed error goes to test_logs/train_step_errors.log (profiles/train_step_accuracy.md is made from it).
"""
import io
import os
import pickle
import random
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_train_cases as LC  # noqa: E402
import train_step_cases as C  # noqa: E402
import train_step_restated as R  # noqa: E402
from test_gpu_optim import log  # noqa: E402
from test_train_step_host import CASES, RUNS, fixture, host_lookup  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOSS = dict(tau=0.1, offset_value="manhattan", eps_positive=1.0, eps_offset=2.0, lambda_p=1.0, lambda_c=1.0, lambda_o=1.0)


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def hip_assembly(inputs, S1, fea=None):
    """ops.map_poses + ops.map_assemble on a case -> (six outputs, rel, gt)"""
    from deeppointmap_amd import ops
    icp, has = host_lookup(inputs, S1)
    rel, gt = ops.map_poses(dev(inputs["R"]), dev(inputs["T"]), dev(inputs["calib"]), dev(icp), dev(has, torch.uint8), inputs["S"], S1)
    fea = dev(inputs["fea"]) if fea is None else fea
    outs = ops.map_assemble(dev(inputs["coor"]), fea, dev(inputs["mask"], torch.bool), rel, gt, inputs["S"], S1, C.COOR_SCALE)
    return outs, rel, gt


@pytest.mark.parametrize("name,seed", RUNS)
def test_assembly_against_the_reference(name, seed):
    inputs, fix = CASES[name], fixture(name)
    S1, Cc, N, S = int(fix[f"{seed}/S1"]), inputs["C"], inputs["N"], inputs["S"]
    (src_desc, dst_desc, src_mask, dst_mask, src_global, dst_global), rel, gt = hip_assembly(inputs, S1)
    got = {"src_desc": src_desc, "dst_desc": dst_desc, "gt": gt, "src_global": src_global, "dst_global": dst_global}
    got = {k: v.cpu().numpy() for k, v in got.items()}
    ref32 = {k: fix[f"{seed}/{k}/32"] for k in got}
    ref64 = {k: fix[f"{seed}/{k}/64"] for k in got}
    assert src_mask.dtype == torch.bool and np.array_equal(src_mask.cpu().numpy(), fix[f"{seed}/src_mask"])
    assert np.array_equal(dst_mask.cpu().numpy(), fix[f"{seed}/dst_mask"])
    for k in ("src_desc", "dst_desc"):
        assert got[k].shape == ref32[k].shape
        assert got[k][:, :Cc].tobytes() == ref32[k][:, :Cc].tobytes(), f"{k}: feature rows"
        assert got[k][:, Cc:, :N].tobytes() == ref32[k][:, Cc:, :N].tobytes(), f"{k}: the first frame's coordinates"
    assert got["dst_global"].tobytes() == got["dst_desc"][:, Cc:].tobytes()
    assert got["dst_global"][:, :, :N].tobytes() == ref32["dst_global"][:, :, :N].tobytes()
    firsts = rel.cpu().view(inputs["B"], S, 3, 4)[:, [0, S1]]
    assert torch.equal(firsts, torch.eye(3, 4).expand_as(firsts)), "the first frames' poses are the exact identity"
    for k in got:
        coords = slice(Cc, None) if k.endswith("desc") else slice(None)
        h, r32, r64 = got[k][:, coords].astype(np.float64), ref32[k][:, coords].astype(np.float64), ref64[k][:, coords]
        err, e = np.abs(h - r64).max(), np.abs(r32 - r64).max()
        bound = max(3 * e, 4 * 2.0 ** -24 * np.abs(r64).max())
        log(f"assembly {name} seed {seed} (S1 {S1}) {k}: max|hip-ref64| {err:.3e}, max|ref32-ref64| {e:.3e}, bound {bound:.3e}")
        assert err <= bound, (k, err, bound)


@pytest.mark.parametrize("name,seed", [("a", 0), ("b", 5), ("c", 0)])
def test_assembly_backward_and_repeatability(name, seed):
    """dfea byte-equal to autograd through the restatement on the same upstream gradients; coor gets none; identical bytes twice"""
    inputs, fix = CASES[name], fixture(name)
    S1 = int(fix[f"{seed}/S1"])
    coor = dev(inputs["coor"]).requires_grad_(True)
    fea = dev(inputs["fea"]).requires_grad_(True)
    with torch.enable_grad():
        from deeppointmap_amd import ops
        icp, has = host_lookup(inputs, S1)
        rel, gt = ops.map_poses(dev(inputs["R"]), dev(inputs["T"]), dev(inputs["calib"]), dev(icp), dev(has, torch.uint8), inputs["S"], S1)
        outs = ops.map_assemble(coor, fea, dev(inputs["mask"], torch.bool), rel, gt, inputs["S"], S1, C.COOR_SCALE)
        gen = torch.Generator().manual_seed(11)
        ups = [torch.randn(o.shape, generator=gen).to(DEV) for o in outs[:2]]
        assert [o.requires_grad for o in outs] == [True, True, False, False, False, False]
        (outs[0] * ups[0]).sum().backward(retain_graph=True)
        only_src = fea.grad.clone()
        (outs[1] * ups[1]).sum().backward()
    assert coor.grad is None
    fea2 = dev(inputs["fea"]).requires_grad_(True)
    with torch.enable_grad():
        want = R.assemble(dev(inputs["coor"]), fea2, dev(inputs["mask"], torch.bool), rel, gt, inputs["S"], S1, C.COOR_SCALE)
        (want[0] * ups[0]).sum().backward(retain_graph=True)
        want_src = fea2.grad.clone()
        (want[1] * ups[1]).sum().backward()
    assert torch.equal(only_src, want_src), "a backward with one descriptor gradient only: the other map's frames get zeros"
    assert torch.equal(fea.grad, fea2.grad)
    again, rel2, gt2 = hip_assembly(inputs, S1)
    assert torch.equal(rel, rel2) and torch.equal(gt, gt2) and all(torch.equal(a, b) for a, b in zip(outs, again))


@pytest.mark.parametrize("B,S,S1,N,Cc", [(2, 3, 1, 1, 4), (1, 4, 3, 8, 1), (2, 6, 5, 12, 3), (1, 2, 1, 300, 2)])
def test_assembly_shapes_beyond_the_cases(B, S, S1, N, Cc):
    """N = 1, S1 = S - 1, C = 1, more than one block of points; aligned (N % 4 == 0) and unaligned rows -- against the
    restatement in fp64.  Features, masks and first frames: exact.  The assembly is checked on the kernel's own poses (read
    back and widened), so its bound is its own arithmetic: 4 roundings of the largest value for a moved point (the floor of
    the fixture bound; the restatement's fp32 run is not a reference, so there is no 3 e term), 8 for src_global, which moves
    a moved point again.  The poses against the restatement's fp64 poses: 64 roundings of the largest entry -- an elimination
    of a 4x4 with condition number below 10 (an orthonormal block and a translation of a few units) and two 4x4 products, each
    entry a 4-term sum, about 20 roundings of values up to the largest entry, with a factor 3 on top."""
    from deeppointmap_amd import ops
    gen = torch.Generator().manual_seed(100 * B + 10 * S + N)
    F = B * S
    rnd = lambda *s: torch.randn(*s, generator=gen)   # noqa: E731
    coor, fea, mask = rnd(F, 3, N) / 60, rnd(F, Cc, N), torch.rand(F, N, generator=gen) < 0.3
    Rm = torch.linalg.qr(rnd(F, 3, 3))[0]
    T, calib = 10 * rnd(F, 3, 1), torch.eye(4).repeat(F, 1, 1)
    calib[:, :3, :3] = torch.linalg.qr(rnd(F, 3, 3))[0]
    calib[:, :3, 3] = rnd(F, 3)
    icp = torch.eye(4).repeat(F + B, 1, 1)
    icp[:, :3, :3] = torch.linalg.qr(rnd(F + B, 3, 3))[0]
    icp[:, :3, 3] = rnd(F + B, 3)
    has = (torch.arange(F + B) % 2).to(torch.uint8)
    d = lambda t: t.to(DEV).contiguous()   # noqa: E731
    rel, gt = ops.map_poses(d(Rm), d(T), d(calib), d(icp.reshape(-1, 16)), d(has), S, S1)
    outs = ops.map_assemble(d(coor), d(fea), d(mask), rel, gt, S, S1, 60.0)
    rel64, gt64 = R.poses(Rm.double(), T.double(), calib.double(), icp.reshape(-1, 16).double(), has, S, S1)
    want = R.assemble(coor.double(), fea.double(), mask, rel.cpu().double(), gt.cpu().double(), S, S1, 60.0)
    assert [tuple(o.shape) for o in outs] == [tuple(w.shape) for w in want]
    assert torch.equal(outs[2].cpu(), want[2]) and torch.equal(outs[3].cpu(), want[3])
    for k, (o, w) in zip(("src_desc", "dst_desc"), zip(outs[:2], want[:2])):
        assert torch.equal(o[:, :Cc].cpu(), w[:, :Cc].float()), k
        assert torch.equal(o[:, Cc:, :N].cpu(), (w[:, Cc:, :N]).float()), k   # coor * scale: one rounding either way
    for k, o, w in (("rel", rel, rel64), ("gt", gt, gt64), ("src_xyz", outs[0][:, Cc:], want[0][:, Cc:]),
                    ("dst_xyz", outs[1][:, Cc:], want[1][:, Cc:]), ("src_global", outs[4], want[4]), ("dst_global", outs[5], want[5])):
        err = float((o.cpu().double() - w).abs().max())
        roundings = {"rel": 64, "gt": 64, "src_global": 8}.get(k, 4)
        bound = roundings * 2.0 ** -24 * max(float(w.abs().max()), float(want[0][:, Cc:].abs().max()))
        log(f"assembly shape B{B} S{S} S1{S1} N{N} C{Cc} {k}: max|hip-restated64| {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (k, err, bound)
    for bad in (dict(S1=0), dict(S1=S)):
        with pytest.raises(ValueError):
            ops.map_assemble(d(coor), d(fea), d(mask), rel, gt, S, bad["S1"], 60.0)


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------

def _args():
    from deeppointmap_amd.config import reduced_args
    cfg = reduced_args()
    cfg.loss = dict(LOSS)
    cfg.train = dict(
        registration=dict(map_size_max=8, optimizer=dict(type="AdamW", kwargs=dict(lr=1e-4, weight_decay=1e-2)),
                          scheduler=dict(type="cosine", kwargs=dict(T_max=10)), K_0=2, K_mult=2, mult_epoch=[2, 4]),
        loop_detection=dict(distance=LC.DISTANCE, optimizer=dict(type="sgd", kwargs=dict(lr=1e-3, momentum=0.9)),
                            scheduler=dict(type="identity", kwargs={})))
    return cfg


def _modules(cfg, dense="hip"):
    import encoder_train_cases as EC
    from deeppointmap_amd.decoder import Decoder
    from deeppointmap_amd.encoder import Encoder
    from deeppointmap_amd.loss import RegistrationLoss
    from deeppointmap_amd.weights import init_procedural
    enc = Encoder(cfg)
    enc.load_state_dict(EC.state_dict(cfg), strict=True)
    dec = init_procedural(Decoder(cfg))
    return enc.to(DEV).set_train_dense(dense), dec.to(DEV).set_train_dense(dense), RegistrationLoss(cfg)


def _batch(tmp_path, N=4096, frames=(0, 3, 5, 9)):
    """one map of four synthetic frames with their global poses, a calibration, and a dictionary that covers one pair"""
    from deeppointmap_amd import synthetic
    base = synthetic.base_cloud(N, seed=4)
    pcd = torch.stack([synthetic.frame(f, N, base) for f in frames]).float()
    P = torch.stack([synthetic.sensor_pose(f) for f in frames]).float()
    calib = torch.eye(4).repeat(len(frames), 1, 1)
    path = str(tmp_path / "refined.pkl")
    with open(path, "wb") as f:   # frame 3 in frame 0, refined: the pipeline must take this, not the global poses
        pickle.dump({(0, 3): synthetic.relative_pose(3, 0).numpy() @ np.array(C._se3(np.random.default_rng(2), 0.002, 0.02))}, f)
    info = {"num_map": 1, "dsf_index": [(0, 0, f) for f in frames], "refined_SE3_file": [path]}
    return (pcd.to(DEV), P[:, :3, :3].contiguous().to(DEV), P[:, :3, 3:].contiguous().to(DEV),
            torch.zeros(len(frames), N, dtype=torch.bool, device=DEV), calib.to(DEV), info)


def _recipe(enc, dec, crit, batch, S1, scale, table, glue):
    """INTEGRATION.md's hand-written step: encoder -> torch glue in `glue` precision -> decoder -> criterion -> backward"""
    from deeppointmap_amd.train_pipeline import icp_table
    pcd, Rm, T, pad, calib, info = batch
    B, S = info["num_map"], pcd.shape[0] // info["num_map"]
    enc.zero_grad(set_to_none=True), dec.zero_grad(set_to_none=True)
    with torch.enable_grad():
        coor, fea, mask = enc(pcd, pad)
        icp, has = icp_table(np.asarray([i[2] for i in info["dsf_index"]]).reshape(B, S), [table], S1)
        rel, gt = R.poses(Rm.to(glue), T.to(glue), calib.to(glue), dev(icp, glue), dev(has, torch.uint8), S, S1)
        sd, dd, sm, dm, sg, dg = R.assemble(coor.to(glue), fea.to(glue), mask, rel.to(DEV), gt.to(DEV), S, S1, scale)
        gt3 = gt.to(DEV).reshape(B, 3, 4).float()
        outs = dec(sd.float(), dd.float(), src_padding_mask=sm, dst_padding_mask=dm, gt_Rt=(gt3[:, :, :3].contiguous(), gt3[:, :, 3:].contiguous()))
        loss, top1, lp, lc, lo = crit(sg.float(), dg.float(), sm, dm, *outs)
        loss.backward()
        off = (torch.norm(outs[4].detach(), p=2, dim=1).mean() + torch.norm(outs[5].detach(), p=2, dim=1).mean()) / 2
    metrics = dict(loss_regis=float(loss), loss_p=float(lp), loss_c=float(lc), loss_o=float(lo), top1_acc=top1, offset_err=float(off))
    grads = {"encoder." + k: p.grad for k, p in enc.flat().items()}
    grads.update({"decoder." + k: p.grad for k, p in dec.flat().items()})
    return float(loss), metrics, {k: (None if g is None else g.detach().clone()) for k, g in grads.items()}


def test_pipeline_registration_step_against_the_recipe(tmp_path):
    from deeppointmap_amd.train_pipeline import METRIC_KEYS, DeepPointModelPipeline
    cfg = _args()
    enc, dec, crit = _modules(cfg)
    batch, S1 = _batch(tmp_path), 2
    model = DeepPointModelPipeline(cfg, enc, dec, crit)
    model.train()
    table = model._load_refined_SE3(batch[5]["refined_SE3_file"][0])

    def pipeline_step():
        model.zero_grad(set_to_none=True)
        with torch.enable_grad():
            loss, metrics = model(*batch, s1=S1)
            loss.backward()
        return loss.detach().clone(), metrics, {k: (None if p.grad is None else p.grad.clone()) for k, p in model.named_parameters()}
    loss, metrics, grads = pipeline_step()
    assert tuple(metrics) == METRIC_KEYS and all(isinstance(v, float) for v in metrics.values()) and torch.isfinite(loss)
    assert metrics["loss_regis"] == float(loss)
    have = [k for k, g in grads.items() if g is not None]
    assert sum(k.startswith("encoder.") for k in have) == 110 and sum(k.startswith("decoder.") for k in have) == 74
    assert sorted(k for k, g in grads.items() if g is None) == sorted("decoder." + k for k in LC.HEAD)
    # identical bytes twice ("hip" dense mode: the whole step is one instruction sequence)
    loss2, metrics2, grads2 = pipeline_step()
    assert torch.equal(loss, loss2) and metrics == metrics2 and all(torch.equal(grads[k], grads2[k]) for k in have)
    # the recipe, with fp32 and with fp64 glue
    scale = cfg.slam_system.coor_scale
    l32, m32, g32 = _recipe(enc, dec, crit, batch, S1, scale, table, torch.float32)
    l64, m64, g64 = _recipe(enc, dec, crit, batch, S1, scale, table, torch.float64)
    worst = 0.0

    def check(what, got, r32, r64):
        nonlocal worst
        got, r32, r64 = (np.asarray(x, np.float64) for x in (got, r32, r64))
        m = max(float(np.abs(r64).max()), 1e-30)
        err, e = float(np.abs(got - r64).max()) / m, float(np.abs(r32 - r64).max()) / m
        log(f"pipeline {what}: |pipeline-recipe64| {err:.3e}, |recipe32-recipe64| {e:.3e} (relative to max |recipe64|)")
        worst = max(worst, err / e if e > 0 else (0.0 if err == 0 else float("inf")))
        assert err <= 3 * e, (what, err, e)
    for k in METRIC_KEYS:
        check("metric " + k, metrics[k], m32[k], m64[k])
    for k in have:
        check("grad " + k, grads[k].cpu().numpy(), g32[k].cpu().numpy(), g64[k].cpu().numpy())
    log(f"pipeline: worst |pipeline-recipe64| / |recipe32-recipe64| over {len(have) + len(METRIC_KEYS)} tensors: {worst:.3f}")


class _FixedEncoder(torch.nn.Module):
    """an encoder that returns a loop_train case's descriptors (its tokens are given, not encoded)"""

    def __init__(self, inputs):
        super().__init__()
        desc = torch.cat([dev(inputs["src"]), dev(inputs["dst"])])
        ps, pd = LC.masks(inputs)
        self.out = (desc[:, -3:].contiguous(), desc[:, :-3].contiguous(), torch.cat([dev(ps, torch.bool), dev(pd, torch.bool)]))
        self.train_stage = "registration"

    def set_train_stage(self, stage):
        self.train_stage = stage
        return self

    def forward(self, pcd, mask):
        return self.out


def test_stage_switch_and_loop_detection_step():
    from deeppointmap_amd.decoder import Decoder
    from deeppointmap_amd.loss import LoopDetectionLoss
    from deeppointmap_amd.train_pipeline import DeepPointModelPipeline
    inputs, cfg = LC.cases()["pairs_256"]
    cfg.slam_system = SimpleNamespace(coor_scale=1.0)
    dec = Decoder(cfg)
    dec.load_state_dict(LC.state_dict(cfg), strict=True)
    dec = dec.to(DEV)
    enc = _FixedEncoder(inputs)
    model = DeepPointModelPipeline(cfg, enc, dec, None)
    model.train()
    assert not any(p.requires_grad for k, p in model.named_parameters() if "loop" in k)
    model.loop_detection()
    model.train()    # what the trainer calls every epoch: the stage survives it
    assert enc.train_stage == dec.train_stage == "loop_detection"
    assert sorted(k for k, p in model.named_parameters() if p.requires_grad) == sorted("decoder." + k for k in LC.HEAD)
    B = inputs["src"].shape[0]
    src_T, dst_T = dev(inputs["src_T"]), dev(inputs["dst_T"])
    dummy, dmask = torch.zeros(B, 3, 1, device=DEV), torch.zeros(B, 1, dtype=torch.bool, device=DEV)
    with torch.enable_grad():
        loss, metrics = model(dummy, None, src_T, dmask, None, dummy, None, dst_T, dmask, None)
        loss.backward()
    got = {k: dec.p(k).grad.clone() for k in LC.HEAD}
    # the hand-written recipe of INTEGRATION.md on the same modules
    dec.zero_grad(set_to_none=True)
    coor, fea, mask = enc(None, None)
    with torch.enable_grad():
        pred = dec.loop_detection_forward(torch.cat([fea[:B], coor[:B] * 1.0], 1), torch.cat([fea[B:], coor[B:] * 1.0], 1),
                                          src_padding_mask=mask[:B], dst_padding_mask=mask[B:])
        want_loss, want_metrics = LoopDetectionLoss(cfg)(pred, src_T, dst_T)
        want_loss.backward()
    assert torch.equal(loss, want_loss) and metrics == want_metrics
    assert all(torch.equal(got[k], dec.p(k).grad) for k in LC.HEAD)
    model.registration()
    model.train()
    assert not any(p.requires_grad for k, p in model.named_parameters() if "loop" in k)
    assert all(p.requires_grad for k, p in model.named_parameters() if "loop" not in k)


def test_train_step_checkpoint_resume_and_weights(tmp_path):
    """two step()s, state_dict(), a fresh TrainStep.load_state_dict(), a third step == the third step of the uninterrupted run,
    byte for byte ("hip" dense mode); weights() loads into fresh modules; the epoch rule and the stage change"""
    from deeppointmap_amd import optim as O
    from deeppointmap_amd.decoder import Decoder
    from deeppointmap_amd.encoder import Encoder
    from deeppointmap_amd.train_pipeline import DeepPointModelPipeline, TrainStep
    batch = _batch(tmp_path)

    def fresh():
        cfg = _args()
        enc, dec, crit = _modules(cfg)
        return cfg, TrainStep(cfg, DeepPointModelPipeline(cfg, enc, dec, crit))
    cfg, one = fresh()
    assert type(one.optimizer) is O.AdamW and len(one.optimizer.param_groups[0]["params"]) == 110 + 74
    def step(ts, k):
        random.seed(k)   # the S1 draw of step k is the same in both runs
        return ts.step(*batch)
    for k in range(2):
        metric = step(one, k)
    assert set(metric) == {"loss_regis", "loss_p", "loss_c", "loss_o", "top1_acc", "offset_err"}
    saved = one.state_dict()
    assert sorted(saved) == ["decoder", "encoder", "epoch", "optimizer", "scheduler", "step"] and saved["step"] == 2
    blob = io.BytesIO()
    torch.save(saved, blob)   # the state dict shares the live tensors: a checkpoint is a copy
    saved = torch.load(io.BytesIO(blob.getvalue()), weights_only=False)
    step(one, 2)
    _, two = fresh()
    two.load_state_dict(saved)
    step(two, 2)
    a, b = dict(one.model.named_parameters()), dict(two.model.named_parameters())
    changed = 0
    for k in a:
        assert torch.equal(a[k], b[k]), k
        changed += int(not torch.equal(a[k].detach().cpu(), saved[k.split(".")[0]][k.split(".", 1)[1]].cpu()))
    assert changed >= 150, changed   # the third step moved the trained tensors
    w = two.weights()
    assert sorted(w) == ["decoder", "encoder"]
    Encoder(cfg).load_state_dict(w["encoder"], strict=True), Decoder(cfg).load_state_dict(w["decoder"], strict=True)
    # epoch_end: scheduler, epoch counter, K = K_0 * K_mult ** (entries of mult_epoch reached)
    lr0 = two.optimizer.param_groups[0]["lr"]
    two.epoch_end()
    assert two.epoch == 2 and two.optimizer.param_groups[0]["lr"] < lr0 and two.train_cfg.registration["K"] == 4
    two.epoch_end(), two.epoch_end()
    assert two.epoch == 4 and two.train_cfg.registration["K"] == 8
    two.next_stage()
    assert type(two.optimizer) is O.SGD and len(two.optimizer.param_groups[0]["params"]) == 8
    assert two.model.decoder.train_stage == "loop_detection"
