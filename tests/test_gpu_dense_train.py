"""GPU: the dense training primitive (csrc/dense_train.hip; ops.dense_linear_train, ops.dense_linear_ln_train), forward and backward.

Reference: the plain-torch restatement (tests/dense_train_restated.py, pinned to torch's own layers by
tests/test_dense_train_host.py) evaluated on the CPU, once per case.

Bounds.  Forward: the project's rule (conftest.assert_features_close, 1e-5 x scale) against the fp64 restatement.  ReLU mask:
`out > 0` equals the fp64 mask except where |pre64| <= 1e-5 max |pre64|, and such exceptions are at most 1e-3 of the elements.
Gradients, per tensor in the maximum norm relative to max |fp64|: max(3 e, FLOOR) against the fp64 restatement GIVEN THE KERNEL'S
MASK (one element whose sign differs between fp32 and fp64 moves a max-norm gradient error to 5e-2: the two are compared on the
same branch), e = the error of the fp32 restatement on the CPU with that mask against the fp64 one (torch on the device is not
used for e: profiles/decoder_train_accuracy.md records a case where its default GEMM backend is 1.1e-2 off), factor 3 the margin
the project grants over a reference's own fp32 error (tests/test_gpu_margin.py), FLOOR = 1.4e-5 the project's figure from
tests/test_gpu_decoder_train.py.  Every observed error goes to conftest's log; profiles/dense_train_accuracy.md keeps the
figures.
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import assert_features_close

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_train_restated as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 1.4e-5
MASK_BAND = 1e-5
MASK_SHARE = 1e-3

# name -> (R, Cin, Cout, normed, relu, operands, make_case keywords)
CASES = {
    "1_cin3": (130, 3, 16, False, False, ("bias",), {}),
    "2_ldw19": (257, 16, 32, False, False, ("bias",), dict(ldw=19)),
    "3_cout3": (77, 64, 3, False, False, ("bias", "residual"), {}),
    "4_strided_x_relu": (1000, 256, 768, False, True, ("bias",), dict(x_in=(768, 256))),
    "5_fused_ln": (4160, 256, 256, True, False, ("bias", "residual", "post"), {}),
    "6_wide_ln_relu": (300, 512, 2048, True, True, ("bias",), {}),
    "7_long_k_ln": (193, 2048, 512, True, True, ("bias", "post"), {}),
}
_inputs = {}


def inputs(name):
    """the case's operands on the CPU (shared, never modified) and which of them the call uses, in the order of the gradients"""
    if name not in _inputs:
        Rr, Cin, Cout, normed, relu, opt, kw = CASES[name]
        t = R.make_case(Rr, Cin, Cout, seed=100 + int(name[0]), **kw)
        names = ["x", "W"] + [k for k in ("bias",) if k in opt] + (["gamma", "beta"] if normed else []) + \
            [k for k in ("residual", "post") if k in opt]
        _inputs[name] = (t, names)
    return _inputs[name]


def hip_run(name, x_grad=True):
    """-> (out, {operand: gradient | None}) on the device; the operands keep the strides of the case (column slices stay slices)"""
    from deeppointmap_amd import ops
    _, _, _, normed, relu, _, _ = CASES[name]
    t, names = inputs(name)
    dev = {}
    for k in names:   # a slice of a buffer goes to the device as the same slice of the buffer's copy
        base = t[k]._base if t[k]._base is not None else t[k]
        d = base.to(DEV)
        dev[k] = (d if t[k]._base is None else d.as_strided(t[k].shape, t[k].stride(), t[k].storage_offset())).requires_grad_(
            x_grad or k != "x")
    act = ops.ACT_RELU if relu else ops.ACT_NONE
    with torch.enable_grad():
        if normed:
            out = ops.dense_linear_ln_train(dev["x"], dev["W"], dev.get("bias"), dev["gamma"], dev["beta"], dev.get("residual"),
                                            dev.get("post"), act)
        else:
            out = ops.dense_linear_train(dev["x"], dev["W"], dev.get("bias"), dev.get("residual"), act)
        wanted = [k for k in names if dev[k].requires_grad]
        grads = dict(zip(wanted, torch.autograd.grad(out, [dev[k] for k in wanted], t["dy"].to(DEV))))
    assert dev["x"].stride() == t["x"].stride() and dev["W"].stride() == t["W"].stride()
    return out.detach(), {k: grads.get(k) for k in names}


def restated(name, dtype, mask):
    """the restatement on the CPU in `dtype` -> (out, pre, h | None, {operand: gradient}); mask None = no activation"""
    _, _, _, normed, _, _, _ = CASES[name]
    t, names = inputs(name)
    a = {k: t[k].to(dtype).clone().requires_grad_(True) for k in names}
    with torch.enable_grad():
        if normed:
            out, pre, h = R.normed(a["x"], a["W"], a.get("bias"), a["gamma"], a["beta"], a.get("residual"), a.get("post"), mask)
        else:
            out, pre = R.plain(a["x"], a["W"], a.get("bias"), a.get("residual"), mask)
            h = None
        grads = torch.autograd.grad(out, [a[k] for k in names], t["dy"].to(dtype))
    return out.detach(), pre.detach(), None if h is None else h.detach(), dict(zip(names, grads))


def rel_err(a, b):
    m = float(b.abs().max())
    return float((a.double() - b.double()).abs().max()) / (m if m > 0 else 1.0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_mask_and_gradients(name):
    _, _, _, normed, relu, _, _ = CASES[name]
    t, names = inputs(name)
    out, grads = hip_run(name)
    out_c = out.cpu()
    # forward against the fp64 restatement with its own mask
    _, pre64, _, _ = restated(name, torch.float64, None)
    want = pre64.clamp(min=0) if relu else pre64
    assert_features_close(out_c.numpy(), want.numpy(), f"dense_train {name} forward")
    # the mask
    mask = None
    if relu:
        mask = out_c > 0
        differ = mask != (pre64 > 0)
        band = MASK_BAND * float(pre64.abs().max())
        assert not (differ & (pre64.abs() > band)).any(), "a sign differs outside the rounding band"
        share = differ.sum().item() / differ.numel()
        borderline = (pre64.abs() <= band).sum().item() / differ.numel()
        print(f"dense_train {name}: mask differs from fp64 at {share:.2e} of {differ.numel()} elements, borderline share {borderline:.2e}")
        assert share <= MASK_SHARE
    # gradients on the kernel's branch
    _, _, _, g64 = restated(name, torch.float64, mask)
    _, _, _, g32 = restated(name, torch.float32, mask)
    for k in names:
        e = rel_err(g32[k], g64[k])
        m = float(g64[k].abs().max()) or 1.0
        assert grads[k].shape == t[k].shape
        assert_features_close(grads[k].cpu().double().numpy() / m, g64[k].numpy() / m, f"dense_train {name} d/d {k} (e {e:.2e})",
                              tol=max(3 * e, FLOOR))


@pytest.mark.parametrize("name", sorted(CASES))
def test_repeatable_and_x_gradient_optional(name):
    _, names = inputs(name)
    out, grads = hip_run(name)
    out2, grads2 = hip_run(name)
    assert torch.equal(out, out2)
    for k in names:
        assert torch.equal(grads[k], grads2[k]), f"d/d {k}: two runs differ"
    out3, grads3 = hip_run(name, x_grad=False)
    assert torch.equal(out, out3) and grads3["x"] is None
    for k in names[1:]:
        assert torch.equal(grads[k], grads3[k]), f"d/d {k} changes when x needs no gradient"


def test_pre_norm_rows_are_the_plain_forms_bits():
    """h of the fused-epilogue kernel (case 5) and of the GEMM-then-rows path (case 6) = dense_linear_train of the same operands"""
    from deeppointmap_amd import ops
    for name in ("5_fused_ln", "6_wide_ln_relu"):
        t, names = inputs(name)
        d = {k: t[k].to(DEV) for k in names}
        _, h, stats = ops.dense_train_forward(d["x"], d["W"], d.get("bias"), d["gamma"], d["beta"], d.get("residual"), d.get("post"))
        plain = ops.dense_linear_train(d["x"], d["W"], d.get("bias"), d.get("residual"))
        assert h.shape == plain.shape and torch.equal(h, plain), name
        h64 = plain.double()
        assert_features_close(stats[:, 0].cpu().numpy(), h64.mean(1).cpu().numpy(), f"dense_train {name} row means")
        rstd = 1 / torch.sqrt(h64.var(1, unbiased=False) + R.EPS)
        assert_features_close((stats[:, 1].double() / rstd).cpu().numpy(), np.ones(h.shape[0]), f"dense_train {name} rstd ratio")


def test_empty_rows():
    """case 8: R = 0 gives empty outputs, an empty x gradient and weight gradients that are exactly zero"""
    from deeppointmap_amd import ops
    for Cin, Cout, normed in ((512, 256, False), (256, 256, True)):
        t = R.make_case(0, Cin, Cout, seed=8)
        a = {k: t[k].to(DEV).requires_grad_(True) for k in ("x", "W", "bias", "gamma", "beta", "residual", "post")}
        with torch.enable_grad():
            if normed:
                out = ops.dense_linear_ln_train(a["x"], a["W"], a["bias"], a["gamma"], a["beta"], a["residual"], a["post"], ops.ACT_RELU)
                leaves = list(a.values())
            else:
                out = ops.dense_linear_train(a["x"], a["W"], a["bias"], a["residual"], ops.ACT_RELU)
                leaves = [a[k] for k in ("x", "W", "bias", "residual")]
            grads = torch.autograd.grad(out, leaves, t["dy"].to(DEV))
        assert tuple(out.shape) == (0, Cout)
        for leaf, g in zip(leaves, grads):
            assert g.shape == leaf.shape and not g.any()
        assert grads[1].numel() == Cout * Cin


def test_leading_dimensions_and_checkpoint():
    """(B, N, Cin) operands as the encoder passes them, and recomputation under torch.utils.checkpoint: identical bytes"""
    from torch.utils.checkpoint import checkpoint
    from deeppointmap_amd import ops
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(2, 75, 19, generator=gen).to(DEV)
    W = torch.randn(64, 19, generator=gen).to(DEV)
    b, g, be = (torch.randn(64, generator=gen).to(DEV) for _ in range(3))
    post = torch.randn(2, 75, 64, generator=gen).to(DEV)
    dy = torch.randn(2, 75, 64, generator=gen).to(DEV)

    def f(x, W, b, g, be, post):
        return ops.dense_linear_ln_train(ops.dense_linear_train(x, W[:, :16].repeat(1, 2)[:, :19], b, act=ops.ACT_RELU)[..., :19],
                                         W, b, g, be, post=post, act=ops.ACT_RELU)
    res = []
    for ck in (False, True):
        leaves = [v.clone().requires_grad_(True) for v in (x, W, b, g, be, post)]
        with torch.enable_grad():
            out = checkpoint(f, *leaves, use_reentrant=False) if ck else f(*leaves)
            res.append((out.detach(),) + torch.autograd.grad(out, leaves, dy))
    assert tuple(res[0][0].shape) == (2, 75, 64)
    for u, v in zip(*res):
        assert torch.equal(u, v)
    flat = ops.dense_linear_ln_train(ops.dense_linear_train(x.view(150, 19), W[:, :16].repeat(1, 2)[:, :19], b, act=ops.ACT_RELU)[:, :19],
                                     W, b, g, be, post=post.view(150, 64), act=ops.ACT_RELU)
    assert torch.equal(flat.view(2, 75, 64), res[0][0])
