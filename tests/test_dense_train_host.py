"""CPU: the restatement the GPU tests of csrc/dense_train.hip compare against (tests/dense_train_restated.py) is what torch's own
layers compute, the workspace of the backward does not grow with the rows, and the Python layer refuses bad operands before it
touches a device."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_train_restated as R  # noqa: E402

NAMES = ("x", "W", "bias", "gamma", "beta", "residual", "post")


def _leaves(t, names=NAMES):
    return {k: t[k].double().clone().requires_grad_(True) for k in names}


@pytest.mark.parametrize("relu", [False, True])
def test_restatement_is_torchs_layers(relu):
    """fp64, outputs and all seven gradients equal to 1e-12, the mask taken from torch's own forward"""
    t = R.make_case(37, 19, 24, seed=11)
    dy = t["dy"].double()
    with torch.enable_grad():
        a = _leaves(t)
        pre = F.layer_norm(F.linear(a["x"], a["W"], a["bias"]) + a["residual"], (24,), a["gamma"], a["beta"], eps=R.EPS) + a["post"]
        want = F.relu(pre) if relu else pre
        gw = torch.autograd.grad(want, list(a.values()), dy)
        b = _leaves(t)
        mask = (pre.detach() > 0) if relu else None
        got, _, h = R.normed(b["x"], b["W"], b["bias"], b["gamma"], b["beta"], b["residual"], b["post"], mask)
        gg = torch.autograd.grad(got, list(b.values()), dy)
    assert (got - want).abs().max() <= 1e-12
    assert (h - (F.linear(a["x"], a["W"], a["bias"]) + a["residual"])).abs().max() <= 1e-12
    for k, u, v in zip(NAMES, gg, gw):
        assert (u - v).abs().max() <= 1e-12 * max(1.0, float(v.abs().max())), k
    # the plain form
    names = ("x", "W", "bias", "residual")
    with torch.enable_grad():
        a = _leaves(t, names)
        pre = F.linear(a["x"], a["W"], a["bias"]) + a["residual"]
        want = F.relu(pre) if relu else pre
        gw = torch.autograd.grad(want, list(a.values()), dy)
        b = _leaves(t, names)
        got, _ = R.plain(b["x"], b["W"], b["bias"], b["residual"], (pre.detach() > 0) if relu else None)
        gg = torch.autograd.grad(got, list(b.values()), dy)
    assert (got - want).abs().max() <= 1e-12
    for k, u, v in zip(names, gg, gw):
        assert (u - v).abs().max() <= 1e-12 * max(1.0, float(v.abs().max())), k


def test_workspace_is_constant_in_the_rows_beyond_32_tiles():
    """at most 32 partial dW (+ d bias) and 256 pairs of column partials of the row pass, whatever R"""
    from deeppointmap_amd import _lib
    ws = _lib.load().dpm_dense_train_workspace_bytes
    for Cin, Cout in ((256, 768), (3, 16), (16, 32), (512, 2048), (2048, 512)):
        cap = ws(32 * 64 + 1, Cin, Cout)
        assert cap <= 256 + 256 + 4 * 32 * (Cout * Cin + Cout) + 4 * 256 * 2 * Cout
        assert ws(0, Cin, Cout) <= ws(64, Cin, Cout) < ws(65, Cin, Cout) <= ws(32 * 64, Cin, Cout) <= cap
        assert all(ws(r, Cin, Cout) == cap for r in (32 * 64 + 2, 4160, 256 * 64, 256 * 64 + 1, 131072, 1 << 30))
    assert ws(-1, 4, 4) == 0 and ws(4, 0, 4) == 0 and ws(4, 4, 0) == 0


def test_invalid_arguments_return_einval_without_a_device():
    """every check of the C entry points comes before the first HIP call"""
    from deeppointmap_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(64, 8)
    p = buf.data_ptr()
    assert lib.dpm_dense_train_forward(p, 4, p, 8, None, None, None, None, None, 8, 8, 8, 0, p, None, None, None) == -1   # ldx < Cin
    assert lib.dpm_dense_train_forward(p, 8, p, 8, None, None, None, None, None, 8, 8, 8, 2, p, None, None, None) == -1   # sigmoid
    assert lib.dpm_dense_train_forward(p, 8, p, 8, None, None, p, None, None, 8, 8, 8, 0, p, p, p, None) == -1            # gamma, no beta
    assert lib.dpm_dense_train_forward(p, 8, p, 8, None, None, None, None, p, 8, 8, 8, 0, p, None, None, None) == -1      # post, plain
    assert lib.dpm_dense_train_forward(p, 8, p, 8, None, None, None, None, None, -1, 8, 8, 0, p, None, None, None) == -1
    assert lib.dpm_dense_train_backward_rows(p, p, None, None, p, 8, 8, 0, None, p, p, None, p, None) == -1              # dgamma alone
    assert lib.dpm_dense_train_backward_gemm(p, p, 8, p, 8, 8, 8, 8, None, None, p, p, None) == -1                        # dbias, no dW
    assert lib.dpm_dense_train_backward_gemm(p, p, 8, p, 8, 8, 8, 8, None, p, None, None, None) == -1                     # no workspace


def test_ops_raise_value_errors():
    from deeppointmap_amd import ops
    x, W, b = torch.zeros(5, 8), torch.zeros(4, 8), torch.zeros(4)
    g = torch.ones(4)
    bad = [
        lambda: ops.dense_linear_train(torch.zeros(5, 7), W, b),                         # Cin
        lambda: ops.dense_linear_train(x, W, torch.zeros(5)),                            # bias
        lambda: ops.dense_linear_train(x, W, b, residual=torch.zeros(5, 5)),             # residual
        lambda: ops.dense_linear_train(x, W, b, residual=torch.zeros(4, 4)),             # residual rows
        lambda: ops.dense_linear_train(x.double(), W, b),                                # dtype
        lambda: ops.dense_linear_train(x, W.double(), b),
        lambda: ops.dense_linear_train(x, W.view(4, 8, 1), b),                           # W not 2-D
        lambda: ops.dense_linear_train(x, W, b, act=ops.ACT_SIGMOID),                    # activation
        lambda: ops.dense_linear_ln_train(x, W, b, None, g),                             # gamma missing
        lambda: ops.dense_linear_ln_train(x, W, b, torch.ones(5), g),                    # gamma
        lambda: ops.dense_linear_ln_train(x, W, b, g, g.double()),                       # beta dtype
        lambda: ops.dense_linear_ln_train(x, W, b, g, g, post=torch.zeros(5, 8)),        # post
        lambda: ops.dense_linear_ln_train(x, W, b, g, g, residual=torch.zeros(1, 5, 4)),
        lambda: ops.dense_linear_ln_train(x, W, b, g, g, act=7),
    ]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {k} did not raise")


def test_set_train_dense_switch(cfg_full):
    import copy
    from deeppointmap_amd.decoder import Decoder
    from deeppointmap_amd.encoder import Encoder
    for cls in (Encoder, Decoder):
        m = cls(cfg_full)
        assert m.train_dense == "torch"
        assert m.set_train_dense("hip") is m and m.train_dense == "hip"
        m.train()
        assert m.train_dense == "hip"
        m.eval()
        assert m.train_dense == "hip" and copy.deepcopy(m).train_dense == "hip"
        for name in ("HIP", "cuda", "", None):
            with pytest.raises(ValueError):
                m.set_train_dense(name)
        assert m.train_dense == "hip"
        assert m.set_train_dense("torch") is m and m.train_dense == "torch" and m.set_train_dense().train_dense == "torch"


def test_torch_body_of_the_dispatch_is_the_literal_expression():
    """ParamTree._dense / _dense_ln in "torch" mode ARE the inline expressions the training forwards used to spell out: equal bytes
    for the outputs and for every input gradient under a fixed dy (CPU, fp32, R = 5, Cin = 8, Cout = 4)"""
    from deeppointmap_amd import ops
    from deeppointmap_amd.params import ParamTree
    m = ParamTree()
    assert m.train_dense == "torch"
    g = torch.Generator().manual_seed(5)
    t = dict(x=torch.randn(5, 8, generator=g), W=torch.randn(4, 8, generator=g), b=torch.randn(4, generator=g),
             gamma=torch.randn(4, generator=g), beta=torch.randn(4, generator=g), residual=torch.randn(5, 4, generator=g),
             post=torch.randn(5, 4, generator=g))
    dy = torch.randn(5, 4, generator=g)
    ln = lambda y, a: F.layer_norm(y, (4,), a["gamma"], a["beta"])   # noqa: E731
    forms = [
        ("x W b", lambda a: m._dense(a["x"], a["W"], a["b"]), lambda a: F.linear(a["x"], a["W"], a["b"])),
        ("x W b residual", lambda a: m._dense(a["x"], a["W"], a["b"], act=ops.ACT_RELU, residual=a["residual"]),
         lambda a: F.relu(F.linear(a["x"], a["W"], a["b"]) + a["residual"])),
        ("x W", lambda a: m._dense(a["x"], a["W"], None), lambda a: F.linear(a["x"], a["W"])),
        ("x W b gamma beta residual post",
         lambda a: m._dense_ln(a["x"], a["W"], a["b"], a["gamma"], a["beta"], residual=a["residual"], post=a["post"]),
         lambda a: ln(F.linear(a["x"], a["W"], a["b"]) + a["residual"], a) + a["post"]),
        ("x W b gamma beta post", lambda a: m._dense_ln(a["x"], a["W"], a["b"], a["gamma"], a["beta"], post=a["post"], act=ops.ACT_RELU),
         lambda a: F.relu(ln(F.linear(a["x"], a["W"], a["b"]), a) + a["post"])),
        ("x W b gamma beta", lambda a: m._dense_ln(a["x"], a["W"], a["b"], a["gamma"], a["beta"]),
         lambda a: ln(F.linear(a["x"], a["W"], a["b"]), a)),
    ]
    for names, got_f, want_f in forms:
        with torch.enable_grad():
            a = {k: t[k].clone().requires_grad_(True) for k in names.split()}
            b = {k: t[k].clone().requires_grad_(True) for k in names.split()}
            got, want = got_f(a), want_f(b)
            gg, gw = torch.autograd.grad(got, list(a.values()), dy), torch.autograd.grad(want, list(b.values()), dy)
        assert torch.equal(got, want), names
        for k, u, v in zip(a, gg, gw):
            assert torch.equal(u, v), (names, k)
