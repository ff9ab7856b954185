"""The training primitive of csrc/dense_train.hip restated in plain torch, in whatever dtype the operands have:

    plain:   out = act(x W^T + bias + residual)
    normed:  h = x W^T + bias + residual;  out = act(LN(h) * gamma + beta + post)      (eps 1e-5, biased variance)

The ReLU is an INPUT here: `mask` (bool, the shape of the output; None = no activation) multiplies the pre-activation, so that two
evaluations in different precisions can be compared on the same piecewise-linear branch.  tests/test_dense_train_host.py pins this
to F.linear / F.layer_norm / F.relu with the mask taken from its own forward.
"""
import torch

EPS = 1e-5


def plain(x, W, bias=None, residual=None, mask=None):
    """-> (out, pre): pre = x W^T + bias + residual, out = pre * mask (pre itself for mask None)"""
    pre = x @ W.transpose(0, 1)
    if bias is not None:
        pre = pre + bias
    if residual is not None:
        pre = pre + residual
    return (pre if mask is None else pre * mask.to(pre.dtype)), pre


def normed(x, W, bias, gamma, beta, residual=None, post=None, mask=None):
    """-> (out, pre, h): h the pre-norm rows, pre = LN(h) * gamma + beta + post, out = pre * mask (pre itself for mask None)"""
    _, h = plain(x, W, bias, residual)
    mean = h.mean(-1, keepdim=True)
    var = ((h - mean) ** 2).mean(-1, keepdim=True)
    pre = (h - mean) / torch.sqrt(var + EPS) * gamma + beta
    if post is not None:
        pre = pre + post
    return (pre if mask is None else pre * mask.to(pre.dtype)), pre, h


def make_case(R, Cin, Cout, seed, ldw=None, x_in=None):
    """The seeded operands of the GPU tests (fp32, CPU): x ~ N(0,1), W ~ N(0,1) / sqrt(Cin), bias and beta ~ 0.1 N, gamma ~
    1 + 0.1 N, residual, post and dy ~ N(0,1).  ldw: W is the first Cin columns of a (Cout, ldw) buffer; x_in = (width, offset): x
    is columns [offset, offset + Cin) of an (R, width) buffer."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)   # noqa: E731
    xb = rn(R, Cin if x_in is None else x_in[0])
    Wb = rn(Cout, Cin if ldw is None else ldw) / Cin ** 0.5
    return dict(x=xb if x_in is None else xb[:, x_in[1]:x_in[1] + Cin], W=Wb[:, :Cin], bias=0.1 * rn(Cout), gamma=1 + 0.1 * rn(Cout),
                beta=0.1 * rn(Cout), residual=rn(R, Cout), post=rn(R, Cout), dy=rn(R, Cout))
