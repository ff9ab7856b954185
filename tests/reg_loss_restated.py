"""RegistrationLoss restated in plain torch: dense, differentiable by autograd, any device and dtype.

The comparator of the fused loss where the reference does not exist (the GPU tests, scripts/reg_loss_bench.py), itself pinned
to the reference's recorded answers by tests/test_reg_loss_host.py.  Squared distances are summed in the reference CPU order
((dx dx + dy dy) + dz dz, one rounding per operation), so its masks equal the reference's on any device.
"""
import torch


def pairs(xa, xb, eps):
    """xa (B,3,M), xb (B,3,N) -> dist2 (B,M,N), nn (B,M) int64 (-1 where the nearest squared distance exceeds eps^2)"""
    d = xa.unsqueeze(3) - xb.unsqueeze(2)
    dist2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    best, idx = dist2.min(dim=2)
    return dist2, torch.where(best <= eps * eps, idx, torch.full_like(idx, -1))


def _unit(x):
    return x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)


def infonce(fa, fb, pad_a, nn, tau, near=None):
    """mean over the rows of a that are not padding and have a partner of logsumexp_j z_ij - z_i,nn(i), z = a^ b^ / tau;
    near (B,M,N): entries dropped from the softmax (except the row's partner).  0 without such rows."""
    z = torch.einsum("bcm,bcn->bmn", _unit(fa), _unit(fb)) / tau
    cols = torch.arange(z.shape[2], device=z.device)
    if near is not None:
        z = z.masked_fill(near & (cols != nn.unsqueeze(2)), float("-inf"))
    rows = (nn >= 0) & ~pad_a
    label = z.gather(2, nn.clamp_min(0).unsqueeze(2)).squeeze(2)
    per_row = torch.logsumexp(z, dim=2) - label
    return per_row[rows].sum() / rows.sum().clamp_min(1)


def top1(fa, fb, pad_a, nn):
    """(argmax_j a^ . b^ (B,M), fraction of counted rows where it is the partner, as the reference's fp32 .item())"""
    am = torch.einsum("bcm,bcn->bmn", _unit(fa), _unit(fb)).argmax(dim=2)
    rows = (nn >= 0) & ~pad_a
    hits = ((am == nn) & rows).sum()
    return am, float(hits.float() / max(int(rows.sum()), 1.0))


def offset(r, mode):
    """(K,3,1) -> mean per-row error"""
    r = r.transpose(1, 2).squeeze(1)
    if mode == "manhattan":
        e = r.abs().sum(-1)
    elif mode == "euclidean":
        e = r.pow(2).sum(-1).sqrt()
    else:
        try:
            ci = torch.linalg.inv(torch.cov(r.detach().T))
        except Exception:
            ci = torch.eye(3, dtype=r.dtype, device=r.device)
        e = ((r @ ci) * r).sum(-1).sqrt()
    return e.sum() / max(e.shape[0], 1.0)


def registration_loss(xs, xd, ps, pd, fs, fd, cs, cd, os_, od, cfg):
    """the five outputs of RegistrationLoss.forward plus a dict of what the tests compare row by row"""
    L = cfg.loss
    d2, nn_s = pairs(xs, xd, L.eps_positive)
    _, nn_d = pairs(xd, xs, L.eps_positive)
    near = d2 <= L.eps_positive * L.eps_positive
    lp = (infonce(fs, fd, ps, nn_s, L.tau) + infonce(fd, fs, pd, nn_d, L.tau)) / 2
    lc = (infonce(cs, cd, ps, nn_s, L.tau, near) + infonce(cd, cs, pd, nn_d, L.tau, near.transpose(1, 2))) / 2
    lo = (offset(os_, L.offset_value) + offset(od, L.offset_value)) / 2
    am_s, acc_s = top1(fs, fd, ps, nn_s)
    am_d, acc_d = top1(fd, fs, pd, nn_d)
    loss = L.lambda_p * lp + L.lambda_c * lc + L.lambda_o * lo
    extra = dict(nn_s=nn_s, nn_d=nn_d, neutral_s=near.sum(2) - (nn_s >= 0).long(),
                 neutral_d=near.sum(1) - (nn_d >= 0).long(), argmax_s=am_s, argmax_d=am_d)
    return (loss, (acc_s + acc_d) / 2, lp, lc, lo), extra
