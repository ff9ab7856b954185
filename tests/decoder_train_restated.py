"""The decoder's training forward (+ RegistrationLoss) restated in plain torch: dense, differentiable by autograd, any device
and dtype.

Written from the contract (Decoder.forward's docstring, include/dpm_hip.h): the comparator of the HIP path where the
reference does not exist (the GPU tests, scripts/decoder_train_bench.py), itself pinned to the reference's recorded answers by
tests/test_decoder_train_host.py.  It builds what the HIP path must not: the (B, heads, M, N) probabilities of every attention
block and the (B, M, N) distance matrix.  Weights come as a state dict `sd` {name: tensor}; everything runs in their dtype.
"""
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reg_loss_restated  # noqa: E402

HEADS = 8


def posemb(xyz, E):
    """xyz (B,3,M) -> (B,M,E): per coordinate F = E // 3 // 2 * 2 channels sin / cos interleaved of pi x / 10000^(2 (i // 2) / F),
    zero padded to E"""
    Fq = E // 3 // 2 * 2
    i = torch.arange(Fq, dtype=xyz.dtype, device=xyz.device)
    dim_t = 10000 ** (2 * torch.div(i, 2, rounding_mode="trunc") / Fq)
    p = (xyz.transpose(1, 2) * math.pi).unsqueeze(-1) / dim_t                      # (B,M,3,F)
    emb = torch.stack([p[..., 0::2].sin(), p[..., 1::2].cos()], dim=-1).reshape(*p.shape[:2], -1)
    return F.pad(emb, (0, E - emb.shape[-1]))


def mha(sd, pre, xq, xkv, key_pad):
    """nn.MultiheadAttention(batch_first, dropout 0): xq (B,M,E), xkv (B,N,E), key_pad (B,N) bool -> (B,M,E), dense"""
    B, M, E = xq.shape
    N, d = xkv.shape[1], E // HEADS
    w, b = sd[pre + ".in_proj_weight"], sd[pre + ".in_proj_bias"]
    q = F.linear(xq, w[:E], b[:E]).view(B, M, HEADS, d).transpose(1, 2)
    k = F.linear(xkv, w[E:2 * E], b[E:2 * E]).view(B, N, HEADS, d).transpose(1, 2)
    v = F.linear(xkv, w[2 * E:], b[2 * E:]).view(B, N, HEADS, d).transpose(1, 2)
    s = q @ k.transpose(-1, -2) / math.sqrt(d)                                       # (B,heads,M,N)
    s = s.masked_fill(key_pad[:, None, None, :], float("-inf"))
    o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, M, E)
    return F.linear(o, sd[pre + ".out_proj.weight"], sd[pre + ".out_proj.bias"])


def _lin(sd, key, x):
    w = sd[key + ".weight"]
    return F.linear(x, w.reshape(w.shape[0], w.shape[1]), sd[key + ".bias"])


def _ln(sd, key, x):
    return F.layer_norm(x, (x.shape[-1],), sd[key + ".weight"], sd[key + ".bias"])


def attention_layers(sd, layers, x, y, pos_x, pos_y, ps, pd):
    for l in range(layers):
        pre = f"descriptor_attention.{l}"
        x, y = x + pos_x, y + pos_y
        x = _ln(sd, pre + ".norm1", x + mha(sd, pre + ".self_attn", x, x, ps))
        y = _ln(sd, pre + ".norm1", y + mha(sd, pre + ".self_attn", y, y, pd))
        x, y = x + pos_x, y + pos_y
        x2 = _ln(sd, pre + ".norm2", x + mha(sd, pre + ".cross_attn", x, y, pd))
        y2 = _ln(sd, pre + ".norm2", y + mha(sd, pre + ".cross_attn", y, x, ps))
        x = _ln(sd, pre + ".norm3", _lin(sd, pre + ".mlp.2", F.relu(_lin(sd, pre + ".mlp.0", x2))) + x2)
        y = _ln(sd, pre + ".norm3", _lin(sd, pre + ".mlp.2", F.relu(_lin(sd, pre + ".mlp.0", y2))) + y2)
    return x, y


def offset_pairs(src_gt, xyz_d, ps, pd, eps):
    """(B,3,M), (B,3,N) -> (K,3) int64 (batch, src, dst), lexicographic; squared distances as (dx dx + dy dy) + dz dz"""
    d = src_gt.unsqueeze(3) - xyz_d.unsqueeze(2)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return torch.nonzero((d2 <= eps * eps) & ~ps.unsqueeze(2) & ~pd.unsqueeze(1))


def _offset_head(sd, X):
    h = _lin(sd, "offset_head.mlp.4", F.relu(_lin(sd, "offset_head.mlp.2", F.relu(_lin(sd, "offset_head.mlp.0", X)))))
    return _lin(sd, "offset_head.head", F.relu(h + _lin(sd, "offset_head.downsample", X)))


def decoder_forward(sd, cfg, src, dst, ps, pd, R, T, xyz_grad=False):
    """-> ([src_pairing (B,E,M), dst_pairing (B,E,N), src_coarse (B,C,M), dst_coarse (B,C,N), src_res (K,3,1), dst_res (K,3,1)],
    pairs (K,3)).  ps / pd (B,M) / (B,N) bool.  xyz_grad False: the coordinates are constants, as in the HIP path."""
    C, E = cfg.decoder.in_channel, cfg.decoder.model_channel
    fs, fd = src[:, :C].transpose(1, 2), dst[:, :C].transpose(1, 2)                   # (B,M,C)
    xs, xd = src[:, C:], dst[:, C:]
    if not xyz_grad:
        xs, xd = xs.detach(), xd.detach()
    coarse = lambda t: _lin(sd, "coarse_pairing_head.2", F.relu(_lin(sd, "coarse_pairing_head.0", t)))   # noqa: E731
    x, y = attention_layers(sd, cfg.decoder.attention_layers, _lin(sd, "projection", fs), _lin(sd, "projection", fd),
                            posemb(xs, E), posemb(xd, E), ps, pd)
    sim = lambda t: _lin(sd, "similarity_head.2", F.relu(_lin(sd, "similarity_head.0", t)))   # noqa: E731
    src_gt = R @ xs + T
    pairs = offset_pairs(src_gt.detach(), xd.detach(), ps, pd, cfg.loss.eps_offset)
    b, i, j = pairs.unbind(1)
    sp, dp = src_gt.transpose(1, 2)[b, i], xd.transpose(1, 2)[b, j]
    fx, fy = x[b, i], y[b, j]
    src_res = _offset_head(sd, torch.cat([fx, fy], 1)).unsqueeze(2) - R[b].transpose(1, 2) @ (dp - sp).unsqueeze(2)
    dst_res = _offset_head(sd, torch.cat([fy, fx], 1)).unsqueeze(2) - (sp - dp).unsqueeze(2)
    outs = [sim(x).transpose(1, 2), sim(y).transpose(1, 2), coarse(fs).transpose(1, 2), coarse(fd).transpose(1, 2), src_res, dst_res]
    return outs, pairs


def training_step(sd, cfg, src, dst, ps, pd, R, T):
    """Decoder.forward -> RegistrationLoss (model_pipeline.py:104-123) -> (loss, outs, pairs); the loss pairs the global
    coordinates R src + T against dst"""
    C = cfg.decoder.in_channel
    outs, pairs = decoder_forward(sd, cfg, src, dst, ps, pd, R, T)
    xs_global = (R @ src[:, C:] + T).detach()
    vals, _ = reg_loss_restated.registration_loss(xs_global, dst[:, C:].detach(), ps, pd, *outs, cfg)
    return vals[0], outs, pairs
