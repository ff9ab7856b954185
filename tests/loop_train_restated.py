"""One step of the loop-detection training stage restated in plain torch: the frozen attention trunk (as in
decoder_train_restated), the loop head, the binary cross-entropy and the reference's metrics; dense, differentiable by autograd,
any device and dtype.

Written from the contract (Decoder.loop_detection_forward's and LoopDetectionLoss's docstrings, include/dpm_hip.h): the
comparator of the HIP path where the reference does not exist (the GPU tests, scripts/loop_train_bench.py), itself pinned to
the reference's recorded answers by tests/test_loop_train_host.py.  It builds what the HIP path must not: the (B, L, E)
activations of the head's first layer.  Weights come as a state dict `sd` {name: tensor}; everything runs in their dtype.
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_train_restated as R  # noqa: E402


def loop_pool(x, W1, b1):
    """x (B,L,E) -> (B,E): mean over ALL L tokens of relu(x W1^T + b1)"""
    return F.relu(F.linear(x, W1, b1)).mean(dim=1)


def loop_head(sd, x, y):
    """OverlapHead: x (B,M,E), y (B,N,E) -> (B,) probabilities; per side Conv1d -> ReLU -> Conv1d, then the mean over the tokens
    (padded ones included)"""
    side = lambda t: R._lin(sd, "loop_head.mlp.2", F.relu(R._lin(sd, "loop_head.mlp.0", t))).mean(dim=1)   # noqa: E731
    h = F.relu(R._lin(sd, "loop_head.projection.0", torch.cat([side(x), side(y)], dim=-1)))
    return torch.sigmoid(R._lin(sd, "loop_head.projection.2", h)).flatten()


def trunk(sd, cfg, src, dst, ps, pd):
    """descriptors (B,C+3,M) / (B,C+3,N), padding masks bool -> correlated features x (B,M,E), y (B,N,E)"""
    C, E = cfg.decoder.in_channel, cfg.decoder.model_channel
    fs, fd = src[:, :C].transpose(1, 2), dst[:, :C].transpose(1, 2)
    return R.attention_layers(sd, cfg.decoder.attention_layers, R._lin(sd, "projection", fs), R._lin(sd, "projection", fd),
                              R.posemb(src[:, C:], E), R.posemb(dst[:, C:], E), ps, pd)


def labels(src_T, dst_T, distance):
    """(B,3,1) frame positions -> (B,) bool: at most `distance` apart"""
    return torch.norm((src_T - dst_T).squeeze(-1), p=2, dim=-1) <= distance


def loop_loss(pred, gt):
    """pred (B,) probabilities, gt (B,) bool -> (loss, metrics): mean binary cross-entropy with both logarithms clamped at -100;
    loop_precision is the share of pred == gt (the reference's name), loop_recall 1.0 without a positive, loop_false_positive
    0.0 without a negative; ratios are fp32 divisions, as the reference's"""
    y = gt.to(pred.dtype)
    loss = -(y * torch.log(pred).clamp(min=-100) + (1 - y) * torch.log1p(-pred).clamp(min=-100)).mean()
    hit = pred.detach() > 0.5
    ratio = lambda a, b: (torch.as_tensor(float(a), dtype=torch.float32) / torch.as_tensor(float(b), dtype=torch.float32)).item()   # noqa: E731
    n_pos, n_neg = int(gt.sum()), int((~gt).sum())
    metrics = {"loss_loop": loss.item(), "loop_precision": ratio(int((hit == gt).sum()), gt.numel()),
               "loop_recall": ratio(int(hit[gt].sum()), n_pos) if n_pos else 1.0,
               "loop_false_positive": ratio(int(hit[~gt].sum()), n_neg) if n_neg else 0.0}
    return loss, metrics


def training_step(sd, cfg, src, dst, ps, pd, src_T, dst_T):
    """-> (loss, prob (B,), metrics): the trunk without a graph (frozen in this stage), the head under autograd"""
    with torch.no_grad():
        x, y = trunk(sd, cfg, src, dst, ps, pd)
    prob = loop_head(sd, x, y)
    loss, metrics = loop_loss(prob, labels(src_T, dst_T, cfg.train.loop_detection.distance))
    return loss, prob, metrics
