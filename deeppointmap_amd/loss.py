"""The training objectives of the reference for the MI355X: RegistrationLoss (network/loss.py) and the loop-detection
stage's binary cross-entropy with its metrics (pipeline/modules/model_pipeline.py:156-181, LoopDetectionLoss below).

The pairing terms run in csrc/reg_loss.hip: nearest neighbours, the InfoNCE forward of both directions and its analytic
backward, in strips of the similarity matrix that are recomputed rather than stored, so no (B, S, D) tensor exists in memory.
The offset term is K x 3 and stays torch, which makes its three modes and their gradients the reference's by construction.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch
from torch import Tensor, nn
from torch.autograd.function import once_differentiable

from . import ops


def _f32(t: Tensor) -> Tensor:
    return t.detach().to(torch.float32).contiguous()


class _PairingLoss(torch.autograd.Function):
    """(loss, stats) of one feature pair in both directions; loss is differentiable with respect to both features, stats (8,)
    is ops.reg_loss_forward's [loss, mean_src, mean_dst, n_src, n_dst, hits_src, hits_dst, 0]."""

    @staticmethod
    def forward(ctx, fea_a, fea_b, xyz_a, xyz_b, pad_a, pad_b, nn_a, nn_b, tau, eps, neutral):
        a, b = _f32(fea_a), _f32(fea_b)
        loss, stats, ws = ops.reg_loss_forward(a, b, xyz_a, xyz_b, pad_a, pad_b, nn_a, nn_b, tau, eps, neutral)
        ctx.save_for_backward(xyz_a, xyz_b, nn_a, nn_b)
        ctx.ws, ctx.stats = ws, stats
        ctx.shape = (a.shape[0], a.shape[1], a.shape[2], b.shape[2])
        ctx.dtypes = (fea_a.dtype, fea_b.dtype)
        ctx.cfg = (tau, eps, neutral)
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _grad_stats):
        xyz_a, xyz_b, nn_a, nn_b = ctx.saved_tensors
        tau, eps, neutral = ctx.cfg
        ga, gb = ops.reg_loss_backward(xyz_a, xyz_b, nn_a, nn_b, ctx.shape, tau, eps, neutral, _f32(grad_loss), ctx.stats,
                                       ctx.ws)
        return ga.to(ctx.dtypes[0]), gb.to(ctx.dtypes[1]), None, None, None, None, None, None, None, None, None


def _agree(xs: Tensor, xd: Tensor, ps: Tensor, pd: Tensor, feats) -> None:
    """the kernels index coordinates, masks and both feature pairs together: they must agree in B, S and D"""
    if xs.dim() != 3 or xd.dim() != 3 or xs.shape[1] != 3 or xd.shape[1] != 3 or xs.shape[0] != xd.shape[0]:
        raise ValueError(f"coordinates must be (B,3,S) / (B,3,D), got {tuple(xs.shape)} / {tuple(xd.shape)}")
    B, S, D = xs.shape[0], xs.shape[2], xd.shape[2]
    for name, t, want in (("src_padding_mask", ps, (B, S)), ("dst_padding_mask", pd, (B, D))):
        if tuple(t.shape) != want:
            raise ValueError(f"{name}: expected shape {want} from the coordinates, got {tuple(t.shape)}")
    for name, t, n in zip(("src_pairing_fea", "dst_pairing_fea", "src_coarse_pairing_fea", "dst_coarse_pairing_fea"), feats,
                          (S, D, S, D)):
        if t.dim() != 3 or t.shape[0] != B or t.shape[2] != n:
            raise ValueError(f"{name}: expected shape ({B}, C, {n}) from the coordinates, got {tuple(t.shape)}")


def _top1(hits: float, n: float) -> float:
    # the reference: torch.sum(bool) / max(n, 1.0) is an fp32 tensor, then .item()
    return float(np.float32(hits) / np.float32(max(n, 1.0)))


class RegistrationLoss(nn.Module):
    """L = lambda_p * L_p + lambda_c * L_c + lambda_o * L_o, the reference's objective (network/loss.py).

    forward(src_global_coor (B,3,S), dst_global_coor (B,3,D), src_padding_mask (B,S), dst_padding_mask (B,D),
    src_pairing_fea (B,C,S), dst_pairing_fea (B,C,D), src_coarse_pairing_fea (B,C',S), dst_coarse_pairing_fea (B,C',D),
    src_offset_res (K,3,1), dst_offset_res (K',3,1)) -> (loss, top1_acc, loss_p, loss_c, loss_o); padding masks are True on
    padding.  loss_p / loss_c are differentiable with respect to the four feature tensors, loss_o with respect to the offsets;
    the coordinates get no gradient.  top1_acc is a Python float.  Where neither direction has a positive row, the reference
    returns a Python 0 for that pairing term; here it is a 0-d zero tensor (with zero gradients).
    Everything is computed in fp32 (distances, masks and similarities included): fp16 / bf16 inputs are upcast and their
    gradients come back in the input dtype; fp64 inputs get fp32 masks and values, which can differ from the reference's fp64
    run for points within an fp32 rounding of eps_positive.  Tensors must be on the GPU and agree in B, S and D (ValueError
    otherwise); C and C' must be one of 64, 128, 192, 256 (ValueError otherwise).
    """

    def __init__(self, args):
        super().__init__()
        self.args = args
        self.loss_cfg = self.args.loss
        self.tau = self.loss_cfg.tau
        self.offset_value = self.loss_cfg.offset_value
        self.eps_positive = self.loss_cfg.eps_positive
        self.eps_offset = self.loss_cfg.eps_offset
        self.lambda_p = self.loss_cfg.lambda_p
        self.lambda_c = self.loss_cfg.lambda_c
        self.lambda_o = self.loss_cfg.lambda_o

    def forward(self, src_global_coor: Tensor, dst_global_coor: Tensor, src_padding_mask: Tensor, dst_padding_mask: Tensor,
                src_pairing_fea: Tensor, dst_pairing_fea: Tensor, src_coarse_pairing_fea: Tensor,
                dst_coarse_pairing_fea: Tensor, src_offset_res: Tensor, dst_offset_res: Tensor):
        xs, xd = _f32(src_global_coor), _f32(dst_global_coor)
        ps, pd = src_padding_mask.detach().bool().contiguous(), dst_padding_mask.detach().bool().contiguous()
        _agree(xs, xd, ps, pd, (src_pairing_fea, dst_pairing_fea, src_coarse_pairing_fea, dst_coarse_pairing_fea))
        nn_s, nn_d = ops.reg_loss_pairs(xs, xd, self.eps_positive)
        loss_p, st = _PairingLoss.apply(src_pairing_fea, dst_pairing_fea, xs, xd, ps, pd, nn_s, nn_d, self.tau,
                                        self.eps_positive, False)
        loss_c, _ = _PairingLoss.apply(src_coarse_pairing_fea, dst_coarse_pairing_fea, xs, xd, ps, pd, nn_s, nn_d, self.tau,
                                       self.eps_positive, True)
        loss_o = (self.offset_loss(src_offset_res.transpose(1, 2)) + self.offset_loss(dst_offset_res.transpose(1, 2))) / 2
        s = st.tolist()
        top1 = (_top1(s[5], s[3]) + _top1(s[6], s[4])) / 2
        loss = self.lambda_p * loss_p + self.lambda_c * loss_c + self.lambda_o * loss_o
        return loss, top1, loss_p, loss_c, loss_o

    @staticmethod
    def make_pairs(src_global_coor: Tensor, dst_global_coor: Tensor, dis_threshold: float) -> Tuple[Tensor, Tensor, Tensor]:
        """(B,S,3), (B,D,3) -> corr_ids (B,S) int64 (-1 where not corr), corr_mask (B,S), neutral_mask (B,S,D): the reference's
        contract, with the distances computed in fp32 whatever the input dtype (the precision forward uses; for fp64 inputs
        the reference computes in fp64, and masks can differ within an fp32 rounding of the threshold).  The dense neutral mask is built here only because it is this function's return value;
        RegistrationLoss.forward never builds it."""
        a, b = _f32(src_global_coor.transpose(1, 2)), _f32(dst_global_coor.transpose(1, 2))
        nn_a, _ = ops.reg_loss_pairs(a, b, dis_threshold)
        corr_ids = nn_a.long()
        corr_mask = corr_ids >= 0
        d = a.unsqueeze(3) - b.unsqueeze(2)                               # (B,3,S,D)
        dist2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        neutral = dist2 <= dis_threshold * dis_threshold
        bi, si = corr_mask.nonzero(as_tuple=True)
        neutral[bi, si, corr_ids[bi, si]] = False
        return corr_ids, corr_mask, neutral

    def offset_loss(self, src_offset_res: Tensor) -> Tensor:
        """(K,1,3) residuals -> mean of the per-row error ('manhattan' | 'euclidean' | 'mahalanobis'); 0 rows give 0."""
        r = src_offset_res.squeeze(1)
        if self.offset_value == "manhattan":
            err = r.abs().sum(dim=-1)
        elif self.offset_value == "euclidean":
            err = torch.norm(r, p=2, dim=-1)
        elif self.offset_value == "mahalanobis":
            try:
                cov_inv = torch.linalg.inv(torch.cov(r.detach().T))
            except Exception:   # a singular covariance: the identity, as the reference falls back
                cov_inv = torch.eye(3, device=r.device, dtype=r.dtype)
            err = torch.sqrt(torch.einsum("nj,jk,nk->n", r, cov_inv, r))
        else:
            raise ValueError(f"offset_value {self.offset_value!r}")
        return err.sum(dim=-1) / max(err.shape[0], 1.0)

    @staticmethod
    def eval_pairing_acc(src_pairing_fea: Tensor, dst_pairing_fea: Tensor, src_padding_mask: Tensor, corr_ids_src: Tensor,
                         corr_mask_src: Tensor) -> float:
        """(B,S,C), (B,D,C), valid mask (B,S) (True on real points, as the reference passes it), corr ids / mask (B,S) ->
        the fraction of valid corr rows whose most similar dst point (first on ties) is the correspondence."""
        a, b = _f32(src_pairing_fea.transpose(1, 2)), _f32(dst_pairing_fea.transpose(1, 2))
        B, _, S = a.shape
        D = b.shape[2]
        nn_a = torch.where(corr_mask_src.bool(), corr_ids_src.long(), -1).to(torch.int32).contiguous()
        pad_a = (~src_padding_mask.bool()).contiguous()
        nn_b = torch.full((B, D), -1, device=a.device, dtype=torch.int32)
        pad_b = torch.zeros(B, D, device=a.device, dtype=torch.bool)
        _, stats, _ = ops.reg_loss_forward(a, b, None, None, pad_a, pad_b, nn_a, nn_b, 1.0, 0.0, False)
        s = stats.tolist()
        return _top1(s[5], s[3])


class LoopDetectionLoss(nn.Module):
    """The objective of the reference's loop-detection stage (pipeline/modules/model_pipeline.py:156-181).

    forward(loop_pred (B,), src_T (B,3,1), dst_T (B,3,1)) -> (loss, metric_dict): a pair is a loop (label 1) when its two
    frames are at most `args.train.loop_detection.distance` apart, ||src_T - dst_T||_2 computed in fp32; loss is
    F.binary_cross_entropy(loop_pred, label), a 0-d tensor differentiable with respect to loop_pred (ops.loop_bce: loss,
    gradient seed and counts in one launch).  metric_dict holds Python floats under the reference's keys, from ONE
    device-to-host copy: `loss_loop`; `loop_precision`, which there is the share of pairs with prediction == label (the name is
    kept); `loop_recall`, 1.0 when no pair is a loop; `loop_false_positive`, 0.0 when every pair is one.  The prediction is
    loop_pred > 0.5."""

    def __init__(self, args):
        super().__init__()
        self.args = args
        self.distance = float(args.train.loop_detection.distance)

    def forward(self, loop_pred: Tensor, src_T: Tensor, dst_T: Tensor):
        if loop_pred.dim() != 1 or loop_pred.numel() < 1:
            raise ValueError(f"loop_pred must be (B,) with B >= 1, got {tuple(loop_pred.shape)}")
        B = loop_pred.numel()
        for name, t in (("src_T", src_T), ("dst_T", dst_T)):
            if tuple(t.shape) != (B, 3, 1):
                raise ValueError(f"{name}: expected shape ({B}, 3, 1), got {tuple(t.shape)}")
        dev = loop_pred.device
        dis = torch.norm((_f32(src_T).to(dev) - _f32(dst_T).to(dev)).squeeze(-1), p=2, dim=-1)
        loop_gt = (dis <= self.distance).float()
        pred = loop_pred if loop_pred.dtype == torch.float32 else loop_pred.float()
        loss, stats = ops.loop_bce(pred, loop_gt)
        s = stats.tolist()
        n_pos, n_neg, n_equal, true_pos, false_pos = s[1:6]
        ratio = lambda a, b: float(np.float32(a) / np.float32(b))   # noqa: E731  (the reference divides fp32 tensors)
        metric_dict = {
            "loss_loop": s[0],
            "loop_precision": ratio(n_equal, B),
            "loop_recall": ratio(true_pos, n_pos) if n_pos > 0 else 1.0,
            "loop_false_positive": ratio(false_pos, n_neg) if n_neg > 0 else 0.0,
        }
        return loss, metric_dict
