"""`Decoder` -- drop-in for the reference's network/decoder/decoder.py::Decoder (inference calls).

Same constructor (`Decoder(args)`), state-dict keys/shapes (params.decoder_shapes) and call
contracts:
  * `registration_forward(src_desc (131,M), dst_desc (131,N), src_padding_mask=None,
     dst_padding_mask=None, num_sample=0.5) -> (R (3,3), T (3,1), conf (K,), rmse: float)`
     (decoder.py:91-127); 3-D inputs give the batched return shapes of the reference.
  * `loop_detection_forward(src (C,131,M), dst (C,131,N)) -> (C,)` (decoder.py:129-143); in `.train()` at train stage
     "loop_detection" (`set_train_stage`) it is the reference's second training stage: the result carries the loop head's graph.
  * `forward(src_desc (B,131,M), dst_desc (B,131,N), src_padding_mask, dst_padding_mask, gt_Rt) -> [six tensors]`
     (decoder.py:34-89) is the training forward; it needs `.train()` and raises in eval mode as the reference does.
Padding masks ((B,M) / (B,N) bool, True = padding) are the key_padding_mask of every attention block and nothing else
(descriptor_attention.py:33-42), as in the reference; no inference call site of the reference passes any
(odometry.py:108-110, mapping.py:153-155, loop_closure.py:170-174,239-242).

All inference arithmetic runs in libdpm_hip.so (the training forward keeps its dense layers in torch under autograd unless
`set_train_dense("hip")` moves them to csrc/dense_train.hip, its attention cores and offset pairing in libdpm_hip.so); the module is re-entrant (no per-call state on self), so
the three SLAM threads of the reference can share one instance (system/core.py:55-57).
"""
from __future__ import annotations

import copy
import threading
from typing import Dict, Tuple, Union

import torch
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

from . import knobs, ops
from .params import ParamTree, decoder_shapes

HEADS = 8


class Decoder(ParamTree):
    def __init__(self, args):
        super().__init__(decoder_shapes(args))
        self.args = args
        self.decoder_cfg = args.decoder
        self.in_channel = self.decoder_cfg.in_channel
        self.model_channel = self.decoder_cfg.model_channel
        self.attention_layers = self.decoder_cfg.attention_layers
        self.tau = args.loss.tau
        self._dim_t: Dict[str, torch.Tensor] = {}
        self.fused_match = knobs.FUSED_MATCH   # similarity -> dual softmax -> top-k as one operator where it applies (ops.match_supported)
        self.stack_sides = True   # M != N: one launch per row-wise layer over both sides (False: the per-side loop)
        # pair lists over shared frames: per-frame work once per frame (False: per pair side, A/B runs)
        self.dedup_frames = knobs.DEDUP_FRAMES
        # One-pair registrations (the reference's own call: odometry.py:108-110, mapping.py:153-155, loop_closure.py:239-242)
        # are ~50 small launches whose enqueue takes longer than their execution.  A shape (M, N, k) that keeps coming back is
        # captured once as a HIP graph over static input / output buffers and replayed from then on: same kernels, same
        # launch arguments, bit-identical results, one host call.  Bounded: the least recently used graph gives its memory
        # back.  A capture is an event for the whole process on this runtime -- another thread that synchronises or allocates
        # meanwhile fails with "operation not permitted when stream is capturing" (measured with three threads on one
        # Decoder, in every capture mode) -- so shapes are only captured while the process has ONE Python thread: the
        # reference's single-thread SlamSystem.step, bench.py, the rank-0 consumer.  Its multi-thread mode (one Decoder
        # shared by the odometry / mapping / loop threads, core.py:55-57) replays what `capture_registration_graphs`
        # captured before the threads started, and launches every other shape eagerly.
        self.graph_min_hits = 2   # eager calls of a shape before it is captured (0 = never capture)
        self.graph_max = 6        # captured shapes kept per decoder
        self._graphs: Dict[tuple, dict] = {}
        self._graph_lock = threading.Lock()
        self._stamp_params = None
        # training forward: from this many stacked tokens (B * (M + N)) on, an attention layer's activations are recomputed in
        # the backward rather than kept (sixteen (tokens, model_channel) tensors per layer: 256 MiB per layer at 16384 tokens)
        self.train_checkpoint_rows = 8192
        self.eval()

    def __deepcopy__(self, memo):
        """copy.deepcopy(decoder) (infer_multiagents.py:100,112-113 makes one copy per agent): parameters and settings are
        copied, captured graphs and their lock are not -- a copy captures its own."""
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k == "_graphs":
                new.__dict__[k] = {}
            elif k == "_stamp_params":
                new.__dict__[k] = None
            elif k == "_graph_lock":
                new.__dict__[k] = threading.Lock()
            else:
                new.__dict__[k] = copy.deepcopy(v, memo)
        return new

    # -- helpers -------------------------------------------------------------------------------
    @property
    def device(self) -> torch.device:
        return self.p("projection.weight").device

    def _dimt(self, dev: torch.device) -> torch.Tensor:
        """temperature ** (2*(i//2)/F), evaluated with the reference's own torch expression
        (descriptor_attention.py:71-72) on the host, once per device."""
        key = str(dev)
        if key not in self._dim_t:
            F = self.model_channel // 3 // 2 * 2
            i = torch.arange(F, dtype=torch.float32)
            self._dim_t[key] = (10000 ** (2 * torch.div(i, 2, rounding_mode="trunc") / F)).to(dev)
        return self._dim_t[key]

    def _lin(self, key: str, x, act=ops.ACT_NONE, residual=None):
        return ops.linear(x, self.p(key + ".weight"), self.p(key + ".bias"), act=act, residual=residual)

    def _ln(self, key: str, x, post=None):
        return ops.layernorm(x, self.p(key + ".weight"), self.p(key + ".bias"), post=post)

    def _lin_ln(self, lin: str, ln: str, x, residual, post=None):
        """LN(x W^T + b + residual) (+ post): projection and LayerNorm in one kernel"""
        return ops.linear_layernorm(x, self.p(lin + ".weight"), self.p(lin + ".bias"), self.p(ln + ".weight"),
                                    self.p(ln + ".bias"), pre=residual, post=post)

    def _block_tail(self, pre: str, a, z1, post=None):
        """The tail of block `pre` (descriptor_attention.py:41-48) from the cross attention's output `a` and its query rows z1:
        z2 = LN2(a Wo^T + bo + z1), then LN3(mlp(z2) + z2) (+ post, the next block's position embedding) -- one kernel where
        ops.decoder_tail applies, otherwise its three launches (the same rows bit for bit)"""
        ca, n2, m0, m2, n3 = pre + ".cross_attn.out_proj", pre + ".norm2", pre + ".mlp.0", pre + ".mlp.2", pre + ".norm3"
        out = ops.decoder_tail(a, z1, self.p(ca + ".weight"), self.p(ca + ".bias"), self.p(n2 + ".weight"), self.p(n2 + ".bias"),
                               self.p(m0 + ".weight"), self.p(m0 + ".bias"), self.p(m2 + ".weight"), self.p(m2 + ".bias"),
                               self.p(n3 + ".weight"), self.p(n3 + ".bias"), post)
        if out is not None:
            return out
        z2 = self._lin_ln(ca, n2, a, z1)
        return self._lin_ln(m2, n3, self._lin(m0, z2, ops.ACT_RELU), z2, post)

    def _stage(self, desc: torch.Tensor, dev) -> Tuple[torch.Tensor, torch.Tensor, int, int]:
        """(B,131,M) any device -> token-major rows (B*M,131) on the GPU.  The rows are 132 floats apart: the 128 feature
        columns of every token start 16-byte aligned, which the projection GEMM's vector loads need (with rows of 131
        floats it took the scalar-load kernel: 34.6 against 13 us per 64-pair batch)."""
        d = desc.to(device=dev, dtype=torch.float32).contiguous()
        B, C, M = d.shape
        if C != self.in_channel + 3:
            raise ValueError(f"descriptor must have {self.in_channel + 3} rows, got {C}")
        t = ops.to_channel_first(d, row_multiple=4)           # (B,M,C) view of a (B,M,ld) buffer
        return t.as_strided((B * M, C), (t.stride(1), 1), t.storage_offset()), B, M

    def _attention_cores(self, pre: str, z, cross: bool, B, M, N=None, mask=None):
        """The q | k | v projection `pre` of the rows z and the attention cores on it -> (rows, E), before the out-projection.
        Self attention: every sequence attends itself; cross attention: its partner on the other side.

        N None: z holds B sequences of M tokens each (for cross attention sources then targets, the partner of sequence b being
        sequence (b + B/2) mod B), mask (B,M) uint8 = their key_padding_mask.  One launch: the projection writes the cores'
        operand planes where ops.qkv_attention applies (no mask, 32-wide heads, M % 64 == 0, enough rows), otherwise one
        projection and one core launch.
        N given: z = [B sequences of M tokens ; B sequences of N tokens], mask = (source (B,M), target (B,N)).  One projection
        over all rows and one core launch per side, writing into the row ranges of one output."""
        E = self.model_channel
        w, b = self.p(pre + ".in_proj_weight"), self.p(pre + ".in_proj_bias")
        if N is None:
            shift = B // 2 if cross else 0
            a = ops.qkv_attention(z, w, b, B, M, HEADS, kv_shift=shift) if mask is None else None
            if a is None:
                qkv = ops.linear(z, w, b)
                a = ops.attention(qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], B, M, M, HEADS, kv_shift=shift, key_mask=mask)
            return a
        ms, md = (None, None) if mask is None else mask
        qkv = ops.linear(z, w, b)
        a = torch.empty(z.shape[0], E, device=z.device, dtype=torch.float32)
        src, dst = slice(0, B * M), slice(B * M, None)
        # (cross: both directions read the pre-update tensors, descriptor_attention.py:41-44)
        for rows, keys, L, Lk, km in ((src, dst, M, N, md), (dst, src, N, M, ms)) if cross else ((src, src, M, M, ms), (dst, dst, N, N, md)):
            ops.attention(qkv[rows, :E], qkv[keys, E:2 * E], qkv[keys, 2 * E:], B, L, Lk, HEADS, out=a[rows], key_mask=km)
        return a

    def _descriptor_attention_forward(self, src_descriptor, dst_descriptor, src_padding_mask=None,
                                      dst_padding_mask=None):
        """-> (x (B*M,256), xyz_s (B*M,3) view, y (B*N,256), xyz_d view, B, M, N)   decoder.py:145-162.
        The padding masks (B,M) / (B,N) bool, True = padding, are the attention blocks' key_padding_mask and nothing else
        (descriptor_attention.py:33-42): padded tokens are still projected, normalised and offered to the pairing, as
        in the reference."""
        dev = self.device
        ts, B, M = self._stage(src_descriptor, dev)
        td, B2, N = self._stage(dst_descriptor, dev)
        if B != B2:
            raise ValueError("src and dst batch sizes differ")
        ms = md = None
        if src_padding_mask is not None or dst_padding_mask is not None:
            def as_mask(m, L):
                if m is None:
                    return torch.zeros(B, L, dtype=torch.uint8, device=dev)
                m = m.to(dev)
                if tuple(m.shape) != (B, L) or m.dtype != torch.bool:
                    raise ValueError(f"padding mask must be a bool tensor of shape ({B}, {L})")
                return m.contiguous().view(torch.uint8)
            ms, md = as_mask(src_padding_mask, M), as_mask(dst_padding_mask, N)
        C = self.in_channel
        xyz_s, xyz_d = ts[:, C:C + 3], td[:, C:C + 3]
        walk = self._attention_layers if M == N or self.stack_sides else self._attention_layers_per_side
        x, y = walk(ts, td, B, M, N, ms, md)
        return x, xyz_s, y, xyz_d, B, M, N

    def _attention_layers_per_side(self, ts, td, B, M, N, ms=None, md=None):
        """The plain form of the attention stack, one side at a time: what `_attention_layers` is held to bit for bit, at M == N
        as well (`stack_sides = False` runs it for M != N)."""
        C, E, dev = self.in_channel, self.model_channel, self.device
        ps, pd = ops.posemb(ts[:, C:C + 3], self._dimt(dev), E), ops.posemb(td[:, C:C + 3], self._dimt(dev), E)
        # x + pos enters every layer: fold the addition into the producing kernel's epilogue
        xp = ops.linear(ts[:, :C], self.p("projection.weight"), self.p("projection.bias"), residual=ps)
        yp = ops.linear(td[:, :C], self.p("projection.weight"), self.p("projection.bias"), residual=pd)

        def cross(pre, xq, xkv, L, Lk, mask):   # one direction: queries of one side, keys / values (and their mask) of the other
            w, b = self.p(pre + ".in_proj_weight"), self.p(pre + ".in_proj_bias")
            q = ops.linear(xq, w[:E], b[:E])
            kv = ops.linear(xkv, w[E:], b[E:])
            return ops.attention(q, kv[:, :E], kv[:, E:], B, L, Lk, HEADS, key_mask=mask)
        for l in range(self.attention_layers):
            pre = f"descriptor_attention.{l}"
            last = l == self.attention_layers - 1
            sa, ca = pre + ".self_attn", pre + ".cross_attn"
            # self attention: LN1(x + attn(x)), then + pos for the cross block   (descriptor_attention.py:31-40)
            x1 = self._lin_ln(sa + ".out_proj", pre + ".norm1", self._attention_cores(sa, xp, False, B, M, mask=ms), xp, ps)
            y1 = self._lin_ln(sa + ".out_proj", pre + ".norm1", self._attention_cores(sa, yp, False, B, N, mask=md), yp, pd)
            # cross attention, both directions read the pre-update tensors      (descriptor_attention.py:41-44)
            # ... LN2, then the MLP: LN3(mlp(x) + x); the next layer starts with + pos   (descriptor_attention.py:47-48)
            xp = self._block_tail(pre, cross(ca, x1, y1, M, N, md), x1, None if last else ps)
            yp = self._block_tail(pre, cross(ca, y1, x1, N, M, ms), y1, None if last else pd)
        return xp, yp

    def _attention_layers(self, ts, td, B, M, N, ms=None, md=None, first=None):
        """The attention stack (descriptor_attention.py:31-48) over the stacked rows [B*M source ; B*N target]: the layers share
        their weights between the sides, so every projection / LayerNorm / MLP is ONE launch over all rows -- the target side's
        launches of a scan-to-map pair (256 rows against 4096: pure launch latency) disappear -- and only the attention cores
        depend on the side sizes (`_attention_cores`: one launch over 2B sequences when M == N, one per side otherwise).
        Row-wise kernels give bit-identical rows whatever the row count, so the result equals `_attention_layers_per_side` bit
        for bit.  ms (B,M) / md (B,N) uint8: the sides' key_padding_mask.

        first = (pos, z1, a) from `_frame_prefix` (ts, td unused): the stacked position embedding, the first block's rows after
        norm1 and its cross-attention output (None: computed here from z1)."""
        C, E, dev = self.in_channel, self.model_channel, self.device
        seqs, Lt, mask = (2 * B, None, None if ms is None else torch.cat([ms, md])) if M == N else \
            (B, N, None if ms is None else (ms, md))
        if first is None:
            z_in = torch.cat([ts, td], dim=0)                       # [src tokens ; dst tokens]
            pos = ops.posemb(z_in[:, C:C + 3], self._dimt(dev), E)
            zp = ops.linear(z_in[:, :C], self.p("projection.weight"), self.p("projection.bias"), residual=pos)
        else:
            pos, z1, a = first
        for l in range(self.attention_layers):
            pre = f"descriptor_attention.{l}"
            last = l == self.attention_layers - 1
            sa, ca = pre + ".self_attn", pre + ".cross_attn"
            if l > 0 or first is None:
                z1 = self._lin_ln(sa + ".out_proj", pre + ".norm1", self._attention_cores(sa, zp, False, seqs, M, Lt, mask), zp, pos)
                a = None
            if a is None:
                a = self._attention_cores(ca, z1, True, seqs, M, Lt, mask)
            zp = self._block_tail(pre, a, z1, None if last else pos)
        return zp[:B * M], zp[B * M:]

    def _frame_prefix(self, tu, order, B, M):
        """What the first block computes from a frame alone, for pairs (frame order[p], frame order[B + p]) of the U distinct
        frames tu (U*M,131), once per frame (consecutive-frame odometry uses every frame twice) -> `first` of `_attention_layers`.
        Projection, position embedding and the first self-attention block; their rows are then gathered per pair.  The first
        cross-attention block's q | k | v projection sees the frame alone as well: the attention kernel picks a pair's sequences
        through `order` (row-wise kernels: the same rows bit for bit).  That kernel exists for 32-wide heads; other widths, and
        `dedup_frames = False`, project per pair side in the walk."""
        C, E, dev = self.in_channel, self.model_channel, self.device
        pos_u = ops.posemb(tu[:, C:C + 3], self._dimt(dev), E)
        zu = ops.linear(tu[:, :C], self.p("projection.weight"), self.p("projection.bias"), residual=pos_u)
        sa, ca = "descriptor_attention.0.self_attn", "descriptor_attention.0.cross_attn"
        z1u = self._lin_ln(sa + ".out_proj", "descriptor_attention.0.norm1",
                           self._attention_cores(sa, zu, False, tu.shape[0] // M, M), zu, pos_u)
        pos = ops.gather_frames(pos_u, order, M, E).view(2 * B * M, E)
        z1 = ops.gather_frames(z1u, order, M, E).view(2 * B * M, E)
        a = None
        if self.dedup_frames and E // HEADS == 32:
            w, b = self.p(ca + ".in_proj_weight"), self.p(ca + ".in_proj_bias")
            a = ops.qkv_attention(z1u, w, b, 2 * B, M, HEADS, kv_shift=B, seq_index=order)
            if a is None:
                qkv = ops.linear(z1u, w, b)
                a = ops.attention(qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:], 2 * B, M, M, HEADS, kv_shift=B, seq_index=order)
        return pos, z1, a

    # -- public API ----------------------------------------------------------------------------
    def train(self, mode: bool = True):
        """A real switch.  `.train()` selects the training mode of `self.train_stage`.  "registration" (the default; the
        reference's model_pipeline.py `registration()`): every parameter whose name does not contain `loop` gets
        requires_grad = True, so `forward` -> RegistrationLoss -> backward() fills their `.grad` and
        `torch.optim.*(decoder.parameters())` can step them; `loop_head` stays frozen.  "loop_detection" (`loop_detection()`
        there): exactly the eight `loop_head.*` tensors get requires_grad = True and `loop_detection_forward` returns a
        probability attached to the graph; everything else is frozen.  `.eval()` (what `__init__` ends in) turns requires_grad
        off again for all of them and drops the weight-derived caches.  In-place optimiser steps bump the parameters' version
        counters, which both the derived-weight cache (ops._derived) and the captured registration graphs (`_weights_stamp`)
        key on: inference after a step reads the new weights."""
        was = self.training
        super().train(mode)
        loop = self.train_stage == "loop_detection"
        for name, p in self._flat.items():
            p.requires_grad_(bool(mode) and (("loop" in name) == loop))
        if was and not mode:
            self.invalidate_caches()
        return self

    def _train_layer(self, l: int, z, pos, B: int, M: int, N: int, ms, md):
        """DescriptorAttentionLayer.forward (descriptor_attention.py:24-52) over the stacked rows [B*M source ; B*N target]:
        the four attention cores are ops.attention_train (HIP, forward and backward); the dense layers go through `_dense` /
        `_dense_ln`: the in-projections are plain products, each out-projection carries its residual, LayerNorm and (norm1) the
        position embedding of the next block, mlp.2 carries the residual and norm3."""
        E, R1 = self.model_channel, B * M
        pre = f"descriptor_attention.{l}"
        nrm = lambda n: (self.p(f"{pre}.{n}.weight"), self.p(f"{pre}.{n}.bias"))   # noqa: E731
        zp = z + pos
        qkv = self._dense(zp, self.p(pre + ".self_attn.in_proj_weight"), self.p(pre + ".self_attn.in_proj_bias"))
        a = torch.cat([ops.attention_train(qkv[:R1, :E], qkv[:R1, E:2 * E], qkv[:R1, 2 * E:], B, M, M, HEADS, ms),
                       ops.attention_train(qkv[R1:, :E], qkv[R1:, E:2 * E], qkv[R1:, 2 * E:], B, N, N, HEADS, md)])
        z1 = self._dense_ln(a, *self._w(pre + ".self_attn.out_proj"), *nrm("norm1"), residual=zp, post=pos)
        qkv = self._dense(z1, self.p(pre + ".cross_attn.in_proj_weight"), self.p(pre + ".cross_attn.in_proj_bias"))
        # both directions read the pre-update tensors (descriptor_attention.py:41-44)
        a = torch.cat([ops.attention_train(qkv[:R1, :E], qkv[R1:, E:2 * E], qkv[R1:, 2 * E:], B, M, N, HEADS, md),
                       ops.attention_train(qkv[R1:, :E], qkv[:R1, E:2 * E], qkv[:R1, 2 * E:], B, N, M, HEADS, ms)])
        z2 = self._dense_ln(a, *self._w(pre + ".cross_attn.out_proj"), *nrm("norm2"), residual=z1)
        u = self._dense(z2, *self._w(pre + ".mlp.0"), act=ops.ACT_RELU)
        return self._dense_ln(u, *self._w(pre + ".mlp.2"), *nrm("norm3"), residual=z2)

    def _dense2(self, x, first: str, second: str):
        """second(relu(first(x))): a two-layer head"""
        return self._dense(self._dense(x, *self._w(first), act=ops.ACT_RELU), *self._w(second))

    def forward(self, src_descriptor: torch.Tensor, dst_descriptor: torch.Tensor, src_padding_mask: torch.Tensor = None,
                dst_padding_mask: torch.Tensor = None, gt_Rt: Tuple[torch.Tensor, torch.Tensor] = None):
        """The reference's training forward (decoder.py:34-89), for a decoder in `.train()` mode on the GPU.

        src_descriptor (B, in_channel + 3, M), dst_descriptor (B, in_channel + 3, N); padding masks (B, M) / (B, N) bool,
        True = padding (None = no padding); gt_Rt = (R (B,3,3), T (B,3,1)), source -> target.  Returns the reference's list
        `[src_pairing_fea (B,E,M), dst_pairing_fea (B,E,N), src_coarse_pairing_fea (B,C,M), dst_coarse_pairing_fea (B,C,N),
        src_offset_res (K,3,1), dst_offset_res (K,3,1)]`, which `RegistrationLoss.forward` takes unchanged; K counts the
        (batch, src, dst) triples of unpadded tokens within `eps_offset` after the ground-truth transform, listed in
        torch.nonzero's order (K = 0 gives (0,3,1) residuals and zero gradients).

        Differentiable with respect to every parameter the reference's autograd reaches (all but `loop_head`) and to the first
        `in_channel` rows of both descriptors.  The three xyz rows get NO gradient (their `.grad` rows are zero): they are
        sampled input points with no parameter upstream; the reference does propagate into them (through the offset
        targets and the position embedding).

        The attention cores and the offset pairing run in csrc/attention_train.hip and csrc/offset_pairs.hip in both
        directions; no tensor of M x N elements exists in the forward, the saved state or the backward.  The dense layers
        (projections, LayerNorm, MLPs, heads) are torch operations under autograd, or, after `set_train_dense("hip")`,
        ops.dense_linear_train / ops.dense_linear_ln_train (csrc/dense_train.hip) in both directions.
        From `train_checkpoint_rows` stacked tokens (B * (M + N)) on, each attention layer is recomputed in the backward
        instead of keeping its sixteen activation tensors (torch.utils.checkpoint: the same kernels on the same inputs,
        identical bytes).  Raises AssertionError in eval mode and without gt_Rt, as the reference does; ValueError for
        descriptors, masks or poses of the wrong shape and for a head width other than 32."""
        assert self.training, "forward is not available during inference!"
        assert gt_Rt is not None, "gt_Rt must be provided during training"
        dev = self._require_gpu()
        C, E = self.in_channel, self.model_channel
        if E // HEADS != ops.ATTENTION_TRAIN_HEAD_DIM or E % HEADS:
            raise ValueError(f"Decoder.forward: model_channel {E} gives heads of width {E / HEADS:g}; the training attention "
                             f"kernels support width {ops.ATTENTION_TRAIN_HEAD_DIM} only (model_channel "
                             f"{ops.ATTENTION_TRAIN_HEAD_DIM * HEADS})")
        for name, d in (("src_descriptor", src_descriptor), ("dst_descriptor", dst_descriptor)):
            if d.dim() != 3 or d.shape[1] != C + 3:
                raise ValueError(f"{name} must be (B, {C + 3}, tokens), got {tuple(d.shape)}")
        src = src_descriptor.to(device=dev, dtype=torch.float32)
        dst = dst_descriptor.to(device=dev, dtype=torch.float32)
        B, _, M = src.shape
        N = dst.shape[2]
        if dst.shape[0] != B:
            raise ValueError("src and dst batch sizes differ")

        def as_mask(m, L, name):
            if m is None:
                return torch.zeros(B, L, dtype=torch.bool, device=dev)
            if tuple(m.shape) != (B, L) or m.dtype != torch.bool:
                raise ValueError(f"{name} must be a bool tensor of shape ({B}, {L})")
            return m.to(dev).contiguous()
        ps, pd = as_mask(src_padding_mask, M, "src_padding_mask"), as_mask(dst_padding_mask, N, "dst_padding_mask")
        gt_R, gt_T = gt_Rt
        if tuple(gt_R.shape) != (B, 3, 3) or tuple(gt_T.shape) != (B, 3, 1):
            raise ValueError(f"gt_Rt must be ((B,3,3), (B,3,1)) with B = {B}, got {tuple(gt_R.shape)}, {tuple(gt_T.shape)}")
        gt_R, gt_T = gt_R.detach().to(device=dev, dtype=torch.float32), gt_T.detach().to(device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            ms, md = ps.view(torch.uint8), pd.view(torch.uint8)
            R1 = B * M
            rows = torch.cat([src[:, :C].transpose(1, 2).reshape(R1, C), dst[:, :C].transpose(1, 2).reshape(B * N, C)])
            xyz_s, xyz_d = src[:, C:].detach(), dst[:, C:].detach()                      # (B,3,M), (B,3,N)
            xyz_rows = torch.cat([xyz_s.transpose(1, 2).reshape(R1, 3), xyz_d.transpose(1, 2).reshape(B * N, 3)])

            def split(t, ch):   # stacked rows -> the reference's (B,ch,M), (B,ch,N)
                return t[:R1].view(B, M, ch).transpose(1, 2), t[R1:].view(B, N, ch).transpose(1, 2)
            # unified descriptor -> coarse pairing feature                                  (decoder.py:46-48)
            coarse = self._dense2(rows, "coarse_pairing_head.0", "coarse_pairing_head.2")
            # unified descriptor -> correlated descriptor                                   (decoder.py:145-162)
            pos = ops.posemb(xyz_rows, self._dimt(dev), E)
            z = self._dense(rows, *self._w("projection"))
            recompute = B * (M + N) >= self.train_checkpoint_rows
            for l in range(self.attention_layers):
                if recompute:
                    z = checkpoint(self._train_layer, l, z, pos, B, M, N, ms, md, use_reentrant=False)
                else:
                    z = self._train_layer(l, z, pos, B, M, N, ms, md)
            # correlated descriptors -> similarity feature                                  (decoder.py:56-58)
            sim = self._dense2(z, "similarity_head.0", "similarity_head.2")
            # correlated descriptors -> offset                                              (decoder.py:60-86)
            src_gt = (gt_R @ xyz_s + gt_T).contiguous()
            pairs = ops.offset_pairs(src_gt, xyz_d.contiguous(), ps, pd, self.args.loss.eps_offset)
            xs, xd = ops.offset_pair_rows(z[:R1], z[R1:], pairs, M, N)
            bi, si, di = pairs[0].long().unbind(1)
            K = bi.numel()
            sp, dp = src_gt.transpose(1, 2)[bi, si], xyz_d.transpose(1, 2)[bi, di]         # (K,3) each, no gradient
            src_gt_off = gt_R[bi].transpose(1, 2) @ (dp - sp).unsqueeze(2)
            dst_gt_off = (sp - dp).unsqueeze(2)
            X = torch.cat([torch.cat([xs, xd], dim=1), torch.cat([xd, xs], dim=1)])        # (2K, 2E): src -> dst rows, then dst -> src
            # the skip connection is the residual of mlp.4, the ReLU after the sum its activation
            h = self._dense(self._dense(X, *self._w("offset_head.mlp.0"), act=ops.ACT_RELU),
                            *self._w("offset_head.mlp.2"), act=ops.ACT_RELU)
            h = self._dense(h, *self._w("offset_head.mlp.4"), act=ops.ACT_RELU,
                            residual=self._dense(X, *self._w("offset_head.downsample")))
            off = self._dense(h, *self._w("offset_head.head")).unsqueeze(2)                # (2K,3,1)
            return [*split(sim, E), *split(coarse, C), off[:K] - src_gt_off, off[K:] - dst_gt_off]

    @staticmethod
    def _num_pairs(num_sample, M: int, N: int) -> int:
        if isinstance(num_sample, int):
            k = num_sample
        elif isinstance(num_sample, float) and num_sample > 1:
            k = int(num_sample)
        elif isinstance(num_sample, float) and 0 < num_sample <= 1:
            k = int(num_sample * (M + N))
        else:
            raise ValueError(f"Argument `num_sample` with value {num_sample} is not supported")
        return k // 2

    def _register(self, src_descriptor, dst_descriptor, num_sample, header_out=None, trace: dict = None, pairs=None,
                  masks=(None, None)):
        """Batched core: (B,131,M), (B,131,N) -> result (B, 20+2k) on the device, nothing synchronises.
        Pairs are independent, so every kernel runs all B of them at once."""
        if pairs is not None:   # src_descriptor holds the U distinct frames, pairs = (sidx, didx) int32 on the device
            dev = self.device
            sidx, didx = pairs[0], pairs[1]
            # pairs may carry the concatenated index list (sources then targets) so that it is built once per pair list
            order = pairs[2] if len(pairs) > 2 else torch.cat([sidx, didx])
            tu, U, M = self._stage(src_descriptor, dev)
            N, B, C = M, sidx.numel(), self.in_channel
            x, y = self._attention_layers(None, None, B, M, N, first=self._frame_prefix(tu, order, B, M))
            xyz_sd = ops.gather_frames(tu, order, M, 3, ld=tu.stride(0), offset=C).view(2 * B * M, 3)
            xyz_s, xyz_d = xyz_sd[:B * M], xyz_sd[B * M:]
        else:
            x, xyz_s, y, xyz_d, B, M, N = self._descriptor_attention_forward(src_descriptor, dst_descriptor, *masks)
        E = self.model_channel
        k = self._num_pairs(num_sample, M, N)
        if k < 1:
            # fewer than two pairs requested (e.g. one token against one): the reference selects nothing, its Kabsch loop
            # averages an empty set and it returns NaN poses with no inliers (decoder.py:227-265) -- so do we
            res = torch.full((B, ops.RES_HDR), float("nan"), device=x.device, dtype=torch.float32)
            res[:, 13:16] = 0.0
            if header_out is not None:
                header_out.copy_(res)
            return res
        # similarity head -> L2 normalise -> M x N similarity -> dual softmax -> top-k   (decoder.py:181-191)
        if (M == N and x.is_contiguous() and y.is_contiguous() and
                x.untyped_storage().data_ptr() == y.untyped_storage().data_ptr() and
                y.storage_offset() == x.storage_offset() + x.numel()):
            # the attention walk left src and dst rows back to back: the head (shared weights, row-wise
            # kernels) runs once over both halves
            z = x.as_strided((2 * B * M, E), (E, 1), x.storage_offset())
            ab = ops.l2_normalize(self._lin("similarity_head.2", self._lin("similarity_head.0", z, ops.ACT_RELU)))
            a, b = ab[:B * M], ab[B * M:]
        else:
            a = ops.l2_normalize(self._lin("similarity_head.2", self._lin("similarity_head.0", x, ops.ACT_RELU)))
            b = ops.l2_normalize(self._lin("similarity_head.2", self._lin("similarity_head.0", y, ops.ACT_RELU)))
        if self.fused_match and ops.match_supported(M, N, E, k):
            # one operator, the M x N matrix never in memory (csrc/match.hip); the choice hangs on the pair's shape alone
            conf, flat = ops.match_topk(a.view(B, M, E), b.view(B, N, E), self.tau, k)
        else:
            S = ops.similarity_batched(a.view(B, M, E), b.view(B, N, E))
            conf, flat = ops.dual_softmax_topk(S, self.tau, k)
        # offset head on both pair directions                                           (decoder.py:204-207)
        X, si, di = ops.gather_pairs(x.view(B, M, E), y.view(B, N, E), flat)
        X = X.view(B * 2 * k, 2 * E)
        h = self._lin("offset_head.mlp.2", self._lin("offset_head.mlp.0", X, ops.ACT_RELU), ops.ACT_RELU)
        h = self._lin("offset_head.mlp.4", h, ops.ACT_RELU, residual=self._lin("offset_head.downsample", X))
        off = self._lin("offset_head.head", h)
        res = ops.corr_kabsch(off, xyz_s, xyz_d, si, di, conf, self.args.loss.eps_offset, header_out=header_out, batch=B)
        if trace is not None:
            trace.update(x=x, y=y, conf=conf, flat=flat, src_index=si, dst_index=di, offsets=off)
        return res.view(B, -1)

    @torch.no_grad()
    def registration_forward_batch(self, src_descriptor: torch.Tensor, dst_descriptor: torch.Tensor,
                                   num_sample: Union[int, float] = 0.5, header_out: torch.Tensor = None) -> torch.Tensor:
        """B independent pairs in one pass (not in the reference API; used by the frame-sharded hot path).
        -> result (B, 20+2k) on the device: per pair R(9) T(3) rmse n_corr n_inlier iters conf30 ..., then the
        inlier confidences.  No host synchronisation."""
        dev = self._require_gpu()
        with torch.cuda.device(dev):
            return self._register(src_descriptor, dst_descriptor, num_sample, header_out)

    @torch.no_grad()
    def registration_forward_pairs(self, descriptors: torch.Tensor, src_frame: torch.Tensor, dst_frame: torch.Tensor,
                                   num_sample: Union[int, float] = 0.5, header_out: torch.Tensor = None,
                                   order: torch.Tensor = None) -> torch.Tensor:
        """Like registration_forward_batch for pairs drawn from ONE set of frames: descriptors (F,131,M), pair p =
        (src_frame[p], dst_frame[p]) (int32 device tensors).  The per-frame part of the decoder (projection, position
        embedding, first self-attention block) runs once per frame instead of once per pair side; results are
        bit-identical to registration_forward_batch(descriptors[src_frame], descriptors[dst_frame])."""
        dev = self._require_gpu()
        with torch.cuda.device(dev):
            pairs = (src_frame, dst_frame) if order is None else (src_frame, dst_frame, order)
            return self._register(descriptors, None, num_sample, header_out, pairs=pairs)

    # -- captured one-pair registrations ---------------------------------------------------------
    def _weights_stamp(self):
        """What a captured graph hangs on: where the parameters live (`_epoch`: bumped by load_state_dict / .to() /
        invalidate_caches, ParamTree), their in-place version counters, and the generation of the weight-derived cache
        (ops.invalidate_derived frees tensors a graph might read).  Versions only on the per-call path: 13 us for the 82
        tensors against 42 us with a data_ptr() each.  Weights edited through `.data` need invalidate_caches(), as before."""
        if self._stamp_params is None:
            self._stamp_params = list(self._flat.values())
        return (self._epoch, ops.derived_generation(), tuple([p._version for p in self._stamp_params]))

    def _stale(self, key, e: dict, stamp=None) -> bool:
        """(under the lock) The one rule by which a graph of either kind is dropped: an entry whose graph was captured under
        another weights stamp (the weights moved or changed) leaves `_graphs` where it is found, and its graph, the graph's
        private pool and its static buffers are freed with it (a replay in flight on another thread keeps them until it ends)."""
        if e["graph"] is None or e["stamp"] == (self._weights_stamp() if stamp is None else stamp):
            return False
        del self._graphs[key]
        return True

    def captured(self, M: int, N: int) -> bool:
        """a live graph of an (M, N) registration exists: captured, of either kind, under the weights as they are now"""
        with self._graph_lock:
            stamp = self._weights_stamp()
            return any(k[:2] == (M, N) and v["graph"] is not None and v["stamp"] == stamp for k, v in self._graphs.items())

    def _graph_entry(self, key, M: int, N: int, num_sample, dev):
        """The calling thread's graph of shape `key`, captured now if the shape has been seen often enough; None = run eagerly."""
        with self._graph_lock:
            e = self._graphs.get(key)
            if e is None or self._stale(key, e):   # (a dropped graph leaves its hit count: the shape is captured again at once)
                e = self._graphs[key] = dict(hits=e["hits"] if e else 0, graph=None, used=0)
            e["hits"] += 1
            e["used"] = max((v["used"] for v in self._graphs.values()), default=0) + 1
            if e["graph"] is not None:
                return e
            if self.graph_min_hits <= 0 or e["hits"] <= self.graph_min_hits or threading.active_count() > 1:
                return None
            self._make_room()
        return self._capture(e, M, N, num_sample, dev)

    def _make_room(self):
        """(under the lock) drop the least recently used graph of the calling kind (its private pool is freed); graphs captured
        ahead of time by capture_registration_graphs are the caller's and stay"""
        live = [k for k, v in self._graphs.items() if v["graph"] is not None and not v.get("pinned")]
        if len(live) >= self.graph_max:
            old = min(live, key=lambda k: self._graphs[k]["used"])
            self._graphs.pop(old)

    def _capture(self, e: dict, M: int, N: int, num_sample, dev):
        src = torch.zeros(1, self.in_channel + 3, M, device=dev, dtype=torch.float32)
        dst = torch.zeros(1, self.in_channel + 3, N, device=dev, dtype=torch.float32)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=side, capture_error_mode="relaxed"):
                res = self._register(src, dst, num_sample)
        except Exception:  # noqa: BLE001  (a shape whose kernels cannot be captured keeps running eagerly)
            with self._graph_lock:
                e["hits"] = -(1 << 30)
            return None
        torch.cuda.current_stream(dev).wait_stream(side)
        e.update(graph=g, src=src, dst=dst, res=res, stamp=self._weights_stamp())
        return e

    @torch.no_grad()
    def capture_registration_graphs(self, shapes, copies: int = 1) -> int:
        """Capture the one-pair registration of every (M, N, num_sample) in `shapes` NOW, for replay from ANY thread -- what a caller
        that is about to start worker threads does first (the reference's multi-thread mode drives one Decoder from several threads,
        system/core.py:54-57, 82-109): on this runtime a capture in progress makes other threads' synchronising calls fail, so
        captures never happen once a second thread exists, and without this call such a process runs every registration eagerly
        (~51 launches, 0.86-1.0 ms of host time per 256 x 256 pair against 0.46 ms replayed).  Replays of one graph from different
        threads are put in order on the device (an event per graph), results are bit-identical to the eager path.  Returns the number
        of graphs captured.  Graphs captured here are not subject to `graph_max`.  After `invalidate_caches()` / new weights they
        are dropped by the rule of all graphs (`_stale`): the first registration that asks for the shape removes its stale instances
        from `_graphs`, which frees their graphs and buffers, and goes on as if none had been captured ahead -- unlike a thread's own
        graphs they are not captured again behind the caller's back: call this again (it captures what is missing or stale).
        `copies` > 1 captures that many instances per shape (each with its own static buffers): threads that ask for the same shape
        at the same time then replay different instances side by side on the device instead of queueing behind one."""
        dev = self._require_gpu()
        if threading.active_count() > 1:
            raise RuntimeError("capture_registration_graphs must run before the process starts its worker threads")
        n = 0
        with torch.cuda.device(dev):
            for M, N, num_sample in shapes:
                k = self._num_pairs(num_sample, M, N)
                if k < 1:
                    continue
                for c in range(max(1, int(copies))):
                    key = (M, N, k, dev.index, None, c)        # None: no owner thread; c: the instance
                    with self._graph_lock:
                        e = self._graphs.get(key)
                        if e is not None and e["graph"] is not None and not self._stale(key, e):
                            continue
                        e = self._graphs[key] = dict(hits=0, graph=None, used=0, pinned=True, lock=threading.Lock(), done=None)
                    if self._capture(e, M, N, num_sample, dev) is not None:
                        n += 1
        return n

    def _shared_graph(self, M: int, N: int, k: int, dev):
        """an instance of the ahead-of-time graph of this shape, LOCKED for the caller (an idle one if there is one, else the first)"""
        first, stamp, c = None, None, 0
        with self._graph_lock:
            while True:
                key = (M, N, k, dev.index, None, c)
                e = self._graphs.get(key)
                if e is None:
                    break
                if e["graph"] is not None:
                    stamp = self._weights_stamp() if stamp is None else stamp
                    if not self._stale(key, e, stamp):
                        if e["lock"].acquire(blocking=False):
                            return e
                        first = e if first is None else first
                c += 1
        if first is not None:
            first["lock"].acquire()
        return first

    @torch.no_grad()
    def registration_forward(self, src_descriptor: torch.Tensor, dst_descriptor: torch.Tensor,
                             src_padding_mask=None, dst_padding_mask=None,
                             num_sample: Union[int, float] = 0.5, trace: dict = None, header_out: torch.Tensor = None):
        dev = self._require_gpu()
        batch = not (src_descriptor.ndim == 2 and dst_descriptor.ndim == 2)
        if not batch:
            src_descriptor, dst_descriptor = src_descriptor.unsqueeze(0), dst_descriptor.unsqueeze(0)
        assert src_descriptor.shape[0] == 1, "batch size in inference must be 1"
        with torch.cuda.device(dev):
            entry = None
            plain = (src_padding_mask is None and dst_padding_mask is None and trace is None and header_out is None and
                     src_descriptor.ndim == 3 and dst_descriptor.ndim == 3 and dst_descriptor.shape[0] == 1 and
                     src_descriptor.shape[1] == self.in_channel + 3 == dst_descriptor.shape[1] and
                     isinstance(num_sample, (int, float)) and not torch.cuda.is_current_stream_capturing())
            if plain and self.graph_min_hits > 0:
                M, N = src_descriptor.shape[2], dst_descriptor.shape[2]
                k = self._num_pairs(num_sample, M, N)   # raises on an unsupported num_sample, as the eager path does
                if k >= 1:
                    entry = self._shared_graph(M, N, k, dev)    # captured ahead of time for every thread, or ...
                    if entry is None:                           # ... this thread's own, captured when the shape keeps coming back
                        entry = self._graph_entry((M, N, k, dev.index, threading.get_ident()), M, N, num_sample, dev)

            def replay():   # one sequence for both kinds of graph: inputs into the static buffers, replay, the result row out
                entry["src"].copy_(src_descriptor, non_blocking=True)
                entry["dst"].copy_(dst_descriptor, non_blocking=True)
                entry["graph"].replay()
                return entry["res"][0].clone()          # the static buffer belongs to the next replay
            if entry is None:
                res = self._register(src_descriptor, dst_descriptor, num_sample, header_out, trace,
                                     masks=(src_padding_mask, dst_padding_mask))[0]
            elif entry.get("lock") is None:
                res = replay()
            else:
                try:   # (locked by _shared_graph) one graph, several threads on their own streams: replays in order on the device too
                    st = torch.cuda.current_stream(dev)
                    if entry["done"] is not None:
                        st.wait_event(entry["done"])
                    res = replay()
                    entry["done"] = st.record_event()
                finally:
                    entry["lock"].release()
            head = res[:ops.RES_HDR].cpu()  # the one host sync of the call: rmse is a python float in the contract
        n_in, rmse = int(head[14]), float(head[12])
        R, T, cf = res[0:9].view(3, 3), res[9:12].view(3, 1), res[ops.RES_HDR:ops.RES_HDR + n_in]
        if trace is not None:
            trace.update(n_corr=int(head[13]), iterations=int(head[15]))
        if not batch:
            return R, T, cf, rmse
        return R.unsqueeze(0), T.unsqueeze(0), cf.unsqueeze(0), [rmse]

    def loop_detection_forward(self, src_descriptor: torch.Tensor, dst_descriptor: torch.Tensor,
                               src_padding_mask=None, dst_padding_mask=None) -> torch.Tensor:
        """(C,131,M), (C,131,N) -> loop probabilities (C,)   (decoder.py:129-143).

        Inference everywhere but in one situation: a decoder in `.train()` mode at stage "loop_detection"
        (`set_train_stage`), called with grad mode enabled, returns the probabilities attached to the autograd graph of the
        eight `loop_head.*` parameters -- the reference's second training stage (model_pipeline.py:136-181).  The attention
        trunk is frozen there and runs on the inference kernels without a graph; the head's token-sized layer is
        ops.loop_pool (csrc/loop_head_train.hip, forward and backward), its (C, 2 E)-sized layers are torch operations under
        autograd.  The descriptors get NO gradient in that mode: nothing upstream of the head is trainable in this stage."""
        dev = self._require_gpu()
        if src_descriptor.ndim == 2 and dst_descriptor.ndim == 2:
            src_descriptor, dst_descriptor = src_descriptor.unsqueeze(0), dst_descriptor.unsqueeze(0)
        E = self.model_channel
        train_head = self.training and self.train_stage == "loop_detection" and torch.is_grad_enabled()
        with torch.no_grad(), torch.cuda.device(dev):
            x, _, y, _, B, M, N = self._descriptor_attention_forward(src_descriptor, dst_descriptor,
                                                                     src_padding_mask, dst_padding_mask)
            if not train_head:
                fx = self._lin("loop_head.mlp.2", self._lin("loop_head.mlp.0", x, ops.ACT_RELU))
                fy = self._lin("loop_head.mlp.2", self._lin("loop_head.mlp.0", y, ops.ACT_RELU))
                cat = torch.empty(B, 2 * E, device=dev, dtype=torch.float32)
                ops.mean_rows(fx.view(B, M, E), cat[:, :E])
                ops.mean_rows(fy.view(B, N, E), cat[:, E:])
                h = self._lin("loop_head.projection.0", cat, ops.ACT_RELU)
                return self._lin("loop_head.projection.2", h, ops.ACT_SIGMOID).flatten()
        with torch.cuda.device(dev):
            return self._loop_head_train(x, y, B, M, N)

    def _loop_head_train(self, x: torch.Tensor, y: torch.Tensor, B: int, M: int, N: int) -> torch.Tensor:
        """OverlapHead (heads.py:60-69) under autograd on correlated features x (B*M,E), y (B*N,E) that carry no graph: the mean
        over the tokens (padding included, heads.py:65-66) of mlp.0 + ReLU is ops.loop_pool, then mlp.2 acts on the means --
        the second convolution is affine and commutes with the mean -- and the projection on (B, 2 E) rows"""
        W1, b1 = self._w("loop_head.mlp.0")
        m = torch.cat([ops.loop_pool(x, B, M, W1, b1), ops.loop_pool(y, B, N, W1, b1)])      # (2B, E)
        f = F.linear(m, *self._w("loop_head.mlp.2"))
        h = F.relu(F.linear(torch.cat([f[:B], f[B:]], dim=1), *self._w("loop_head.projection.0")))
        return torch.sigmoid(F.linear(h, *self._w("loop_head.projection.2"))).flatten()
