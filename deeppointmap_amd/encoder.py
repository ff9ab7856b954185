"""`Encoder` -- drop-in for the reference's network/encoder/encoder.py::Encoder.

Same constructor (`Encoder(args)`), same state-dict keys/shapes (params.encoder_shapes), same
call contract: `encoder(points (B,C>=3,N) f32, points_padding (B,N) bool) ->
[coor (B,3,S), fea (B,out_channel,S), padding (B,S)]` (encoder.py:51-69).  Inputs may arrive on
the CPU (ScanPack keeps CPU tensors, system/modules/pose_graph.py:43-45); they are staged to the
module's GPU.  All inference arithmetic runs in libdpm_hip.so; there is no torch fallback.  In `.train()` mode the same
call is the reference's training forward: `fea` carries the autograd graph, the grouping layers run in csrc/group_train.hip in
both directions and the dense layers are torch operations under autograd or, after `set_train_dense("hip")`, the kernels of
csrc/dense_train.hip (`Encoder.train`, `Encoder._forward_train`).

Internally everything is point-major fp32 with a per-frame valid length (valid points lead,
exactly what the reference's FPS assumes, utils.py:255).
"""
from __future__ import annotations

from typing import List, Optional

import torch
from torch.utils.checkpoint import checkpoint

from . import ops
from .params import ParamTree, encoder_shapes


class Encoder(ParamTree):
    def __init__(self, args):
        super().__init__(encoder_shapes(args))
        self.args = args
        self.encoder_cfg = args.encoder
        self.in_channel = self.encoder_cfg.in_channel
        self.out_channel = self.encoder_cfg.out_channel
        self.downsample_layers = len(self.encoder_cfg.npoint)
        self.upsample_layers = self.encoder_cfg.upsample_layers
        for s in self.encoder_cfg.sample:
            if s["type"] not in ("fps", "fps-t3d", "voxel"):  # pointnext.py:21
                raise ValueError(f"{dict(s)} is not a supported sampling way, please use 'fps' or 'voxel'")
            if s["type"] == "voxel" and not ("size" in s and "range" in s):  # pointnext.py:30-31
                raise ValueError("a voxel sampler needs 'size' and 'range'")
        self.all_fps = all(s["type"] != "voxel" for s in self.encoder_cfg.sample)
        # Farthest point sampling is nested: level i+1 samples the level-i picks starting from the same first point,
        # and the k-th level-i pick is the farthest of ALL level-(i-1) points from the picks before it -- in
        # particular the farthest among the level-i picks themselves -- so level i+1 reproduces the level-i pick
        # ORDER: its result is the first npoint[i+1] picks of level i (ties included: the first-index rule on
        # positions agrees with the pick order).  Only the first level is computed; False runs every level
        # (tests assert both give identical tensors).
        self.nested_fps = self.all_fps and all(b <= a for a, b in zip(self.encoder_cfg.npoint, self.encoder_cfg.npoint[1:]))
        # Neighbour queries repeat: a SetAbstraction asks, for the FPS-picked subset of a level's points, exactly what the preceding
        # LocalAggregation answered for ALL of them when radius and K coincide (they do in every shipped config), and consecutive
        # LocalAggregations of a stage may share (radius, K) too.  The plan, per downsampling level: sa = the SetAbstraction's
        # (radius, K), answered = the previous level's LocalAggregations hold it, la = the distinct LocalAggregation keys in
        # order, block = the key of each InvResMLP block (`_level_queries` resolves it, `presample` sorts its searches' grids)
        self._plan, prev = [], []
        for radii, ks in zip(self.encoder_cfg.radius_list, self.encoder_cfg.nsample_list):
            sa, *block = [(float(r), int(k)) for r, k in zip(radii, ks)]
            self._plan.append(dict(sa=sa, answered=sa in prev, la=list(dict.fromkeys(block)), block=block))
            prev = self._plan[-1]["la"]
        # presample() also answers the neighbour queries (coordinates only): a pipeline knob -- where they run moves
        # work between the geometry and the feature stage, the results are the same tensors either way
        self.presample_neighbours = False
        # ... or only the queries of the downsampling levels from this one on (None: none): the lower levels' searches are
        # microseconds of work each but launches of the feature stream's dependent chain, and the geometry streams have slack
        self.presample_neighbours_from = None
        self._price_tail = 0   # measurement only (scripts/price_tail.py): extra evaluations of levels 3+ and the upsamplers
        # training forward: from this many input points per call (B * N) on, every downsampling stage is recomputed in the
        # backward instead of keeping the activations of its dense layers.  Measured (profiles/encoder_train_bench.md): a
        # step at 8 x 16 384 points keeps 200 MiB, recomputation saves 68 MiB of them for +0.6 ms -- not worth a forward
        # at the shipped sizes, so the threshold sits where the activations reach about 1.5 GiB
        self.train_checkpoint_rows = 1 << 20
        self._was_trained = False
        self.eval()

    # -- helpers -------------------------------------------------------------------------------
    @property
    def device(self) -> torch.device:
        return self.p("point_mlp0.weight").device

    def _mlp_ln(self, x: torch.Tensor, conv: str, ln: str, act: int, post: Optional[torch.Tensor] = None):
        return ops.linear_layernorm(x, self.p(conv + ".weight"), self.p(conv + ".bias"), self.p(ln + ".weight"),
                                    self.p(ln + ".bias"), act=act, post=post)

    def _group(self, prefix: str, radius: float, xyz, fea, centers, idx):
        return ops.group_mlp_max(xyz, fea, centers, idx, self.p(prefix + ".0.weight"), self.p(prefix + ".0.bias"),
                                 self.p(prefix + ".1.ln.weight"), self.p(prefix + ".1.ln.bias"), radius)

    # -- forward -------------------------------------------------------------------------------
    def _sample_level(self, i: int, xyz: torch.Tensor, lengths: torch.Tensor):
        """The sampler of downsampling stage i (pointnext.py:29-35, 45-46) -> (idx (B,K) int32 into the level's points,
        -1 = padding; new_xyz (B,K,3), zero rows at padding; new_lengths (B,)).  'voxel' stages (no shipped config has
        one) go through the voxel-grid kernels of csrc/voxel_sample.hip, which read the grid size back once per call."""
        st, k = self.encoder_cfg.sample[i], self.encoder_cfg.npoint[i]
        if st["type"] != "voxel":
            return ops.fps(xyz, lengths, k)
        N = xyz.shape[1]
        pad = torch.arange(N, device=xyz.device).unsqueeze(0) >= lengths.unsqueeze(1)
        sel, _ = ops.voxel_sample(xyz, pad, k, st["size"], st["range"])
        mask = sel < 0
        new = torch.gather(xyz, 1, sel.clamp(min=0).long().unsqueeze(-1).expand(-1, -1, 3)).masked_fill(mask.unsqueeze(-1), 0.0)
        return sel, new.contiguous(), (~mask).sum(1).to(torch.int32)

    @torch.no_grad()
    def sample_first_level(self, points_list, padding_list):
        """First-level farthest point sampling of SEVERAL batches in one launch (the sampling kernel runs one wave per
        frame: more frames per launch = more of the chip's latency-bound chains in flight).  Returns one
        (idx, new_xyz, new_lengths) per batch, views of the joint result."""
        dev = self.device
        with torch.cuda.device(dev):
            pts = torch.cat([p.to(device=dev, dtype=torch.float32) for p in points_list], 0)
            pad = torch.cat([p.to(device=dev) for p in padding_list], 0)
            xyz, lengths = ops.prepare_points(pts.contiguous(), pad.contiguous())
            fidx, new, nl = self._sample_level(0, xyz, lengths)
        out, o = [], 0
        for p in points_list:
            b = p.shape[0]
            out.append((fidx[o:o + b], new[o:o + b], nl[o:o + b]))
            o += b
        return out

    @torch.no_grad()
    def presample(self, points: torch.Tensor, points_padding: torch.Tensor, levels: Optional[int] = None,
                  sampled0=None) -> dict:
        """Input staging + the whole farthest-point-sampling chain (all levels), on the CURRENT stream.
        Sampling depends on coordinates only (level i+1 samples the points level i kept), never on features;
        it is a serial chain of dependent rounds that occupies one CU per frame, so a streaming caller runs it
        for batch i+1 on a side stream while batch i finishes on the main stream (pipeline.HotPath.submit).
        Pass the result to forward(..., presampled=...).  `levels` limits the pass to the first FPS levels (the
        remaining, much shorter ones then run inside forward) -- a knob for balancing pipeline stages.
        `sampled0` = (idx, new_xyz, new_lengths) of the first level when the caller sampled it already."""
        dev = self._require_gpu()
        with torch.cuda.device(dev):
            pts = points.to(device=dev, dtype=torch.float32).contiguous()
            pad = points_padding.to(device=dev).contiguous()
            xyz, lengths = ops.prepare_points(pts, pad)
            out = dict(pts=pts, xyz=xyz, lengths=lengths)
            n_levels = len(self.encoder_cfg.npoint) if levels is None else levels
            npoint = list(self.encoder_cfg.npoint[:n_levels])
            if n_levels >= 1 and (self.nested_fps or n_levels == 1):
                first = sampled0 if sampled0 is not None else self._sample_level(0, xyz, lengths)
                # every lower level is a prefix of the first level's picks: one bookkeeping launch for all of them
                lower = ops.nested_levels(first[1], first[2], npoint[1:]) if n_levels > 1 else []
                for i, (fidx, cur, cur_len) in enumerate([first] + lower):
                    out[f"fidx{i}"], out[f"xyz{i}"], out[f"len{i}"] = fidx, cur, cur_len
            else:
                cur, cur_len = xyz, lengths
                for i, k in enumerate(npoint):
                    fidx, cur, cur_len = sampled0 if (i == 0 and sampled0 is not None) else self._sample_level(i, cur, cur_len)
                    out[f"fidx{i}"], out[f"xyz{i}"], out[f"len{i}"] = fidx, cur, cur_len
            # The search grids of the neighbour queries depend on coordinates and radii only: they are sorted here,
            # next to the sampling, and forward() runs just the searches: one grid per search of the plan (a
            # SetAbstraction whose (radius, K) the previous level's LocalAggregation already answered needs none).
            grids, pts_i, len_i = {}, xyz, lengths
            for i, lv in enumerate(self._plan[:n_levels]):
                if not lv["answered"] and pts_i.shape[1] >= ops.GRID_MIN_N:
                    grids[("sa", i)] = ops.knn_grid(pts_i, len_i, lv["sa"][0])
                pts_i, len_i = out[f"xyz{i}"], out[f"len{i}"]
                for key in lv["la"] if pts_i.shape[1] >= ops.GRID_MIN_N else ():
                    grids[("la", i, key)] = ops.knn_grid(pts_i, len_i, key[0])
            out["grids"] = grids
            ahead = 0 if self.presample_neighbours else self.presample_neighbours_from
            if n_levels == len(self.encoder_cfg.npoint) and ahead is not None:
                out["knn"] = self._neighbour_queries(out, first_level=int(ahead))
        return out

    def _neighbour_queries(self, samp: dict, first_level: int = 0) -> dict:
        """The neighbour queries of the downsampling levels from `first_level` on -- they depend on coordinates only, like the
        sampling.  forward()'s own resolver answers them: ("sa", i) / ("la", i, (radius, K)) -> idx (a reused answer is a copy of
        rows of an identical query: the same tensors whether a level's first query finds a predecessor here or not)."""
        knn, self_q, level = {}, {}, (samp["xyz"], samp["lengths"])
        for i in range(len(self._plan)):
            sampled, own = (samp[f"fidx{i}"], samp[f"xyz{i}"], samp[f"len{i}"]), {}
            if i >= first_level:
                knn[("sa", i)], *_ = self._level_queries(i, level, sampled, self_q, own, {}, samp.get("grids", {}))
                knn.update((("la", i, key), idx) for key, idx in own.items())
            level, self_q = sampled[1:], own
        return knn

    def _level_queries(self, i: int, level, sampled, self_q: dict, own: dict, knn: dict, grids: dict):
        """The neighbour queries of downsampling level i, resolved by the plan: yields the SetAbstraction's idx (B,S,K), then the
        LocalAggregation idx (B,S,K) of each InvResMLP block -- each answered when it is asked for, so the searches stay where
        they were among the level's launches.  level = (xyz, lengths) the level samples from, sampled = (fidx, new_xyz, new_len)
        its picks; self_q = the self-queries of `level` (the previous level's LocalAggregations), (radius, K) -> idx (B,N,K); `own`
        receives those of the sampled level.  An answer presampled into `knn` is taken; a SetAbstraction whose key self_q holds
        copies its rows (only padded centres are searched); every other query is a search, in the grid presample() sorted for it
        (`grids`) where there is one."""
        lv = self._plan[i]
        (xyz, lengths), (fidx, new_xyz, new_len) = level, sampled
        gidx = knn.get(("sa", i))
        if gidx is None:
            prev = self_q.get(lv["sa"])
            gidx = ops.knn_hybrid(xyz, lengths, new_xyz, lv["sa"][1], lv["sa"][0], reuse_idx=prev,
                                  center_src=fidx if prev is not None else None, grid=grids.get(("sa", i)) if prev is None else None)
        yield gidx
        for key in lv["block"]:
            if key not in own:
                own[key] = knn[("la", i, key)] if ("la", i, key) in knn else ops.knn_hybrid(
                    new_xyz, new_len, new_xyz, key[1], key[0], grid=grids.get(("la", i, key)))
            yield own[key]

    @torch.no_grad()
    def forward(self, points: torch.Tensor, points_padding: torch.Tensor, trace: Optional[dict] = None,
                presampled: Optional[dict] = None, descriptor_scale: float = 0.0, spare_frames: int = 0,
                stop_level: Optional[int] = None, resume: Optional[dict] = None) -> List[torch.Tensor]:
        """-> [coor (B,3,S), fea (B,out_channel,S), padding (B,S)] (encoder.py:51-69).  descriptor_scale > 0 (not in the
        reference signature; used by the batched hot path): return instead the unified descriptor (B,out_channel+3,S) =
        [fea ; coor * descriptor_scale] that ExtractionThread.process builds from the triple (odometry.py:47-49).
        stop_level = i: run the downsampling levels below i and return the state (a dict) instead; resume = that state: run
        the rest (same kernels in the same order: the two halves may sit on different HIP streams, pipeline.py).
        In `.train()` mode: the training forward (`_forward_train`), `fea` attached to the autograd graph; the extra arguments
        are inference-only and raise ValueError there.  At train stage "loop_detection" (`set_train_stage`) the encoder is
        frozen and `.train()` changes nothing here: this inference forward runs, with all its arguments."""
        dev = self._require_gpu()
        if self.training and self.train_stage != "loop_detection":
            for name, given in (("presampled", presampled is not None), ("descriptor_scale", descriptor_scale != 0.0),
                                ("spare_frames", spare_frames != 0), ("stop_level", stop_level is not None),
                                ("resume", resume is not None)):
                if given:
                    raise ValueError(f"Encoder.forward: `{name}` belongs to the inference pipeline and is not available in "
                                     f".train() mode (call .eval() first)")
            return self._forward_train(points, points_padding, trace)
        enc = self.encoder_cfg
        if resume is not None:
            samp = resume["samp"]
        else:
            samp = presampled if presampled is not None else self.presample(points, points_padding)
        with torch.cuda.device(dev):
            pts, xyz, lengths = samp["pts"], samp["xyz"], samp["lengths"]
            # level-0 features = point_mlp0(points).  With xyz-only input (every shipped config) they are only ever
            # consumed by the first SetAbstraction, which evaluates them inside its gather (fea = None here).
            w0 = self.p("point_mlp0.weight")
            fuse0 = (self.in_channel == 3 and w0.shape[0] % 4 == 0 and 2 * w0.shape[0] in (32, 64, 128)
                     and enc.nsample_list[0][0] in (16, 32))
            if resume is not None or fuse0:
                fea = None
            elif self.in_channel == 3:
                fea = ops.linear(xyz, w0, self.p("point_mlp0.bias"))
            else:  # extra input channels: point-major copy of the first in_channel rows
                fea = ops.linear(pts[:, :self.in_channel].transpose(1, 2).contiguous(), w0, self.p("point_mlp0.bias"))
            levels = [(xyz, fea, lengths)] if resume is None else resume["levels"]
            # `self_q` remembers the self-queries of the current level for the next one's SetAbstraction (`_level_queries`):
            # (radius, K) -> idx (B,N,K)
            self_q = {} if resume is None else resume["self_q"]
            grids, knn = samp.get("grids", {}), samp.get("knn", {})
            for i, npoint in enumerate(enc.npoint):
                if resume is not None and i < resume["next"]:
                    continue
                if stop_level is not None and i >= stop_level:
                    return dict(samp=samp, levels=levels, self_q=self_q, next=i)
                xyz, fea, lengths = levels[-1]
                radii = enc.radius_list[i]
                pre = f"downsampler.{i}"
                if f"fidx{i}" in samp:
                    fidx, new_xyz, new_len = samp[f"fidx{i}"], samp[f"xyz{i}"], samp[f"len{i}"]
                else:  # levels the geometry pass left to this stream
                    fidx, new_xyz, new_len = self._sample_level(i, xyz, lengths)
                # (self._price_tail > 0: levels 3+ and the upsamplers are computed that many extra times, results identical --
                # scripts/price_tail.py measures what the launch-bound tail of the encoder costs a pipelined step)
                for _rep in range(1 + (self._price_tail if i >= 3 else 0)):
                    own = {}
                    queries = self._level_queries(i, (xyz, lengths), (fidx, new_xyz, new_len), self_q, own, knn, grids)
                    gidx = next(queries)
                    self_q = own  # from here on the level is the sampled one
                    if fea is None:
                        m = pre + ".sa.mlp"
                        new_fea = ops.group_mlp_max_from_xyz(xyz, w0, self.p("point_mlp0.bias"), new_xyz, gidx,
                                                             self.p(m + ".0.weight"), self.p(m + ".0.bias"),
                                                             self.p(m + ".1.ln.weight"), self.p(m + ".1.ln.bias"), radii[0])
                    else:
                        new_fea = self._group(pre + ".sa.mlp", radii[0], xyz, fea, new_xyz, gidx)
                    if trace is not None:
                        trace[pre + ".fps.idx"], trace[pre + ".fps.new"] = fidx, new_xyz
                        trace[pre + ".sa.idx"], trace[pre + ".sa.out"] = gidx, new_fea
                    for j, lidx in enumerate(queries, 1):
                        q = f"{pre}.irm.{j - 1}"
                        t = self._group(q + ".la.mlp", radii[j], new_xyz, new_fea, new_xyz, lidx)
                        pair = ops.pwconv_pair(t, self.p(q + ".pw_conv.0.weight"), self.p(q + ".pw_conv.0.bias"),
                                               self.p(q + ".pw_conv.1.ln.weight"), self.p(q + ".pw_conv.1.ln.bias"),
                                               self.p(q + ".pw_conv.3.weight"), self.p(q + ".pw_conv.3.bias"),
                                               self.p(q + ".pw_conv.4.ln.weight"), self.p(q + ".pw_conv.4.ln.bias"), post=new_fea)
                        if pair is not None:     # the first level: both layers in one kernel, the 4C-wide intermediate in registers
                            new_fea = pair
                        else:
                            u = self._mlp_ln(t, q + ".pw_conv.0", q + ".pw_conv.1.ln", ops.ACT_RELU)
                            new_fea = self._mlp_ln(u, q + ".pw_conv.3", q + ".pw_conv.4.ln", ops.ACT_RELU, post=new_fea)
                        if trace is not None:
                            trace[q + ".la.idx"], trace[q + ".la.out"], trace[q + ".out"] = lidx, t, new_fea
                levels.append((new_xyz, new_fea, new_len))
            L = self.downsample_layers
            for i in range(self.upsample_layers):
                xyz1, fea1, len1 = levels[L - i - 1]
                xyz2, fea2, len2 = levels[-1]
                q = f"upsampler.{i}"
                for _rep in range(1 + self._price_tail):
                    x = ops.three_interp_cat(xyz1, xyz2, len2, fea1, fea2)
                    x = self._mlp_ln(x, q + ".mlp.0", q + ".mlp.1.ln", ops.ACT_RELU)
                    x = self._mlp_ln(x, q + ".mlp.3", q + ".mlp.4.ln", ops.ACT_RELU)
                if trace is not None:
                    trace[q + ".out"] = x
                levels.append((xyz1, x, len1))
            xyz, fea, lengths = levels[-1]
            coor, feat, padding, desc = ops.emit_descriptors(xyz, fea, lengths, descriptor_scale, spare_frames)
            if descriptor_scale > 0:
                return desc
        return [coor, feat, padding]

    # -- training --------------------------------------------------------------------------------
    def train(self, mode: bool = True):
        """A real switch, like Decoder.train.  `.train()` selects the reference's registration training mode
        (model_pipeline.py's `registration()` turns on every parameter whose name lacks `loop`: all of the encoder): every
        parameter gets requires_grad = True and `forward` returns `fea` attached to the graph, so encoder -> decoder ->
        RegistrationLoss -> backward() fills `.grad` of all 110 tensors.  `.eval()` (what `__init__` ends in) turns
        requires_grad off again and drops the weight-derived caches; in-place optimiser steps bump the parameters' version
        counters, which those caches key on, so inference after a step reads the new weights.
        At train stage "loop_detection" (`set_train_stage`; model_pipeline.py's `loop_detection()` freezes every parameter
        whose name lacks `loop`: all of the encoder) `.train()` leaves every parameter frozen and `forward` stays the
        inference forward: the same bytes as in `.eval()`, at inference cost."""
        super().train(mode)
        on = bool(mode) and self.train_stage != "loop_detection"
        for p in self._flat.values():
            p.requires_grad_(on)
        if mode:
            self._was_trained = True
        elif getattr(self, "_was_trained", False):
            self._was_trained = False
            self.invalidate_caches()
        return self

    def _mlp_ln_train(self, x, conv: str, ln: str, post=None):
        """relu(LN(conv x) [+ post]): what ops.linear_layernorm evaluates, under autograd"""
        return self._dense_ln(x, *self._w(conv), self.p(ln + ".weight"), self.p(ln + ".bias"), post=post, act=ops.ACT_RELU)

    def _group_train(self, prefix: str, radius: float, xyz, fea, centers, idx, keep):
        """SetAbstraction / LocalAggregation body: the projection under autograd, the rest in csrc/group_train.hip"""
        W, bias = self._w(prefix + ".0")
        Cin = fea.shape[2]
        if W.shape[0] not in ops.GROUP_TRAIN_COUT or idx.shape[2] not in ops.GROUP_TRAIN_K:
            raise ValueError(f"Encoder.forward (train mode): layer {prefix} has width {W.shape[0]} and {idx.shape[2]} "
                             f"neighbours; the training kernels cover widths {ops.GROUP_TRAIN_COUT} and neighbour counts "
                             f"{ops.GROUP_TRAIN_K}")
        P = self._dense(fea, W[:, :Cin], bias)
        slots = None if keep is None else []
        out = ops.group_train(P, xyz, centers, idx, W[:, Cin:].contiguous(), self.p(prefix + ".1.ln.weight"),
                              self.p(prefix + ".1.ln.bias"), radius, layer=prefix, keep_slots=slots)
        if keep is not None:
            keep[prefix + ".idx"], keep[prefix + ".winners"] = idx, ops.group_train_winners(idx, slots[0])
        return out

    def _train_stage(self, i: int, xyz, fea, new_xyz, gidx, lidx_list, keep):
        """Stage i (pointnext.py:169-173): SetAbstraction, then its InvResMLP blocks"""
        radii = self.encoder_cfg.radius_list[i]
        pre = f"downsampler.{i}"
        new_fea = self._group_train(pre + ".sa.mlp", radii[0], xyz, fea, new_xyz, gidx, keep)
        for j in range(1, len(radii)):
            q = f"{pre}.irm.{j - 1}"
            t = self._group_train(q + ".la.mlp", radii[j], new_xyz, new_fea, new_xyz, lidx_list[j - 1], keep)
            u = self._mlp_ln_train(t, q + ".pw_conv.0", q + ".pw_conv.1.ln")
            new_fea = self._mlp_ln_train(u, q + ".pw_conv.3", q + ".pw_conv.4.ln", post=new_fea)
        return new_fea

    @staticmethod
    def _interp_weights(xyz1, xyz2, len2):
        """FeaturePropagation's 3-NN inverse-distance weights (pointnext.py:199-210) as a dense (B,N,S) matrix with three
        non-zeros per row, made without gradient (coordinates have no parameter upstream): interpolation is then a bmm,
        whose backward is a bmm again -- no scatter.  Padded coarse points are infinitely far (weight 0), as in
        csrc/encoder_ops.hip."""
        with torch.no_grad():
            B, N, _ = xyz1.shape
            S = xyz2.shape[1]
            d = -2.0 * torch.bmm(xyz1, xyz2.transpose(1, 2))
            d += (xyz1 ** 2).sum(-1).unsqueeze(2)
            d += (xyz2 ** 2).sum(-1).unsqueeze(1)
            pad = torch.arange(S, device=xyz2.device).unsqueeze(0) >= len2.unsqueeze(1)
            d = d.masked_fill(pad.unsqueeze(1), float("inf"))
            dist, nn = torch.topk(d, min(3, S), dim=-1, largest=False)
            w = 1.0 / dist.clamp(min=1e-8)
            w = w / w.sum(-1, keepdim=True)
            return torch.zeros(B, N, S, device=xyz1.device, dtype=torch.float32).scatter_(2, nn, w)

    def _forward_train(self, points: torch.Tensor, points_padding: torch.Tensor, trace: Optional[dict] = None):
        """The reference's training forward (encoder.py:51-69 under autograd) -> [coor (B,3,S), fea (B,out_channel,S),
        padding (B,S)], `fea` differentiable with respect to all 110 parameters.

        Sampling, the neighbour queries and the level bookkeeping are the inference kernels under no_grad (geometry has no
        parameter upstream).  Every grouping layer is ops.group_train (HIP forward and backward, no (B,S,K,C) tensor);
        point_mlp0, the W_f projections, pw_conv and the upsampler MLPs with their LayerNorms are torch operations under
        autograd, and the interpolation is a bmm with a weight matrix built without gradient.  Grad mode is enabled here,
        whatever the caller's is.  From `train_checkpoint_rows` input points (B * N) on, each downsampling stage is
        recomputed in the backward (torch.utils.checkpoint: the same kernels on the same inputs, identical bytes).
        trace (a dict) receives, per grouping layer, `<layer>.idx` (B,S,K) and `<layer>.winners` (B,S,C): the neighbour
        point that gave the maximum, -1 where the ReLU floor did, and per stage `downsampler.<i>.fps.new` / `.len`, the sampled
        coordinates and valid counts (tracing turns the recomputation off).
        Raises ValueError for configurations with a voxel sampler and for layer widths the kernels do not cover."""
        if not self.all_fps:
            raise ValueError("Encoder.forward (train mode): voxel samplers are inference-only; use 'fps' stages for training")
        enc, dev = self.encoder_cfg, self.device
        with torch.no_grad():
            samp = self.presample(points, points_padding)
            knn = samp["knn"] if "knn" in samp and self.presample_neighbours else self._neighbour_queries(samp)
        keep = trace   # tracing keeps the winners of every grouping layer
        with torch.enable_grad(), torch.cuda.device(dev):
            pts, xyz, lengths = samp["pts"], samp["xyz"], samp["lengths"]
            x0 = xyz if self.in_channel == 3 else pts[:, :self.in_channel].transpose(1, 2).contiguous()
            fea = self._dense(x0, *self._w("point_mlp0"))
            recompute = keep is None and xyz.shape[0] * xyz.shape[1] >= self.train_checkpoint_rows
            levels = [(xyz, fea, lengths)]
            for i in range(len(enc.npoint)):
                new_xyz, new_len = samp[f"xyz{i}"], samp[f"len{i}"]
                lidx = [knn[("la", i, key)] for key in self._plan[i]["block"]]
                if recompute:
                    new_fea = checkpoint(self._train_stage, i, xyz, fea, new_xyz, knn[("sa", i)], lidx, None, use_reentrant=False)
                else:
                    new_fea = self._train_stage(i, xyz, fea, new_xyz, knn[("sa", i)], lidx, keep)
                if keep is not None:
                    keep[f"downsampler.{i}.fps.new"], keep[f"downsampler.{i}.len"] = new_xyz, new_len
                levels.append((new_xyz, new_fea, new_len))
                xyz, fea = new_xyz, new_fea
            L = self.downsample_layers
            for i in range(self.upsample_layers):
                xyz1, fea1, len1 = levels[L - i - 1]
                xyz2, fea2, len2 = levels[-1]
                q = f"upsampler.{i}"
                if xyz2.shape[1] == 1:   # pointnext.py:194-196
                    up = fea2.expand(-1, xyz1.shape[1], -1)
                else:
                    up = torch.bmm(self._interp_weights(xyz1, xyz2, len2), fea2)
                x = self._mlp_ln_train(torch.cat([fea1, up], dim=2), q + ".mlp.0", q + ".mlp.1.ln")
                x = self._mlp_ln_train(x, q + ".mlp.3", q + ".mlp.4.ln")
                levels.append((xyz1, x, len1))
            xyz, fea, lengths = levels[-1]
            coor, _, padding, _ = ops.emit_descriptors(xyz, fea.detach().contiguous(), lengths)
            return [coor, fea.transpose(1, 2), padding]
