"""The encoder's training forward (network/encoder/encoder.py:51-69 with pointnext.py's Stage / FeaturePropagation) restated
in plain, dense, differentiable torch -- any device, any dtype.  No library code, no reference code.

Geometry is GIVEN: the sampled coordinates per level and the neighbour indices per grouping layer come from the caller (the
fixture, or the module's trace), because they depend on coordinates only and have no parameter upstream.

`winners` (optional): {layer: (B,S,C) int64} the neighbour POINT that wins the max of channel c at centre s (-1: none, the
ReLU floor).  With it the max over the K neighbours is replaced by a gather at the first slot holding that point, which is
differentiable and identical to the max wherever the choice equals the true argmax: gradients of two implementations can be
compared on equal routes.  Without it the true max is taken and the chosen points are returned."""
import torch
import torch.nn.functional as F


def layer_names(cfg):
    """the grouping layers in evaluation order -> [(name, stage, radius, K)]"""
    enc, out = cfg.encoder, []
    for i in range(len(enc.npoint)):
        out.append((f"downsampler.{i}.sa.mlp", i, enc.radius_list[i][0], enc.nsample_list[i][0]))
        for j in range(1, len(enc.radius_list[i])):
            out.append((f"downsampler.{i}.irm.{j - 1}.la.mlp", i, enc.radius_list[i][j], enc.nsample_list[i][j]))
    return out


def _w(sd, key):
    w = sd[key + ".weight"]
    return w.reshape(w.shape[0], w.shape[1]), sd[key + ".bias"]


def _ln(x, sd, key):
    return F.layer_norm(x, (x.shape[-1],), sd[key + ".weight"], sd[key + ".bias"], 1e-5)


def _conv(x, sd, key):
    """Conv1d(k=1) on point-major rows, evaluated channel-first like the reference"""
    W, b = _w(sd, key)
    return F.conv1d(x.transpose(1, 2), W.unsqueeze(-1), b).transpose(1, 2)


def group_layer(xyz, fea, centers, idx, W, b, gamma, beta, radius, winners=None):
    """xyz (B,N,3), fea (B,N,Cin), centers (B,S,3), idx (B,S,K) -> (out (B,S,C), winning point (B,S,C) int64, dense
    post-activation values (B,S,K,C)): pointnext.py:52-61 / 97-107"""
    B, S, K = idx.shape
    gi = idx.long()
    bi = torch.arange(B, device=idx.device).view(B, 1, 1)
    rel = (xyz[bi, gi] - centers.unsqueeze(2)) / radius
    # the reference's own operand layout, (B,C+3,K,S) through a 1x1 convolution: the same GEMM, so that an fp32 run on the CPU
    # rounds like the reference's and near-ties of the max fall the same way
    h = F.conv2d(torch.cat([fea[bi, gi], rel], dim=-1).permute(0, 3, 2, 1), W.unsqueeze(-1).unsqueeze(-1), b)
    y = F.relu(F.layer_norm(h.permute(0, 2, 3, 1), (W.shape[0],), gamma, beta, 1e-5)).transpose(1, 2)   # (B,S,K,C)
    if winners is None:
        out, slot = y.max(dim=2)
        pts = torch.gather(gi, 2, slot)
        return out, torch.where(out > 0, pts, torch.full_like(pts, -1)), y
    match = gi.unsqueeze(3) == winners.unsqueeze(2)                            # (B,S,K,C)
    order = torch.arange(K, 0, -1, device=idx.device).view(1, 1, K, 1)
    slot = (match * order).argmax(dim=2)                                       # the first slot holding the winner
    out = torch.gather(y, 2, slot.unsqueeze(2)).squeeze(2)
    return out * (winners >= 0).to(out.dtype), winners, y


def interpolate(xyz1, xyz2, len2, fea2):
    """pointnext.py:194-213: 3-NN inverse-distance interpolation of the coarse features onto the fine points; padded coarse
    points never rank among the three (the reference moves them far away)"""
    B, N, _ = xyz1.shape
    S = xyz2.shape[1]
    if S == 1:
        return fea2.expand(-1, N, -1)
    with torch.no_grad():
        d = -2 * torch.bmm(xyz1, xyz2.transpose(1, 2))
        d += (xyz1 ** 2).sum(-1).unsqueeze(2)
        d += (xyz2 ** 2).sum(-1).unsqueeze(1)
        pad = torch.arange(S, device=xyz2.device).unsqueeze(0) >= len2.unsqueeze(1)
        d = d.masked_fill(pad.unsqueeze(1), float("inf"))
        dist, nn = torch.topk(d, 3, dim=-1, largest=False)
        w = 1.0 / dist.clamp(min=1e-8)
        w = w / w.sum(-1, keepdim=True)
    bi = torch.arange(B, device=xyz1.device).view(B, 1, 1)
    return (fea2[bi, nn] * w.unsqueeze(-1)).sum(dim=2)


def encoder_train_restated(cfg, sd, xyz, level_xyz, level_len, idx, winners=None):
    """cfg: the project's args; sd {key: tensor} in the working dtype (leaves with requires_grad for gradients);
    xyz (B,N,3) input points; level_xyz[i] (B,S_i,3), level_len[i] (B,) of downsampling stage i; idx {layer: (B,S,K)};
    winners {layer: (B,S,C)} or None  ->  (fea (B,S,C) point-major of the returned level, {layer: winning points})."""
    enc = cfg.encoder
    dt = sd["point_mlp0.weight"].dtype
    xyz = xyz.to(dt)
    fea = _conv(xyz, sd, "point_mlp0")
    levels, routes = [(xyz, fea, None)], {}
    for i in range(len(enc.npoint)):
        pre = f"downsampler.{i}"
        radii = enc.radius_list[i]
        new_xyz = level_xyz[i].to(dt)

        def group(name, radius, pts, f, ctr):
            W, b = _w(sd, name + ".0")
            out, routes[name], _ = group_layer(pts, f, ctr, idx[name], W, b, sd[name + ".1.ln.weight"], sd[name + ".1.ln.bias"],
                                               radius, None if winners is None else winners[name])
            return out
        new_fea = group(pre + ".sa.mlp", radii[0], xyz, fea, new_xyz)
        for j in range(1, len(radii)):
            q = f"{pre}.irm.{j - 1}"
            t = group(q + ".la.mlp", radii[j], new_xyz, new_fea, new_xyz)
            u = F.relu(_ln(_conv(t, sd, q + ".pw_conv.0"), sd, q + ".pw_conv.1.ln"))
            new_fea = F.relu(_ln(_conv(u, sd, q + ".pw_conv.3"), sd, q + ".pw_conv.4.ln") + new_fea)
        levels.append((new_xyz, new_fea, level_len[i]))
        xyz, fea = new_xyz, new_fea
    L = len(enc.npoint)
    for i in range(enc.upsample_layers):
        xyz1, fea1, len1 = levels[L - i - 1]
        xyz2, fea2, len2 = levels[-1]
        q = f"upsampler.{i}"
        x = torch.cat([fea1, interpolate(xyz1, xyz2, len2, fea2)], dim=2)
        x = F.relu(_ln(_conv(x, sd, q + ".mlp.0"), sd, q + ".mlp.1.ln"))
        x = F.relu(_ln(_conv(x, sd, q + ".mlp.3"), sd, q + ".mlp.4.ln"))
        levels.append((xyz1, x, len1))
    return levels[-1][1], routes
