"""Case builders for the edge tests of the encoder's grouping training operator (csrc/group_train.hip): the launch plan restated,
shapes that put the kernels on the plan's and the lanes' edges, seeded inputs and constructed variants.  CPU torch only, no
library code.  tests/test_group_train_cases_host.py pins everything here on the CPU; tests/test_gpu_group_train_edges.py runs it.

A shape is (Cout, B, N, S, K).  An inputs dict holds xyz (B,N,3), centers (B,S,3), idx (B,S,K) int32, P (B,N,Cout),
W_rel (Cout,3), gamma, beta (Cout), dout (B,S,Cout) with integer values, radius, and `ungathered`: the number of points at the
end of every frame that idx never names.
"""
import collections
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_train_restated as R  # noqa: E402

RADIUS = 0.5
NO_WINNER = 255

Plan = collections.namedtuple("Plan", "rpw groups cap ppw waves bytes dead_iterations ragged waves_mod4")


def _r256(n):
    return (n + 255) // 256 * 256


def plan(B, N, S, K, Cout):
    """make_plan of csrc/group_train.hip restated: how the backward spreads the B N points over its waves, and the workspace"""
    if Cout not in (32, 64, 128, 256, 512) or K not in (16, 32) or B < 1 or N < 1 or S < 1:
        return Plan(0, 0, 0, 0, 0, 0, 0, 0, 0)
    V = 2 if Cout == 512 else 1
    rpw = 64 // (Cout // (4 * V))
    points = B * N
    groups = -(-points // rpw)
    cap = max(131072 // Cout, 256)
    ppw = -(-groups // cap)
    waves = -(-groups // ppw)
    size = sum(_r256(n) for n in (4 * B * S, 4 * points, 4 * (points + 1), 4 * B * S * K, 4 * B * S * K, 4 * waves * 5 * Cout))
    return Plan(rpw, groups, cap, ppw, waves, size, waves * ppw - groups, points % rpw, waves % 4)


# One shape per width on every plan edge at once: ppw = 2, one dead t iteration in the last wave, waves no multiple of 4 (a block
# with idle waves), B N no multiple of rpw (lane groups past the last point), frames of odd length (lane groups of one wave in
# two frames); S = 37: B S neither a multiple of 4 (the forward's block) nor of 256 (row_mask_kernel's)
PLAN_SHAPES = [(32, 3, 10925, 37, 16), (32, 3, 10925, 37, 32), (64, 3, 2731, 37, 32), (128, 3, 683, 37, 32), (256, 3, 171, 37, 32),
               (512, 7, 37, 37, 16)]
# ppw = 1: 39 points in 5 groups (7 live lane groups in the last), one point, small odd everything, n = 1024 + 1 for the scan
TINY_SHAPES = [(32, 3, 13, 5, 16), (64, 1, 1, 1, 32), (128, 5, 7, 3, 32), (256, 1, 3, 2, 32), (32, 1, 1025, 9, 32)]
SHIPPED = [(32, 32), (64, 32), (128, 32), (256, 32), (512, 16), (32, 16), (512, 32)]
SHIPPED_SMALL = [(Cout, 2, 300, 70, K) for Cout, K in SHIPPED]
# distinct neighbours per centre need N - N // 4 >= K (PERM) and, with no point serving two centres, >= S K (TIE)
PERM_SHAPES = [(32, 3, 29, 5, 16), (128, 2, 45, 3, 32), (512, 2, 23, 3, 16)]
TIE_SHAPES = {32: (32, 2, 87, 4, 16), 64: (64, 2, 173, 4, 32), 128: (128, 2, 173, 4, 32), 256: (256, 2, 173, 4, 32),
              512: (512, 2, 87, 4, 16)}
# the constructed dead / flat / poisoned / out-of-range variants run on these
VARIANT_SHAPES = [(32, 3, 13, 5, 16), (128, 3, 683, 37, 32), (512, 7, 37, 37, 16)]


def shape_id(shape):
    return "C{}-B{}-N{}-S{}-K{}".format(*shape)


def tie_pairs(Cout, K):
    """slot pairs (k1, k2): neighbours in two lane groups of one iteration, in one lane group of consecutive iterations, the
    first and the last slot, the last two"""
    rpw = plan(1, 1, 1, K, Cout).rpw
    pairs = [(1, 2), (1, 1 + rpw), (0, K - 1), (K - 2, K - 1)]
    if rpw > 1:
        pairs.insert(1, (rpw - 1, rpw))
    return sorted(set(pairs))


def ungathered_count(N):
    return max(N // 4, 1) if N > 2 else 0


def never(t):
    """(B,N) bool: the points idx is built never to name"""
    _, B, N, _, _ = t["shape"]
    return (torch.arange(N) >= N - t["ungathered"]).unsqueeze(0).expand(B, N)


def inputs(shape, seed=0):
    Cout, B, N, S, K = shape
    assert S <= N
    gen = torch.Generator().manual_seed(7919 * seed + Cout + K + N)
    xyz = torch.rand(B, N, 3, generator=gen)
    centers = xyz[:, :S].clone()
    ung = ungathered_count(N)
    idx = torch.randint(0, N - ung, (B, S, K), generator=gen, dtype=torch.int32)
    Cin = Cout // 2
    fea = torch.randn(B, N, Cin, generator=gen)
    W = torch.randn(Cout, Cin + 3, generator=gen) / (Cin + 3) ** 0.5
    bias = 0.1 * torch.randn(Cout, generator=gen)
    gamma = 1 + 0.2 * torch.randn(Cout, generator=gen)
    gamma[::7] *= -1                                   # both signs
    beta = 0.2 * torch.randn(Cout, generator=gen)
    dout = torch.randint(-4, 5, (B, S, Cout), generator=gen).float()   # integers: sums of them are exact in fp32 in any order
    return dict(shape=shape, xyz=xyz, centers=centers, idx=idx, P=torch.nn.functional.linear(fea, W[:, :Cin], bias).contiguous(),
                W_rel=W[:, Cin:].contiguous(), gamma=gamma, beta=beta, dout=dout, radius=RADIUS, ungathered=ung)


def _copy(t):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in t.items()}


def frame(t, b):
    """frame b alone, as a batch of one"""
    out = {k: (v[b:b + 1].clone() if torch.is_tensor(v) and v.dim() == 3 else v) for k, v in _copy(t).items()}
    out["shape"] = (t["shape"][0], 1) + tuple(t["shape"][2:])
    return out


# ---- constructed variants: inputs dict -> a new one ----------------------------------------------------------------------------

def distinct(t, seed=0):
    """idx redrawn so that the K neighbours of a centre are K different points (a point may still serve several centres)"""
    Cout, B, N, S, K = t["shape"]
    assert N - t["ungathered"] >= K
    gen = torch.Generator().manual_seed(seed + 31)
    out = _copy(t)
    out["idx"] = torch.stack([torch.randperm(N - t["ungathered"], generator=gen)[:K] for _ in range(B * S)]).view(B, S, K).int()
    return out


def permute_slots(t, seed=0):
    """-> (inputs with the K slots of every centre permuted, perm (B,S,K) int64): the neighbour of slot k moves to slot perm[k]"""
    _, B, _, S, K = t["shape"]
    gen = torch.Generator().manual_seed(seed + 57)
    perm = torch.stack([torch.randperm(K, generator=gen) for _ in range(B * S)]).view(B, S, K)
    out = _copy(t)
    out["idx"] = torch.empty_like(t["idx"]).scatter_(2, perm, t["idx"])
    return out, perm


SPIKE = 8.0   # the pair then wins 0.45 to 0.6 of the live maxima (4: 0.32 to 0.48)


def tie(t, k1, k2, seed=0):
    """Two DIFFERENT points with the same row at slots k1 < k2 of every centre.  idx is redrawn: all B S K neighbours of a frame
    are different points.  The point of slot k2 gets P and xyz of the point of slot k1, so the two post-activation rows are equal
    in every arithmetic.  So that this pair decides a good share of the maxima (alone it would win one in K), the other K - 2
    neighbours get a spike of SPIKE sqrt(Cout) in channel 0 or 1: LayerNorm then leaves them about -1 / sqrt(Cout) elsewhere."""
    Cout, B, N, S, K = t["shape"]
    assert 0 <= k1 < k2 < K and N - t["ungathered"] >= S * K
    gen = torch.Generator().manual_seed(seed + 101 * k1 + k2)
    out = _copy(t)
    idx = torch.stack([torch.randperm(N - t["ungathered"], generator=gen)[:S * K] for _ in range(B)]).view(B, S, K)
    bi = torch.arange(B).view(B, 1)
    keep = torch.ones(K, dtype=torch.bool)
    keep[[k1, k2]] = False
    others = idx[:, :, keep].reshape(B, -1)
    out["P"][bi, others, others % 2] += SPIKE * Cout ** 0.5
    a, c = idx[:, :, k1], idx[:, :, k2]
    out["P"][bi, c] = out["P"][bi, a]
    out["xyz"][bi, c] = out["xyz"][bi, a]
    out["idx"] = idx.int()
    return out


def all_dead(t):
    """no neighbour of any centre exceeds the ReLU floor: |gamma n| <= |gamma| sqrt(Cout - 1) < 100"""
    out = _copy(t)
    out["beta"] = torch.full_like(t["beta"], -100.0)
    return out


def dead_channel(t, c0):
    out = _copy(t)
    out["beta"][c0] = -100.0
    return out


def flat_rows(t, seed=0):
    """zero variance: W_rel = 0 and every P row one value in all channels, so rs = 1 / sqrt(1e-5), n = 0, y = beta"""
    _, B, N, _, _ = t["shape"]
    gen = torch.Generator().manual_seed(seed + 211)
    out = _copy(t)
    out["W_rel"] = torch.zeros_like(t["W_rel"])
    out["P"] = torch.randn(B, N, 1, generator=gen).expand_as(t["P"]).contiguous()
    return out


def poison_ungathered(t):
    out = _copy(t)
    out["P"][never(t)] = float("nan")
    out["xyz"][never(t)] = float("nan")
    return out


def out_of_range(t, seed=0):
    """a seeded 10 % of idx replaced by -1, -7, N and N + 5 -> (raw inputs, the same with idx clamped to [0, N))"""
    N = t["shape"][2]
    gen = torch.Generator().manual_seed(seed + 307)
    hit = torch.rand(t["idx"].shape, generator=gen) < 0.1
    bad = torch.tensor([-1, -7, N, N + 5], dtype=torch.int32)[torch.randint(0, 4, t["idx"].shape, generator=gen)]
    raw, clamped = _copy(t), _copy(t)
    raw["idx"] = torch.where(hit, bad, t["idx"])
    clamped["idx"] = raw["idx"].clamp(0, N - 1)
    return raw, clamped


# ---- the dense restatement on a case ---------------------------------------------------------------------------------------------

def restate(t, dtype=torch.float64, device="cpu", winners=None, grads=False):
    """R.group_layer on the case with P itself as the features through [I | W_rel] (so that d/d fea is dP) ->
    (out (B,S,C), winning points (B,S,C), y (B,S,K,C), (dP, dW_rel, dgamma, dbeta) or None).  winners forces the routes."""
    Cout = t["shape"][0]
    to = lambda x: x.detach().to(device=device, dtype=dtype)   # noqa: E731
    leaves = [to(t[k]).requires_grad_(grads) for k in ("P", "W_rel", "gamma", "beta")]
    with torch.enable_grad():
        W = torch.cat([torch.eye(Cout, device=device, dtype=dtype), leaves[1]], dim=1)
        out, pts, y = R.group_layer(to(t["xyz"]), leaves[0], to(t["centers"]), t["idx"].to(device), W,
                                    torch.zeros(Cout, device=device, dtype=dtype), leaves[2], leaves[3], t["radius"], winners)
        g = torch.autograd.grad(out, leaves, to(t["dout"])) if grads else None
    return out.detach(), pts, y.detach(), g


def all_cases():
    """every case the GPU tests run whose idx is in range -> [(name, inputs, kind, extra)]"""
    out = []
    for shape in PLAN_SHAPES + TINY_SHAPES + SHIPPED_SMALL:
        out.append((shape_id(shape), inputs(shape), "plain", None))
    for shape in PERM_SHAPES:
        t = distinct(inputs(shape))
        out.append(("distinct " + shape_id(shape), t, "plain", None))
        out.append(("permuted " + shape_id(shape), permute_slots(t)[0], "plain", None))
    for Cout, shape in TIE_SHAPES.items():
        for k1, k2 in tie_pairs(Cout, shape[4]):
            out.append((f"tie {k1},{k2} " + shape_id(shape), tie(inputs(shape), k1, k2), "tie", (k1, k2)))
    for shape in VARIANT_SHAPES:
        t = inputs(shape)
        out.append(("all_dead " + shape_id(shape), all_dead(t), "all_dead", None))
        out.append(("dead_channel " + shape_id(shape), dead_channel(t, 5), "dead_channel", 5))
        out.append(("flat_rows " + shape_id(shape), flat_rows(t), "plain", None))
        out.append(("poison_ungathered " + shape_id(shape), poison_ungathered(t), "poison", None))
        out.append(("out_of_range clamped " + shape_id(shape), out_of_range(t)[1], "clamped", None))
    return out
