"""TEST INFRASTRUCTURE: plain torch restatements and seeded cases of the registration tail -- the kernels behind
match_topk in the decoder (gather_pairs, corr_kabsch FROM OFFSETS, the result header), the map-tile assembly in front of it
and the copy / reduce kernels around them.  No GPU here; tests/test_registration_tail_host.py holds this file to its
conditions, tests/test_gpu_registration_tail.py runs the kernels against it.

The Kabsch loop itself is the oracle's (oracle.dpm_oracle.solve_svd, which calls torch.topk, so equal weights at the 64th
place are resolved the reference's way); this file adds what stands in front of it when the decoder calls the kernel:
the two correspondence copies and the cut on the offset length."""
import math

import torch

from oracle import dpm_oracle as O

EPS = 2.0          # eps_offset of every Kabsch case (metres)
RES_HDR = 20       # floats in front of the inlier confidences of a result row (deeppointmap_amd.ops.RES_HDR, asserted equal)
LD, XYZ_COL = 131, 128   # the decoder reads xyz out of descriptor rows: row stride 131, xyz from column 128 (decoder.py:453)


# ---------------------------------------------------------------------------------------------------------------------
# correspondence sets from offsets                          oracle.dpm_oracle.correspondence_sets without the head
# ---------------------------------------------------------------------------------------------------------------------
def offset_cut(off: torch.Tensor, eps: float) -> torch.Tensor:
    """(2k,3) fp32 -> bool (2k,): (x^2 + y^2) + z^2 <= eps^2 in fp32, the association the kernel states"""
    o = off.float()
    return (o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1]) + o[:, 2] * o[:, 2] <= torch.tensor(eps * eps, dtype=torch.float32)


def correspondences(off, xyz_s, xyz_d, si, di, conf, eps):
    """off (2k,3) [source->target offsets ; target->source offsets], xyz_s (M,3), xyz_d (N,3), si / di (k,), conf (k,)
    -> (src (3,n), dst (3,n), w (n,), keep (2k,) bool):  [ps + off_a ; ps] <-> [pd ; pd + off_b], both copies weighted by
    conf, entries whose offset is longer than eps dropped, order kept."""
    k = conf.numel()
    ps, pd = xyz_s[si.long()], xyz_d[di.long()]
    src = torch.cat([ps + off[:k], ps], dim=0)
    dst = torch.cat([pd, pd + off[k:]], dim=0)
    w = conf.repeat(2)
    keep = offset_cut(off, eps)
    return src[keep].t().contiguous(), dst[keep].t().contiguous(), w[keep], keep


def solve_svd_rounds(w, src, dst, num_iter: int = 3, std_ratio: float = 3.0):
    """oracle.dpm_oracle.solve_svd, line by line, that also returns the inlier mask every round STARTS from plus the final
    one (the host suite asserts the same R, T, mask and rmse bits as the oracle's own function on every case)."""
    it = 0
    inl = w > 0.5
    inl[torch.topk(w, k=min(64, len(w)), dim=0)[1]] = True
    masks = [inl.clone()]
    while True:
        s, d, ww = src[:, inl], dst[:, inl], w[inl]
        cs = (s * ww).sum(dim=1, keepdim=True) / ww.sum()
        cd = (d * ww).sum(dim=1, keepdim=True) / ww.sum()
        cov = (s - cs) @ torch.diag(ww) @ (d - cd).T
        u, _, v = torch.svd(cov.double())
        R = v @ u.T
        T = cd.double() - R @ cs.double()
        R, T = R.to(src.dtype), T.to(src.dtype)
        err = torch.norm(R @ src + T - dst, p=2, dim=0)
        new = err <= (err[inl].mean() + std_ratio * err[inl].std())
        it += 1
        stop = it >= num_iter or bool((inl == new).all()) or int(new.sum()) < 30
        inl = new
        masks.append(inl.clone())
        if stop:
            break
    rmse = (R @ src[:, inl] + T - dst[:, inl]).pow(2).sum(0).mean().sqrt().item()
    return R, T, inl, rmse, masks


def solve_svd64(w, src, dst, masks):
    """The last round of the loop with its inlier decisions forced to those of the fp32 run (masks from solve_svd_rounds) and
    every sum in double: -> (R (3,3), T (3,1), rmse) fp64, plus the singular values of the covariance."""
    w, src, dst = w.double(), src.double(), dst.double()
    inl, fin = masks[-2], masks[-1]
    s, d, ww = src[:, inl], dst[:, inl], w[inl]
    cs = (s * ww).sum(dim=1, keepdim=True) / ww.sum()
    cd = (d * ww).sum(dim=1, keepdim=True) / ww.sum()
    cov = ((s - cs) * ww) @ (d - cd).T
    u, sv, v = torch.svd(cov)
    R = v @ u.T
    T = cd - R @ cs
    rmse = float((R @ src[:, fin] + T - dst[:, fin]).pow(2).sum(0).mean().sqrt()) if bool(fin.any()) else float("nan")
    return R, T, rmse, sv


def straddling_tie(w: torch.Tensor) -> bool:
    """does a run of equal weights cross the 64th place of the descending order (torch.topk then has a choice)"""
    if w.numel() <= 64:
        return False
    s = w.sort(descending=True).values
    return bool(s[63] == s[64])


# ---------------------------------------------------------------------------------------------------------------------
# Kabsch cases
# ---------------------------------------------------------------------------------------------------------------------
def _motion():
    a, b = 0.2, -0.1
    Rz = torch.tensor([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]], dtype=torch.float64)
    Rx = torch.tensor([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]], dtype=torch.float64)
    return (Rz @ Rx), torch.tensor([0.5, 1.0, -0.25], dtype=torch.float64)


def _conf(kind: str, k: int, g: torch.Generator) -> torch.Tensor:
    if kind in ("plain", "high"):
        # a top-k output: descending, distinct by construction (one value per 1/k cell); "plain" stays below 0.5, "high" has
        # many entries above it, so that the w > 0.5 rule admits more than 64
        c = (torch.randperm(k, generator=g) + torch.rand(k, generator=g)) / k * (0.4 if kind == "plain" else 0.9) + 0.01
    elif kind in ("levels6", "levels40"):      # few distinct values (the existing tie test's): ties everywhere
        lv = int(kind[6:])
        c = torch.randint(0, lv, (k,), generator=g).float() / (2.5 * lv)
    elif kind == "highlevels6":  # tied AND above 0.5 at the 64th place: the 0.5 rule decides, nothing to replay
        c = torch.randint(0, 6, (k,), generator=g).float() * 0.15 + 0.05
    else:
        raise ValueError(kind)
    return c.sort(descending=True).values.contiguous()


# name -> k, seed, survivors of copy A / copy B (None = all), conf kind, coordinate shift, what the GPU test may assert:
#   "pose":     everything (counts, inlier list, pose, rmse)
#   "counts":   n_corr, n_inlier, iterations (std of the residuals undefined or the pose rank deficient)
#   "n_corr":   n_corr and iterations only (two mirror-image correspondences: the inlier cut sits ON both residuals)
def _spec(k, seed, keep_a=None, keep_b=None, conf="plain", shift=0.0, check="pose", noise=0.3):
    return dict(k=k, seed=seed, keep_a=keep_a, keep_b=keep_b, conf=conf, shift=shift, check=check, noise=noise)


KABSCH = {
    # 2k below, on, across one 256-thread round, across many; roughly a fifth of each copy cut
    "k1":            _spec(1, 1, check="n_corr"),
    "k20":           _spec(20, 1, 17, 15),
    "k127":          _spec(127, 1, 101, 99),
    "k128":          _spec(128, 1, 100, 103),
    "k129":          _spec(129, 1, 104, 97),
    "k640":          _spec(640, 1, 500, 530),
    "k2048":         _spec(2048, 1, 1700, 1500),
    "k4096":         _spec(4096, 1, 3500, 3300),           # the decoder's stated maximum
    "nothing_cut":   _spec(300, 7),                        # n = 2k; also fed to direct mode (distinct conf)
    "copy_a_cut":    _spec(300, 2, 0, 250),                # nA = 0
    "copy_b_cut":    _spec(300, 3, 260, 0),
    "under64":       _spec(300, 4, 22, 27),                # kk = n = 49
    "under30":       _spec(300, 5, 11, 14),                # 25 survivors: the loop leaves after its first round
    "one_survivor":  _spec(300, 6, 0, 1, check="counts"),
    "tie6_wave":     _spec(640, 2, 500, 530, conf="levels6"),     # kk * 64 > n: nth-element replay
    "tie40_wave":    _spec(640, 3, 500, 530, conf="levels40"),
    "tie6_heap":     _spec(2560, 4, 2300, 2200, conf="levels6"),  # kk * 64 <= n: heap replay
    "tie40_heap":    _spec(2560, 6, 2300, 2200, conf="levels40"),
    "high":          _spec(640, 6, 500, 530, conf="high"),
    "high_tied":     _spec(640, 7, 500, 530, conf="highlevels6"),
    "shift1000":     _spec(640, 18, 500, 530, shift=1000.0, noise=0.6),
    # the three elements of the batched call (same k, different survivor counts) and the empty element
    "batch0":        _spec(200, 1, 150, 170),
    "batch1":        _spec(200, 2, 200, 0),
    "batch2":        _spec(200, 3, 31, 9),
    "empty":         _spec(200, 4, 0, 0, check="empty"),
}
BATCH = ("batch0", "batch1", "batch2")
BATCH_WITH_EMPTY = ("batch0", "empty", "batch2")
TIED = ("tie6_wave", "tie40_wave", "tie6_heap", "tie40_heap", "high_tied")


def kabsch_case(name: str) -> dict:
    """-> off (2k,3), xyz_s (M,3), xyz_d (N,3), si, di (k,) int32, conf (k,), eps.  The target points come first; the paired
    source points are the target points moved back by one rigid motion plus noise (a tenth of them displaced by metres:
    outliers the rounds have to shed), so no pair shares a target and duplicate indices overwrite nothing."""
    sp = KABSCH[name]
    k = sp["k"]
    g = torch.Generator().manual_seed(1000 * sp["seed"] + k)
    M = N = k + 5
    R0, t0 = _motion()
    xyz_d = torch.randn(N, 3, generator=g) * 10
    xyz_s = torch.randn(M, 3, generator=g) * 10
    si = torch.randperm(M, generator=g)[:k]
    di = torch.randperm(N, generator=g)[:k]
    back = ((xyz_d[di].double() - t0) @ R0).float()          # R0^T (p - t0), row form
    back = back + sp["noise"] * torch.randn(k, 3, generator=g)
    out = torch.rand(k, generator=g) < 0.1
    back[out] += 5.0 * torch.randn(int(out.sum()), 3, generator=g)
    xyz_s[si] = back
    if sp["shift"]:
        xyz_s, xyz_d = xyz_s + sp["shift"], xyz_d + sp["shift"]
    # offsets: direction random, length <= 0.5 eps for the survivors and in [1.5, 3] eps for the cut ones
    d = torch.randn(2 * k, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    length = torch.rand(2 * k, generator=g) * 0.5 * EPS
    far = (1.5 + 1.5 * torch.rand(2 * k, generator=g)) * EPS
    for copy, kept in ((0, sp["keep_a"]), (1, sp["keep_b"])):
        if kept is not None:
            cut = torch.randperm(k, generator=g)[:k - kept] + copy * k
            length[cut] = far[cut]
    off = (d * length.unsqueeze(1)).contiguous()
    return dict(name=name, k=k, off=off, xyz_s=xyz_s.contiguous(), xyz_d=xyz_d.contiguous(), si=si.int(), di=di.int(),
                conf=_conf(sp["conf"], k, g), eps=EPS, check=sp["check"],
                n=(k if sp["keep_a"] is None else sp["keep_a"]) + (k if sp["keep_b"] is None else sp["keep_b"]))


_REF = {}


def kabsch_reference(name: str, num_iter: int = 3) -> dict:
    """case + restated correspondences + the oracle's loop on them (computed once per process, shared, never modified).
    num_iter = 1 stops after the first round: R, T are then those of the SEEDING (w > 0.5 plus the 64 largest), which the
    later rounds of the full loop otherwise wash out."""
    key = (name, num_iter)
    if key not in _REF:
        c = kabsch_case(name)
        src, dst, w, keep = correspondences(c["off"], c["xyz_s"], c["xyz_d"], c["si"], c["di"], c["conf"], c["eps"])
        ref = dict(c, src=src, dst=dst, w=w, keep=keep)
        if w.numel():
            margins = []
            R, T, inl, rmse = O.solve_svd(w, src, dst, num_iter=num_iter, margins=margins)
            _, _, _, _, masks = solve_svd_rounds(w, src, dst, num_iter=num_iter)
            ref.update(R=R, T=T, inl=inl, rmse=rmse, margins=margins, masks=masks, iterations=len(masks) - 1)
        _REF[key] = ref
    return _REF[key]


def wide_rows(xyz: torch.Tensor, fill: float = -7.0) -> torch.Tensor:
    """(R,3) -> the (R,3) view at column XYZ_COL of an (R, LD) buffer, as the decoder hands coordinates to the kernel"""
    buf = torch.full((xyz.shape[0], LD), fill, dtype=torch.float32)
    buf[:, XYZ_COL:XYZ_COL + 3] = xyz
    return buf


# ---------------------------------------------------------------------------------------------------------------------
# gather_pairs
# ---------------------------------------------------------------------------------------------------------------------
GATHER_PAIRS = [(1, 5, 7, 3, 4), (2, 64, 64, 256, 2048), (3, 37, 200, 96, 500), (1, 4096, 256, 256, 1088)]


def gather_pairs_case(B, M, N, E, k, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * k)
    x, y = torch.randn(B, M, E, generator=g), torch.randn(B, N, E, generator=g)
    flat = torch.randint(0, M * N, (B, k), generator=g, dtype=torch.int32)
    flat[:, 0], flat[:, -1] = 0, M * N - 1
    if k >= 4:
        flat[:, 2] = flat[:, 1]                                # a repeat
    return x, y, flat


def gather_pairs(x, y, flat):
    """x (B,M,E), y (B,N,E), flat (B,k) -> X (B,2k,2E), si, di (B,k) int32"""
    N = y.shape[1]
    si, di = flat // N, flat % N
    bi = torch.arange(x.shape[0]).unsqueeze(1)
    xs, yd = x[bi, si.long()], y[bi, di.long()]
    return torch.cat([torch.cat([xs, yd], 2), torch.cat([yd, xs], 2)], 1), si.int(), di.int()


# ---------------------------------------------------------------------------------------------------------------------
# map tile
# ---------------------------------------------------------------------------------------------------------------------
def _rot(g):
    q = torch.randn(4, generator=g, dtype=torch.float64)
    w, x, y, z = (q / q.norm()).tolist()
    return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=torch.float64)


# (n scans, C, S, select or None)
MAP_TILE = {
    "one_scan":      (1, 131, 256, None),
    "all_in_order":  (5, 131, 255, None),
    "repeat_back":   (6, 131, 300, [4, 1, 4, 0, 5]),      # a scan twice, non-monotone
    "one_point":     (3, 4, 1, [2, 0]),
    "c4":            (4, 4, 300, [3, 3, 1]),
    "c131_s1":       (3, 131, 1, [1, 2, 0]),
}


def map_tile_case(name):
    """KITTI-scale: scans a few metres across (descriptor xyz rows in metres), poses hundreds of metres from the origin, the
    centring pose among them -- the tile is small, the intermediates are large."""
    n, C, S, sel = MAP_TILE[name]
    g = torch.Generator().manual_seed(11 + n * 1000 + S)
    kp = torch.randn(n, C, S, generator=g)
    kp[:, -3:, :] *= 20.0
    base = torch.tensor([412.0, -655.0, 38.0], dtype=torch.float64)
    poses = torch.eye(4, dtype=torch.float64).repeat(n, 1, 1)
    for i in range(n):
        poses[i, :3, :3] = _rot(g)
        poses[i, :3, 3] = base + 15.0 * torch.randn(3, generator=g, dtype=torch.float64)
    centre = poses[n // 2].clone()
    return kp, poses.float(), centre.float(), sel


def map_tile64(kp, poses, centre, sel):
    """fp64: feature rows copied, xyz rows R_c^T ((R_k x + t_k) - t_c), scans in `sel` order"""
    order = list(range(kp.shape[0])) if sel is None else list(sel)
    kp, poses, centre = kp.double(), poses.double(), centre.double()
    parts = []
    for i in order:
        p = kp[i].clone()
        p[-3:] = centre[:3, :3].T @ ((poses[i, :3, :3] @ p[-3:] + poses[i, :3, 3:]) - centre[:3, 3:])
        parts.append(p)
    return torch.cat(parts, dim=1)


def map_tile32(kp, poses, centre, sel):
    """the oracle's fp32 statement of the same"""
    order = list(range(kp.shape[0])) if sel is None else list(sel)
    return O.map_tile([kp[i] for i in order], [poses[i] for i in order], centre)


# ---------------------------------------------------------------------------------------------------------------------
# the copy and reduce kernels
# ---------------------------------------------------------------------------------------------------------------------
def emit_descriptors(xyz, fea, lengths, scale):
    """xyz (B,S,3), fea (B,S,C), lengths (B,) -> coor (B,3,S), feat (B,C,S), padding (B,S) bool, desc (B,C+3,S) or None"""
    S = xyz.shape[1]
    coor, feat = xyz.transpose(1, 2).contiguous(), fea.transpose(1, 2).contiguous()
    padding = torch.arange(S).unsqueeze(0) >= lengths.unsqueeze(1)
    desc = torch.cat([feat, coor * torch.tensor(scale, dtype=torch.float32)], dim=1) if scale > 0 else None
    return coor, feat, padding, desc


def nested_levels(xyz0, len0, npoints):
    """xyz0 (B,K0,3), len0 (B,) -> per K: (idx (B,K) int32 = position or -1 past the valid count, xyz0[:, :K], min(len0, K))"""
    out = []
    for K in npoints:
        j = torch.arange(K, dtype=torch.int32).unsqueeze(0).expand(xyz0.shape[0], K)
        ln = torch.clamp(len0, max=K).int()
        out.append((torch.where(j < ln.unsqueeze(1), j, torch.full_like(j, -1)), xyz0[:, :K].contiguous(), ln))
    return out


def l2_normalize64(x):
    """F.normalize in double: x / max(|x|, 1e-12)"""
    x = x.double()
    return x / x.norm(dim=-1, keepdim=True).clamp(min=1e-12)


def l2_bound(C: int) -> float:
    """relative error per element of one wave's fp32 row norm and quotient: ceil(C / 64) fused adds per lane, six adds of the
    wave reduction, the square root and the division, each at most 2^-24 (the norm's error is half that of the sum of
    squares, which only helps)"""
    return (-(-C // 64) + 8) * 2.0 ** -24


def mean_rows_bound(x):
    """(B,R,C) -> (B,C): the recursive-sum bound of the mean, (R - 1) 2^-24 mean|x| per column"""
    R = x.shape[1]
    return (R - 1) * 2.0 ** -24 * x.double().abs().mean(dim=1)


def dim_t(emb_dim: int = 256, temperature: float = 10000.0):
    """the position embedding's frequency table, the reference's torch expression (descriptor_attention.py:71-72)"""
    nf = emb_dim // 3 // 2 * 2
    i = torch.arange(nf, dtype=torch.float32)
    return temperature ** (2 * torch.div(i, 2, rounding_mode="trunc") / nf)
