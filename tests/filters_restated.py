"""The scan filters' kernels restated in plain numpy, over ALL pairs: no KD-tree, no candidate shortlist, nothing of the code
under test.  Each function states the rule the header comment of its kernel states (csrc/knn.hip: knn_self_kernel,
point_normals_kernel, ball_query_kernel, knn_grid_build_kernel; csrc/preprocess.hip: lowpass_sim_kernel, stat_filter_kernel).

fp32 arithmetic is restated with np.float32 arrays, one rounding per operation, in the order the kernel writes it (the library
is compiled without contraction, so `a * b + c` there is two roundings as it is here).  The two fused multiply-adds of the
expanded-form distance of ball_query have no numpy counterpart: each is evaluated in fp64 and rounded once to fp32.  That equals
the fused result only when the fp64 evaluation is itself exact, which `_fma32` ASSERTS (an error-free transformation of the
fp64 sum); it holds for coordinates on a dyadic lattice of small magnitude, which is what every ball-query case uses.

Rows are processed in chunks (a few threads, numpy releases the interpreter lock) so that the 82 092-point real frame -- 6.7e9
pairs -- needs about 1 GB and some seconds."""
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

F32 = np.float32
THREADS = max(1, min(16, os.cpu_count() or 1))


def _chunks(n, step):
    return [(s, min(s + step, n)) for s in range(0, n, step)]


def _map(fn, jobs):
    if len(jobs) <= 1 or THREADS == 1:
        return [fn(j) for j in jobs]
    with ThreadPoolExecutor(THREADS) as ex:
        return list(ex.map(fn, jobs))


def direct_d2(q, p, out=None, tmp=None):
    """fp32 direct-form squared distances (dx*dx + dy*dy) + dz*dz of the rows of q (M,3) to the rows of p (N,3) -> (M,N) f32
    (out / tmp: optional (M,N) f32 buffers, so that a loop over chunks allocates nothing)"""
    q, p = np.asarray(q, dtype=F32), np.asarray(p, dtype=F32)
    shape = (q.shape[0], p.shape[0])
    out = np.empty(shape, dtype=F32) if out is None else out[:shape[0]]
    tmp = np.empty(shape, dtype=F32) if tmp is None else tmp[:shape[0]]
    np.subtract(q[:, None, 0], p[None, :, 0], out=out)
    np.multiply(out, out, out=out)
    for k in (1, 2):
        np.subtract(q[:, None, k], p[None, :, k], out=tmp)
        np.multiply(tmp, tmp, out=tmp)
        np.add(out, tmp, out=out)
    return out


# ------------------------------------------------------------------------------------------------------------------
# knn_self_kernel
# ------------------------------------------------------------------------------------------------------------------
def mean_dist_of(dist2, K):
    """(mean_dist as the kernel's fp32 sequence, its fp64 value) of the K columns of dist2 (N,K) f32"""
    dist2 = np.asarray(dist2, dtype=F32)
    acc = np.zeros(dist2.shape[0], dtype=F32)
    for k in range(K):                                   # sqrt per column, summed in column order
        acc = acc + np.sqrt(dist2[:, k])
    return acc / F32(K), np.sqrt(dist2.astype(np.float64)).sum(1) / K


def knn_self(xyz, K, tie="smallest", chunk=256):
    """The K+1 smallest of ALL N points (the query itself among them) by (fp32 direct-form d^2, index); rank 0 is dropped,
    whatever index it holds; N < K+1 leaves the missing columns at (q, 0.0).
    -> dict idx (N,K) int32, dist2 (N,K) f32, mean_dist (N,) f32 [the kernel's sequence], mean_dist64 (N,) f64.
    tie='largest' is NOT the kernel's rule: it breaks equal distances by the LARGEST index (the host test measures with it how
    many rows of a case a wrong tie rule would change)."""
    p = np.ascontiguousarray(xyz, dtype=F32)
    N = p.shape[0]
    K1 = min(K + 1, N)
    chunk = max(16, min(chunk, (1 << 23) // N))                         # at most 8 M pairs (32 MB) per buffer
    col = np.arange(N, dtype=np.uint64)
    if tie == "largest":
        col = np.uint64(N - 1) - col

    local = threading.local()

    def rows(se):
        s, e = se
        if not hasattr(local, "buf"):
            local.buf = [np.empty((min(chunk, N), N), dtype=F32) for _ in range(2)]
        d2 = direct_d2(p[s:e], p, local.buf[0], local.buf[1])
        sel = local.buf[1][:e - s]
        np.copyto(sel, d2)
        sel.partition(K1 - 1, axis=1)
        kth = sel[:, K1 - 1].copy()                                     # the (K+1)-th smallest distance of every row
        r, c = np.nonzero(d2 <= kth[:, None])                           # everything up to it, ties included: >= K+1 per row
        # a non-negative float orders like its bit pattern: one 64-bit key carries (distance, index)
        key = (d2[r, c].view(np.uint32).astype(np.uint64) << np.uint64(32)) | col[c]
        order = np.lexsort((key, r))
        first = np.searchsorted(r, np.arange(e - s))                    # r is ascending: where every row starts
        key = key[order][first[:, None] + np.arange(K1)[None, :]]
        i = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
        if tie == "largest":
            i = N - 1 - i
        return i, (key >> np.uint64(32)).astype(np.uint32).view(F32)

    parts = _map(rows, _chunks(N, chunk))
    idx = np.tile(np.arange(N, dtype=np.int32)[:, None], (1, K))
    dist2 = np.zeros((N, K), dtype=F32)
    idx[:, :K1 - 1] = np.concatenate([a for a, _ in parts])[:, 1:]
    dist2[:, :K1 - 1] = np.concatenate([b for _, b in parts])[:, 1:]
    m32, m64 = mean_dist_of(dist2, K)
    return {"idx": idx, "dist2": dist2, "mean_dist": m32, "mean_dist64": m64}


def knn_prefix(full, K):
    """the answer for a smaller K from the answer for a larger one (N > the larger K): the first K columns of the ordered list"""
    d2 = np.ascontiguousarray(full["dist2"][:, :K])
    m32, m64 = mean_dist_of(d2, K)
    return {"idx": np.ascontiguousarray(full["idx"][:, :K]), "dist2": d2, "mean_dist": m32, "mean_dist64": m64}


# ------------------------------------------------------------------------------------------------------------------
# point_normals_kernel
# ------------------------------------------------------------------------------------------------------------------
def _members(p, s, e, radius, rule):
    d2 = direct_d2(p[s:e], p)
    r2 = F32(radius * radius)
    return d2 <= r2 if rule == "<=" else d2 < r2


def _normal_of(cov):
    w, v = np.linalg.eigh(cov)
    n = v[:, 0]
    return n / np.linalg.norm(n), w


def point_normals(xyz, radius, rule="<", chunk=256):
    """Members of row i: every point (i itself included) whose fp32 direct-form d^2 is STRICTLY below float32(radius^2).  fp64
    cumulants of the members, covariance E[x x^T] - m m^T, np.linalg.eigh, unit eigenvector of the smallest eigenvalue; fewer
    than 3 members -> (0, 0, 1).  -> dict normals (N,3) f64, count (N,), eig (N,3) ascending, maxsq (N,) = max |x|^2 of the members.
    rule='<=' is NOT the kernel's rule (the host test measures with it what an inclusive radius would change)."""
    p = np.ascontiguousarray(xyz, dtype=F32)
    P = p.astype(np.float64)
    N = p.shape[0]
    iu = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    feat = np.concatenate([np.ones((N, 1)), P, np.stack([P[:, a] * P[:, b] for a, b in iu], 1)], 1)      # (N,10)
    sq = (P * P).sum(1)

    def rows(se):
        s, e = se
        mem = _members(p, s, e, radius, rule)
        return mem.astype(np.float64) @ feat, np.where(mem, sq[None, :], 0.0).max(1)

    parts = _map(rows, _chunks(N, chunk))
    cum, maxsq = np.concatenate([a for a, _ in parts]), np.concatenate([b for _, b in parts])
    normals = np.tile(np.array([0.0, 0.0, 1.0]), (N, 1))
    eig = np.zeros((N, 3))
    for i in np.nonzero(cum[:, 0] >= 3)[0]:
        n = cum[i, 0]
        m = cum[i, 1:4] / n
        cov = np.empty((3, 3))
        for k, (a, b) in enumerate(iu):
            cov[a, b] = cov[b, a] = cum[i, 4 + k] / n - m[a] * m[b]
        normals[i], eig[i] = _normal_of(cov)
    return {"normals": normals, "count": cum[:, 0].astype(np.int64), "eig": eig, "maxsq": maxsq}


def point_normals_centred(xyz, radius, rule="<", chunk=256):
    """the same normals a second way: the members' coordinates centred on their mean in np.longdouble before the covariance is
    formed (no cancellation of large cumulants) -> normals (N,3) f64.  The host test bounds the angle between the two."""
    p = np.ascontiguousarray(xyz, dtype=F32)
    N = p.shape[0]
    PL = p.astype(np.longdouble)
    normals = np.tile(np.array([0.0, 0.0, 1.0]), (N, 1))
    for s, e in _chunks(N, chunk):
        mem = _members(p, s, e, radius, rule)
        for i in range(s, e):
            nb = np.nonzero(mem[i - s])[0]
            if nb.size < 3:
                continue
            c = PL[nb] - PL[nb].mean(0)
            normals[i], _ = _normal_of((c.T @ c / nb.size).astype(np.float64))
    return normals


def normals_bound(res):
    """the per-row bound on sin(angle) between two evaluations of the same normal (the issue's formula): cumulants of up to 64-term
    fp64 sums of magnitude max|x|^2, against the gap between the two smallest eigenvalues; rows with < 3 members are exact"""
    gap = res["eig"][:, 1] - res["eig"][:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        b = 2.0 * 64.0 * 2.0 ** -52 * res["maxsq"] / gap + 2.0 ** -22
    return np.where(res["count"] >= 3, np.where(gap > 0, b, np.inf), 0.0)


def sin_angle(a, b):
    return np.linalg.norm(np.cross(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)), axis=1)


# ------------------------------------------------------------------------------------------------------------------
# lowpass_sim_kernel
# ------------------------------------------------------------------------------------------------------------------
def lowpass_similarity(normals, idx, flux):
    """sum of the `flux` largest |n_j . n_i| over the row's neighbours j, in fp64 -> (N,) f64"""
    n = np.asarray(normals, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    v = np.abs((n[idx] * n[:, None, :]).sum(-1))
    return np.sort(v, axis=1)[:, ::-1][:, :flux].sum(1)


# ------------------------------------------------------------------------------------------------------------------
# stat_filter_kernel
# ------------------------------------------------------------------------------------------------------------------
def stat_threshold(stat, k_std, mode):
    """-> (mean_f, std_f, thr) as float32: fp64 mean and unbiased variance (0 for N = 1), each rounded to fp32, then
    thr = float32(mean_f +- float32(float32(k_std) * std_f))"""
    s = np.asarray(stat, dtype=F32).astype(np.float64)
    N = s.shape[0]
    with np.errstate(invalid="ignore"):
        mean = s.sum() / N
        var = ((s - mean) ** 2).sum() / (N - 1) if N > 1 else 0.0
        mean_f, std_f = F32(mean), F32(np.sqrt(var))
        prod = F32(F32(k_std) * std_f)
        thr = F32(mean_f + prod) if mode == 0 else F32(mean_f - prod)
    return mean_f, std_f, thr


def stat_filter(stat, k_std, mode, xyz, idx_in=None, ratio=1.0, cut=None):
    """mode 0 keeps stat <= thr, mode 1 keeps stat > thr; survivors in order, coordinates through a true fp32 division by
    float32(ratio), indices from idx_in or arange -> (xyz_out (M,3) f32, idx_out (M,) int32, M).
    cut = '<' / '>=' is NOT the kernel's rule (the host test measures with it what the other comparison would change)."""
    stat = np.asarray(stat, dtype=F32)
    _, _, thr = stat_threshold(stat, k_std, mode)
    op = cut or ("<=" if mode == 0 else ">")
    with np.errstate(invalid="ignore"):
        keep = {"<=": stat <= thr, "<": stat < thr, ">": stat > thr, ">=": stat >= thr}[op]
    src = np.arange(stat.shape[0], dtype=np.int32) if idx_in is None else np.asarray(idx_in, dtype=np.int32)
    out = np.asarray(xyz, dtype=F32)[keep] / F32(ratio)
    return out.astype(F32), src[keep], int(keep.sum())


# ------------------------------------------------------------------------------------------------------------------
# ball_query_kernel
# ------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """float32(a * b + c) with ONE rounding, for float32 arrays: the product of two floats is exact in fp64; the fp64 sum is
    checked to be exact as well (TwoSum), so the one conversion to fp32 is the only rounding, as in a fused multiply-add"""
    t = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = t + c
    bb = s - t
    err = (t - (s - bb)) + (c - bb)
    assert not err.any(), "fp64 evaluation of the fused multiply-add is not exact for this input: keep ball-query inputs on a small lattice"
    return s.astype(F32)


def _sq3(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def expanded_d2(c, p):
    """the reference's expanded form ((-2 * fma(cz,z, fma(cy,y, cx*x))) + |c|^2) + |p|^2 of centres c (S,3) to points p (N,3)"""
    c, p = np.asarray(c, dtype=F32), np.asarray(p, dtype=F32)
    caa, bb = _sq3(c), _sq3(p)
    S, N = c.shape[0], p.shape[0]
    bc = lambda a, b: (np.broadcast_to(a[:, None], (S, N)), np.broadcast_to(b[None, :], (S, N)))
    cx, x = bc(c[:, 0], p[:, 0])
    cy, y = bc(c[:, 1], p[:, 1])
    cz, z = bc(c[:, 2], p[:, 2])
    dot = _fma32(cz, z, _fma32(cy, y, cx * x))
    return ((F32(-2.0) * dot) + caa[:, None]) + bb[None, :]


def ball_query(points, lengths, centers, K, radius):
    """points (B,N,3), lengths (B,), centers (B,S,3) -> (B,S,K) int32: the first K indices below lengths[b], ascending, whose
    expanded-form distance is not above float32(radius^2), padded with the first of them; nothing in range -> 0 in every slot"""
    points, centers = np.asarray(points, dtype=F32), np.asarray(centers, dtype=F32)
    B, N, _ = points.shape
    S = centers.shape[1]
    r2 = F32(radius * radius)
    out = np.zeros((B, S, K), dtype=np.int32)
    for b in range(B):
        n = int(min(max(int(lengths[b]), 0), N))
        if n == 0:
            continue
        keep = ~(expanded_d2(centers[b], points[b, :n]) > r2)
        for s in range(S):
            hit = np.nonzero(keep[s])[0][:K]
            if hit.size:
                out[b, s, :hit.size] = hit
                out[b, s, hit.size:] = hit[0]
    return out


# ------------------------------------------------------------------------------------------------------------------
# knn_grid_build_kernel, as the self search uses it (r2_margin = 0: cell edge = max(cell, extent / 127))
# ------------------------------------------------------------------------------------------------------------------
GDIM = 128


def grid_geometry(xyz, cell):
    """-> dict lox, loy, cs, inv_cs (float32), g, cx, cy (N,) int, count (g,g) int [count[cy, cx]], block3 (N,) = points in the
    3x3 cells around every point's cell.  Used by the host test only, to prove that a case reaches the path it is named for."""
    p = np.ascontiguousarray(xyz, dtype=F32)
    lox, loy = p[:, 0].min(), p[:, 1].min()
    ext = max(max(F32(p[:, 0].max() - lox), F32(p[:, 1].max() - loy)), F32(1e-6))
    cs = max(F32(cell), F32(ext / F32(GDIM - 1)))
    inv_cs = F32(F32(1.0) / cs)
    g = min(GDIM, int(F32(ext * inv_cs)) + 1)
    cx = np.clip(np.floor((p[:, 0] - lox) * inv_cs).astype(np.int64), 0, g - 1)
    cy = np.clip(np.floor((p[:, 1] - loy) * inv_cs).astype(np.int64), 0, g - 1)
    count = np.zeros((g, g), dtype=np.int64)
    np.add.at(count, (cy, cx), 1)
    pad = np.pad(count, 1)
    box = sum(pad[1 + dy:1 + dy + g, 1 + dx:1 + dx + g] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    return {"lox": lox, "loy": loy, "cs": cs, "inv_cs": inv_cs, "g": g, "cx": cx, "cy": cy, "count": count, "block3": box[cy, cx]}
