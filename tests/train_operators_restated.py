"""The decoder's training operators (csrc/offset_pairs.hip, csrc/attention_train.hip) restated plainly, and the small inputs
their kernel-by-kernel tests share.  No project imports: numpy for what must be reproduced byte for byte (one float32 rounding
per operation), torch autograd for attention.

The restatements are pinned on the CPU by tests/test_train_operators_host.py (known answers, torch.nonzero of the dense mask,
mutants that must be told apart) so that tests/test_gpu_train_operators.py cannot agree with a kernel by sharing its mistake.
"""
import numpy as np
import torch

F32 = np.float32
INT32_MAX = 2 ** 31 - 1


# ---- restatements ----------------------------------------------------------------------------------------------------------

def pair_list(xa, xb, pad_a, pad_b, eps):
    """xa (B,3,M), xb (B,3,N) float32, pad_a (B,M), pad_b (B,N) bool (True = padding) ->
    (triples (K,3) int32 in (batch, a, b) lexicographic order, offsets_a (B*M+1,) int64, offsets_b (B*N+1,) int64,
    perm_b (K,) int64: the pairs stably sorted by (batch, b)).
    d2 = (dx dx + dy dy) + dz dz in float32, one rounding per operation; a pair is kept when d2 <= float32(eps_double^2); a NaN
    distance compares false and is dropped; padded rows and columns are dropped."""
    xa, xb = np.asarray(xa), np.asarray(xb)
    assert xa.dtype == F32 and xb.dtype == F32
    B, _, M = xa.shape
    N = xb.shape[2]
    eps2 = F32(np.float64(eps) * np.float64(eps))
    triples, cnt_a, cnt_b = [], np.zeros(B * M, np.int64), np.zeros(B * N, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            dx = xa[b, 0][:, None] - xb[b, 0][None, :]
            dy = xa[b, 1][:, None] - xb[b, 1][None, :]
            dz = xa[b, 2][:, None] - xb[b, 2][None, :]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == F32
            keep = (d2 <= eps2) & ~pad_a[b][:, None] & ~pad_b[b][None, :]
            ia, ib = np.nonzero(keep)          # row-major: ascending a, then ascending b
            triples.append(np.stack([np.full(ia.shape, b), ia, ib], axis=1))
            cnt_a[b * M:(b + 1) * M] = keep.sum(axis=1)
            cnt_b[b * N:(b + 1) * N] = keep.sum(axis=0)
    triples = np.concatenate(triples).astype(np.int32)
    off_a = np.concatenate([[0], np.cumsum(cnt_a)])
    off_b = np.concatenate([[0], np.cumsum(cnt_b)])
    perm_b = np.argsort(triples[:, 0].astype(np.int64) * N + triples[:, 2], kind="stable")
    return triples, off_a, off_b, perm_b


def offsets_clipped(counts):
    """exclusive scan of `counts` in Python ints -> list of len(counts) + 1: every entry clipped at 2^31 - 1, the last one (the
    total) -1 where it exceeds 2^31 - 1"""
    out, run = [], 0
    for c in counts:
        out.append(min(run, INT32_MAX))
        run += int(c)
    out.append(-1 if run > INT32_MAX else run)
    return out


def segment_sum_ordered(g, offsets, perm):
    """g (K,E) float32, offsets (R+1,), perm (K,) or None -> (R,E) float32: out[r] = the sum of g[perm[k]] (g[k] without perm)
    for k = offsets[r] .. offsets[r+1] - 1 in that order, a float32 accumulator that starts at +0 and takes one add per step"""
    g = np.asarray(g)
    assert g.dtype == F32
    R = len(offsets) - 1
    out = np.zeros((R, g.shape[1]), F32)
    for r in range(R):
        acc = np.zeros(g.shape[1], F32)
        for k in range(int(offsets[r]), int(offsets[r + 1])):
            acc = acc + g[int(perm[k]) if perm is not None else k]
        out[r] = acc
    return out


def attention_dense(q, k, v, B, M, N, heads, mask, dtype):
    """q (B*M,E), k, v (B*N,E), E = 32 heads, mask (B,N) non-zero = padding key or None -> (out (B*M,E), lse (B,heads,M)):
    softmax(q k^T / sqrt(32) over the unmasked keys) v and the log-sum-exp of every score row, dense, in `dtype` on the
    operands' device, differentiable by autograd"""
    E = 32 * heads
    h = lambda t, n: t.to(dtype).view(B, n, heads, 32).transpose(1, 2)   # noqa: E731
    s = h(q, M) @ h(k, N).transpose(-1, -2) / 32 ** 0.5
    if mask is not None:
        s = s.masked_fill(mask.bool()[:, None, None, :], float("-inf"))
    return (torch.softmax(s, -1) @ h(v, N)).transpose(1, 2).reshape(B * M, E), torch.logsumexp(s, -1)


# ---- inputs of section A ---------------------------------------------------------------------------------------------------

EPS = 1.0
RAGGED_SHAPES = [(1, 1, 1), (2, 255, 257), (3, 257, 255), (2, 256, 513), (1, 600, 256), (2, 300, 700)]
CHUNK_EDGE_N = (257, 513, 700)   # for these N, b columns 255, 256 and N - 1 are padding with a live a point exactly on each


def ragged_case(B, M, N, seed=0, eps=EPS, per_row=6.0):
    """Uniform points in a cube sized for about `per_row` pairs per row, ragged lengths on both sides (the first sequence of
    each side is complete), a few padded tokens inside.  Every padded token sits exactly on a live token of the other side, so a
    missed pad test lists it.  -> dict(xa, xb, pad_a, pad_b, eps)"""
    rng = np.random.default_rng(1000 * seed + 7 * B + 31 * M + N)
    side = eps * (N * 4.19 / per_row) ** (1.0 / 3.0)
    xa = (rng.random((B, 3, M)) * side).astype(F32)
    xb = (rng.random((B, 3, N)) * side).astype(F32)
    pad_a, pad_b = np.zeros((B, M), bool), np.zeros((B, N), bool)
    for b in range(B):
        for pad, n in ((pad_a, M), (pad_b, N)):
            if b > 0:
                pad[b, n - int(rng.integers(1, n // 2 + 1)):] = True
            if n > 16:
                pad[b, rng.integers(8, n // 2, size=3)] = True
        if N in CHUNK_EDGE_N:
            cols = [255, 256, N - 1]
            pad_b[b, cols] = True
            pad_a[b, :3] = False
            xa[b, :, :3] = xb[b][:, cols]
    for b in range(B):
        edge = (255, 256, N - 1) if N in CHUNK_EDGE_N else ()
        live_a, live_b = np.nonzero(~pad_a[b])[0][len(edge):], np.nonzero(~pad_b[b])[0]
        for i in np.nonzero(pad_a[b])[0]:
            xa[b, :, i] = xb[b, :, live_b[i % len(live_b)]]
        for j in np.nonzero(pad_b[b])[0]:
            if j not in edge:
                xb[b, :, j] = xa[b, :, live_a[j % len(live_a)]]
    return dict(xa=xa, xb=xb, pad_a=pad_a, pad_b=pad_b, eps=eps)


def _one_batch(pa, pb, eps, pad_a=None, pad_b=None):
    pa, pb = np.asarray(pa, F32), np.asarray(pb, F32)
    return dict(xa=np.ascontiguousarray(pa.T[None]), xb=np.ascontiguousarray(pb.T[None]),
                pad_a=np.zeros((1, len(pa)), bool) if pad_a is None else np.asarray(pad_a, bool)[None],
                pad_b=np.zeros((1, len(pb)), bool) if pad_b is None else np.asarray(pad_b, bool)[None], eps=eps)


def _rounding_case(eps, dy):
    """one a point at the origin and one b point at (dx, dy, 0) with d2 = fl(fl(dx dx) + dy dy) EXACTLY the larger of
    float32(eps_double^2) and float32(float32(eps)^2) (they must differ): dx is looked for among the float32 neighbours of the
    square root.  -> (case, kept): kept says whether the pair is listed (the larger value is the true eps2) or not."""
    true2, mut2 = F32(np.float64(eps) * np.float64(eps)), F32(F32(eps) * F32(eps))
    assert true2 != mut2, eps
    tgt, dy = max(true2, mut2), F32(dy)
    x = F32(np.sqrt(np.float64(tgt) - np.float64(dy) * np.float64(dy)))
    for _ in range(8):
        x = np.nextafter(x, F32(0))
    for _ in range(17):
        if F32(F32(x * x) + F32(dy * dy)) == tgt:
            return _one_batch([[0, 0, 0]], [[x, dy, 0]], eps), bool(tgt == true2)
        x = np.nextafter(x, F32(np.inf))
    raise AssertionError(f"no float32 dx puts d2 on {tgt!r} (eps {eps}, dy {dy})")


def lattice_cases():
    """-> {name: (case, expected (K,3) list of triples or None where pair_list is the only expectation)}

    near / far    a_i = (0.25 i, 0, 16 i) (+ 4096 on every axis), b_i = a_i + (0.75, y_i, 0), eps = 1.25 (eps^2 = 1.5625 exact):
                  y = 1: d2 = 0.5625 + 1 = eps^2, kept; y one float32 above 1: dropped; one below: kept.  At 4096 the spacing is
                  2^-11, y = 1 +- 2^-11 and every difference and square is still exact (1 + 2^-10 + 2^-22 has 23 bits).
    eps_zero      coincident points pair, a neighbour one ulp away does not
    eps_inf       every unpadded pair
    eps_0.1       d2 = float32(float32(0.1)^2) = 0.010000001 > float32(0.1 x 0.1 in double) = 0.01: dropped; a comparison
                  against the float32 square keeps it
    eps_0.7       d2 = float32(0.49) > float32(float32(0.7)^2) = 0.48999998: kept; the float32 square drops it
    The issue's example eps = 0.3 tells nothing apart: float32(0.3)^2 rounds to float32(0.09) as well (so do 0.6 and 1.1); 0.1
    and 0.7 differ, one in each direction."""
    one = F32(1.0)
    cases = {}
    for name, origin, ys in (("near", 0.0, (one, np.nextafter(one, F32(2)), np.nextafter(one, F32(0)))),
                             ("far", 4096.0, (one, F32(1 + 2.0 ** -11), F32(1 - 2.0 ** -11)))):
        pa = [[origin + 0.25 * i, origin, origin + 16.0 * i] for i in range(3)]
        pb = [[F32(origin + 0.25 * i + 0.75), F32(origin) + ys[i], origin + 16.0 * i] for i in range(3)]
        cases[name] = (_one_batch(pa, pb, 1.25), [(0, 0, 0), (0, 2, 2)])
    five = F32(5.0)
    cases["eps_zero"] = (_one_batch([[1, 2, 3], [5, 5, 5]], [[1, 2, 3], [np.nextafter(five, F32(6)), 5, 5]], 0.0), [(0, 0, 0)])
    c = ragged_case(2, 12, 9, seed=3)
    live = [(b, i, j) for b in range(2) for i in range(12) for j in range(9) if not c["pad_a"][b, i] and not c["pad_b"][b, j]]
    cases["eps_inf"] = (dict(c, eps=float("inf")), live)
    c, kept = _rounding_case(0.1, 0.0)
    assert not kept
    cases["eps_0.1"] = (c, [])
    c, kept = _rounding_case(0.7, 0.5)
    assert kept
    cases["eps_0.7"] = (c, [(0, 0, 0)])
    return cases


def nan_case():
    """-> (clean case, case with a NaN coordinate in one a row and one b column, (batch, a row), (batch, b column)): both named
    tokens have pairs in the clean case"""
    clean = ragged_case(2, 40, 50, seed=5, per_row=12.0)
    t = pair_list(**clean)[0]
    ra = tuple(int(v) for v in t[t[:, 0] == 0][0][:2])
    rb = tuple(int(v) for v in t[t[:, 0] == 1][-1][[0, 2]])
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in clean.items()}
    bad["xa"][ra[0], 1, ra[1]] = np.nan
    bad["xb"][rb[0], 0, rb[1]] = np.nan
    return clean, bad, ra, rb


SCAN_ROWS = (1, 255, 257, 1000)
SCAN_WHERE = ("first", "last", "none", "mixed")
SCAN_SITES = (1, 2, 3, 4)   # b points per site; a fifth site is empty


def scan_case(R, where):
    """B = 1, M = R rows against N = 10 b points that sit on four sites (1, 2, 3, 4 coincident points) 10 m apart.
    first / last: that row alone sits on the 4-point site; none: no row near any; mixed: row r sits on site (3 r + 2) % 5, site 4
    being empty.  -> (case, counts (R,) as a list of ints: known by construction)"""
    pb = [[10.0 * s, 0, 0] for s, n in enumerate(SCAN_SITES) for _ in range(n)]
    site = {"first": lambda r: 3 if r == 0 else 4, "last": lambda r: 3 if r == R - 1 else 4, "none": lambda r: 4,
            "mixed": lambda r: (3 * r + 2) % 5}[where]
    pa = [[10.0 * site(r), 0.25 * (r % 3), 0] if site(r) < 4 else [1000.0 + r, 0, 0] for r in range(R)]
    counts = [SCAN_SITES[site(r)] if site(r) < 4 else 0 for r in range(R)]
    return _one_batch(pa, pb, EPS), counts


def hub_case():
    """B = 2, M = 310, N = 320: a_0 and b_0..299 on one site (a row with 300 pairs), b_300 and a_1..300 on another (a column with
    300), a_301 / b_301 a single pair, everything else alone; the second sequence is the first with both token orders reversed
    and its last five tokens of each side padded (they sit on the single pair's site)."""
    M, N = 310, 320
    pa = np.array([[2000.0 + 10 * i, 0, 0] for i in range(M)], F32)
    pb = np.array([[0, 3000.0 + 10 * j, 0] for j in range(N)], F32)
    pa[0] = pb[:300] = (100, 100, 100)
    pb[300] = pa[1:301] = (200, 200, 200)
    pa[301] = pb[301] = (300, 300, 300)
    xa = np.stack([pa.T, pa[::-1].T]).astype(F32)
    xb = np.stack([pb.T, pb[::-1].T]).astype(F32)
    pad_a, pad_b = np.zeros((2, M), bool), np.zeros((2, N), bool)
    pad_a[1, -5:] = pad_b[1, -5:] = True
    xa[1, :, -5:] = xb[1, :, -5:] = 300.0
    return dict(xa=np.ascontiguousarray(xa), xb=np.ascontiguousarray(xb), pad_a=pad_a, pad_b=pad_b, eps=EPS)


OVERFLOW_N = 46341   # 46341^2 = 2 147 488 281 > 2^31 - 1 = 2 147 483 647 > 46340 x 46341 = 2 147 441 940
