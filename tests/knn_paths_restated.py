"""The path choices of the hybrid neighbour search (csrc/knn.hip) restated in plain numpy: which grid a frame gets and which exit
of knn_grid_fast_kernel a centre must take.  Nothing of the code under test is used; distances are the reference's float32
expanded form (oracle.dpm_oracle.expanded_sqdist), the form the kernels are specified to reproduce bit for bit.

  grid_header(points, length, radius)   knn_grid_build_kernel's header: lox, loy, inv_cs, g, err2, H, h (float32 arithmetic in
                                        the kernel's order) plus the quantities the layout choice hangs on, for margins
  classify(points, length, centers, header, K, r2)
                                        per centre the exit of the fast kernel, decided in the kernel's order
  tie_rows(points, length, centers, K, r2)
                                        rows whose K-th and (K+1)-th distances are bit-equal and within the radius
  counts(cls)                           exit name -> number of rows

Exits, in the order the kernel decides them (a row takes the first that applies):
  outside   the centre's cell is not in the grid: left to the full search
  overflow  the block holds more than QCAP = 320 points: left to the full search
  empty     no point of the block has a computed distance <= r^2: left to the full search
  full      the block is the covering (2H+1)^2 one (H = h, or H = 2 and the 5x5 block was small enough: `widened`); the answer
            needs no border test
  inner     the block is the inner (2h+1)^2 one; `border` says what the test (bound + err2) * 1.004 < rho^2 must answer
A full or inner row whose K-th and (K+1)-th distances INSIDE ITS BLOCK are bit-equal goes to the tie queue before any border
test (`block_tie`).

The border test's bound is the fast kernel's separator: some float above the block's K-th distance and at most its (K+1)-th
(which one depends on the probe sequence).  `border` is therefore "pass" when the test holds even for the (K+1)-th distance,
"fail" when it fails even for the K-th, and "either" in between; with at most K points of the block inside the radius the
bound is r^2 and the answer is definite.  Both definite answers keep a relative 1e-5 away from the threshold (the header's
float rounding)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import dpm_oracle as O  # noqa: E402

F = np.float32
GDIM, GRID_MIN_N, QCAP, QL, QB, KMAX, TIE_CAP = 128, 1024, 320, 16, 5, 64, 4096
GRID_RHO_POINTS, GRID_PI = F(128.0), F(3.14159265)
EXITS = ("outside", "overflow", "empty", "full", "inner")
CHUNK = 1024  # centres per block of the (S, N) distance matrix


def _sq3(p):
    return (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]


def grid_header(points, length, radius):
    """points (N, 3) float32, the frame's first `length` are valid -> dict.  Every operation is a float32 one, in the order of
    knn_grid_build_kernel (min / max reductions are exact in any order)."""
    p = np.ascontiguousarray(points, dtype=F)[:length]
    assert length > 0
    lox, hix, loy, hiy = p[:, 0].min(), p[:, 0].max(), p[:, 1].min(), p[:, 1].max()
    m2 = _sq3(p).max()
    ext = max(max(hix - lox, hiy - loy), F(1e-6))
    r2 = F(float(radius) * float(radius))
    err2 = F(2e-5) * max(F(1.0), m2)
    cs_min = max(F(np.sqrt(float(radius) * float(radius) + 2e-5) * 1.002), np.sqrt(r2 + err2) * F(1.002))
    floor_cs = ext / F(GDIM - 1)
    cover = max(cs_min, floor_cs)
    area = max(hix - lox, F(1e-6)) * max(hiy - loy, F(1e-6))
    rho_t = np.sqrt(GRID_RHO_POINTS * (area * (GRID_PI / F(4.0))) / (GRID_PI * F(length)))
    cs2 = max(max(rho_t, cover * F(0.5005)), floor_cs)
    cs3 = max(max(rho_t * F(0.5), cover * F(0.3337)), floor_cs)
    cs, H, h = cover, 1, 1
    best = F(9.0) * cover * cover
    compared = []   # (lhs, rhs) of every "<" the layout choice evaluates

    def less(a, b):
        compared.append((float(a), float(b)))
        return a < b
    if less(cs2, cover) and less(F(9.0) * cs2 * cs2, best):
        best, cs, H, h = F(9.0) * cs2 * cs2, cs2, 2, 1
    if less(cs3, cover * F(0.5)) and less(F(25.0) * cs3 * cs3, best):
        best, cs, H, h = F(25.0) * cs3 * cs3, cs3, 3, 2
    inv_cs = F(1.0) / cs
    cells = ext * inv_cs
    g = min(GDIM, int(cells) + 1)
    return dict(lox=lox, loy=loy, inv_cs=inv_cs, g=g, err2=err2, H=H, h=h,
                # what the choices above hang on (tests keep them away from their thresholds)
                cover=cover, rho_t=rho_t, cs=cs, cs2=cs2, cs3=cs3, floor_cs=floor_cs, cells=cells, ext=ext, compared=compared)


def header_margin(hd):
    """-> (the smallest relative gap |lhs - rhs| / rhs of the comparisons that chose the layout; the distance of ext / cs from
    an integer, on which g = int(ext / cs) + 1 hangs, None where the GDIM cap or the grid-size floor decides g).  Where the floor
    ext / 127 is the edge, ext / cs is 127 up to rounding and g is 127 or 128 by the last bit of three IEEE operations: both
    sides evaluate the same correctly rounded operations, so that case is compared exactly and has no margin to keep."""
    on_floor = float(hd["cs"]) == float(hd["floor_cs"])
    # (on the floor cs2 and cs3 ARE the covering edge, the same float: those comparisons are false by identity, not by rounding)
    rel = min([abs(a - b) / b for a, b in hd["compared"] if not (on_floor and a == b)], default=1.0)
    cells = float(hd["cells"])
    frac = None if on_floor or cells >= GDIM + 1 else min(cells - np.floor(cells), np.ceil(cells) - cells)
    return rel, frac


def point_cells(points, length, hd):
    """cell (column, row) of every valid point: clamp(floor((x - lox) * inv_cs), 0, g - 1)"""
    p = np.ascontiguousarray(points, dtype=F)[:length]
    cx = np.clip(np.floor((p[:, 0] - hd["lox"]) * hd["inv_cs"]), 0, hd["g"] - 1).astype(np.int64)
    cy = np.clip(np.floor((p[:, 1] - hd["loy"]) * hd["inv_cs"]), 0, hd["g"] - 1).astype(np.int64)
    return cx, cy


ROW_MULTIPLE = 64


def pad_rows(centers):
    """(..., S, 3) -> the same with the last centre repeated up to a multiple of ROW_MULTIPLE rows.  The oracle's distance is a
    torch.matmul, and the host BLAS behind it rounds a REMAINDER row of the centre matrix differently from the rest on some
    hosts (seen: the single row of S = 1 on one, row 16 of S = 17 on another: not an fma chain, and bit-equal ties fall
    elsewhere).  The kernels are specified as the main path -- dot = fma(az, bz, fma(ay, by, ax * bx)), csrc/knn.hip -- so the
    oracle is always called with whole row groups; chain_sqdist below is that path written out, and the host test holds the
    oracle to it.  The same holds for a remainder COLUMN, a frame of 9 points, so `expanded` pads the points too."""
    c = np.array(centers, dtype=F)
    extra = -c.shape[-2] % ROW_MULTIPLE
    return c if extra == 0 else np.concatenate([c, np.repeat(c[..., -1:, :], extra, axis=-2)], axis=-2)


def expanded(centers, points):
    """(S, 3), (N, 3) float32 -> (S, N) float32 numpy: the reference's expanded-form squared distances"""
    c, p = torch.from_numpy(pad_rows(centers)), torch.from_numpy(pad_rows(points))   # (copies: the cases are read-only)
    return O.expanded_sqdist(c[None], p[None])[0].numpy()[:len(centers), :len(points)]


def _fma32(a, b, c):
    """correctly rounded float32 fma of float32 arrays: the product is exact in float64, the sum is rounded to odd there (TwoSum
    tells whether it was exact), and 53 >= 2 * 24 + 2 bits make the final rounding to float32 the single rounding of an fma"""
    p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    odd = (s.view(np.int64) & 1) == 1
    fix = (err != 0) & ~odd & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F)


def chain_sqdist(centers, points):
    """the same distances with the K = 3 product written as the fma chain the kernels run: ((-2 dot) + |a|^2) + |b|^2"""
    a, b = np.array(centers, dtype=F), np.array(points, dtype=F)
    ax, ay, az = (a[:, None, k] for k in range(3))
    bx, by, bz = (b[None, :, k] for k in range(3))
    dot = _fma32(az, bz, _fma32(ay, by, ax * bx))
    return ((F(-2.0) * dot) + _sq3(a)[:, None]) + _sq3(b)[None, :]


def _kth_pair(d, K):
    """(S, M) with +inf for absent entries -> the K-th and (K+1)-th smallest per row (+inf where there are not that many)"""
    S, M = d.shape
    if M < K + 1:
        d = np.concatenate([d, np.full((S, K + 1 - M), np.inf, F)], 1)
    part = np.partition(d, (K - 1, K), axis=1)
    return part[:, K - 1], part[:, K]


def classify(points, length, centers, hd, K, r2):
    """-> dict of (S,) arrays: exit (index into EXITS), widened, block_tie, border (0 none, 1 pass, 2 fail, 3 either), tot (points
    in the block searched), slots (5 / 10 / 15 / 20: the slot group of a row the registers hold, 0 otherwise)"""
    p = np.ascontiguousarray(points, dtype=F)[:length]
    c = np.ascontiguousarray(centers, dtype=F)
    r2 = F(r2)
    S, g, H, h = len(c), hd["g"], hd["H"], hd["h"]
    pcx, pcy = point_cells(points, length, hd)
    fx, fy = (c[:, 0] - hd["lox"]) * hd["inv_cs"], (c[:, 1] - hd["loy"]) * hd["inv_cs"]
    flx, fly = np.floor(fx), np.floor(fy)
    with np.errstate(invalid="ignore"):
        inside = (flx >= 0) & (flx < g) & (fly >= 0) & (fly < g)
    cx, cy = np.where(inside, flx, 0).astype(np.int64), np.where(inside, fly, 0).astype(np.int64)
    out = dict(exit=np.zeros(S, np.int64), widened=np.zeros(S, bool), block_tie=np.zeros(S, bool), border=np.zeros(S, np.int64),
               tot=np.zeros(S, np.int64), slots=np.zeros(S, np.int64))
    full_cells, inner_cells = (2 * H + 1) ** 2, (2 * h + 1) ** 2
    for s0 in range(0, S, CHUNK):
        sl = slice(s0, min(s0 + CHUNK, S))
        dx, dy = np.abs(pcx[None, :] - cx[sl, None]), np.abs(pcy[None, :] - cy[sl, None])
        in_inner = (dx <= h) & (dy <= h)
        tot = in_inner.sum(1)
        block = in_inner
        inner = np.full(len(tot), H > h)
        widened = np.zeros(len(tot), bool)
        if H > h and 2 * H + 1 <= 5:
            in_full = (dx <= H) & (dy <= H)
            ftot = in_full.sum(1)
            widened = (tot * full_cells <= QCAP * inner_cells) & (ftot <= QCAP)
            block = np.where(widened[:, None], in_full, in_inner)
            tot = np.where(widened, ftot, tot)
            inner &= ~widened
        d = np.where(block, expanded(c[sl], p), F(np.inf))
        d = np.where(d <= r2, d, F(np.inf))
        cnt = np.isfinite(d).sum(1)
        kth, kth1 = _kth_pair(d, K)
        sel = cnt > K
        tie = sel & (kth == kth1)
        # the border test in float32, as the kernel writes it
        u, v = (fx - flx)[sl], (fy - fly)[sl]
        with np.errstate(invalid="ignore"):
            m = F(h) + np.minimum(np.minimum(u, F(1.0) - u), np.minimum(v, F(1.0) - v)) - F(1e-3)
        rho2 = ((m / hd["inv_cs"]) * (m / hd["inv_cs"])).astype(np.float64)
        lhs = lambda bound: ((bound + hd["err2"]) * F(1.004)).astype(np.float64)  # noqa: E731
        with np.errstate(invalid="ignore", over="ignore"):
            lo, hi = lhs(np.where(sel, kth, r2).astype(F)), lhs(np.where(sel, kth1, r2).astype(F))
            sure_pass, sure_fail = hi * (1 + 1e-5) < rho2, ~(lo * (1 - 1e-5) < rho2)
        border = np.where(sure_pass, 1, np.where(sure_fail, 2, 3))
        ex = np.where(~inside[sl], 0, np.where(tot > QCAP, 1, np.where(cnt == 0, 2, np.where(inner, 4, 3))))
        held = ex >= 3
        out["exit"][sl] = ex
        out["widened"][sl] = widened & held
        out["block_tie"][sl] = tie & held
        out["border"][sl] = np.where((ex == 4) & ~tie, border, 0)
        out["tot"][sl] = np.where(inside[sl], tot, 0)
        groups = -(-np.maximum(tot, 1) // QL)
        out["slots"][sl] = np.where(held, -(-groups // QB) * QB, 0)
    return out


def counts(cls):
    """exit name -> rows; plus widened, block_tie, border_pass / border_fail / border_either and todo_min: the rows the
    restatement is sure the fast kernel leaves to the full search"""
    n = {name: int((cls["exit"] == k).sum()) for k, name in enumerate(EXITS)}
    n["widened"], n["block_tie"] = int(cls["widened"].sum()), int(cls["block_tie"].sum())
    for k, name in ((1, "border_pass"), (2, "border_fail"), (3, "border_either")):
        n[name] = int((cls["border"] == k).sum())
    n["todo_min"] = n["outside"] + n["overflow"] + n["empty"] + n["border_fail"]
    for sg in (5, 10, 15, 20):
        n[f"slots{sg}"] = int((cls["slots"] == sg).sum())
    return n


def tie_rows(points, length, centers, K, r2, d=None):
    """(S,) bool: the K-th and (K+1)-th smallest expanded distances over the frame's valid points are bit-equal and <= r^2
    (d: the (S, length) distances where the caller has them already)"""
    if d is None:
        p = np.ascontiguousarray(points, dtype=F)[:length]
        c = np.ascontiguousarray(centers, dtype=F)
        return np.concatenate([tie_rows(None, length, None, K, r2, d=expanded(c[s0:s0 + CHUNK], p)) for s0 in range(0, len(c), CHUNK)])
    if length < K + 1:
        return np.zeros(len(d), bool)
    kth, kth1 = _kth_pair(d, K)
    return (kth == kth1) & (kth1 <= F(r2))
