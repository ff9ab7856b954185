"""The cases of tests/test_gpu_knn_paths.py: small inputs (N <= 8192, S <= 8192) built so that, judged by the reference's arithmetic
alone (tests/knn_paths_restated.py), rows take each exit of the hybrid neighbour search (csrc/knn.hip).  CPU torch / numpy only,
no library code.  tests/test_knn_paths_host.py proves per case that the exits it is named for are reached.

A case is a dict:
  name, pts (B, N, 3) float32, lens (B,), ctr (B, S, 3), K, r
  path     "grid" (N >= 1024) or "brute";  regime  "heap" (64 K <= N: torch.topk's partial_sort) or "nth" (nth_element)
  need     exit / property name (a key of knn_paths_restated.counts) -> the least number of rows, summed over the frames,
           that must take it
  ties     the least number of rows with a boundary tie inside the radius (tie_rows)
  header   (g, H, h) of frame 0, or None where the case is not about the layout
  fallback True for the one case that pins the documented deviation (tie queue full in the nth_element regime)
  by_mark  True where the rows left to the full search must outnumber the todo list (B N entries)
  fp64     the coordinates stay within the unit cube / ball (|p|^2 <= 3): the fp64 band check applies
Minimums are round numbers below what the restatement counts for these seeds (the counts are printed by the host test)."""
import functools

import numpy as np
import torch

F = np.float32


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def lattice(n, steps, seed):
    """n points with coordinates randint(0, steps) / steps: many duplicates, every distance tied many times over"""
    return (torch.randint(0, steps, (n, 3), generator=_gen(seed)).float() / float(steps)).numpy()


def square(n, seed, side=1.0, zmax=0.02, centre=(0.0, 0.0, 0.0)):
    """n points uniform in a square of the given side around `centre`, |z| <= zmax: distinct points, ties improbable"""
    u = torch.rand(n, 3, generator=_gen(seed)).numpy().astype(F)
    p = (u - F(0.5)) * np.array([side, side, 2 * zmax], F)
    return (p + np.array(centre, F)).astype(F)


def pick(points, s, seed, replace=False):
    """s centres drawn from the points"""
    g = _gen(seed)
    n = len(points)
    sel = torch.randint(0, n, (s,), generator=g) if replace else torch.randperm(n, generator=g)[:s]
    return points[sel.numpy()]


def _case(name, pts, ctr, K, r, lens=None, **kw):
    pts, ctr = np.ascontiguousarray(pts, F), np.ascontiguousarray(ctr, F)
    if pts.ndim == 2:
        pts, ctr = pts[None], ctr[None]
    B, N, _ = pts.shape
    lens = [N] * B if lens is None else list(lens)
    c = dict(name=name, pts=pts, ctr=ctr, K=K, r=float(r), lens=lens, path="grid" if N >= 1024 else "brute",
             regime="heap" if 64 * K <= N else "nth", need={}, ties=0, header=None, fallback=False, by_mark=False, fp64=False)
    c.update(kw)
    pts.setflags(write=False), ctr.setflags(write=False)
    return c


def _layout(name, n, r, seed, header, need, ties=0, K=32, lifted_z=5.0):
    """uniform square, 500 centres of the frame + 20 outside the bounding box + 20 lifted in z"""
    p = square(n, seed)
    inside = pick(p, 500, seed + 1)
    out = square(20, seed + 2)
    out[:10, 0] = F(-0.5) - F(0.003) - np.abs(out[:10, 0]) * F(0.3)      # left of the box, some within the radius of it
    out[10:, 1] = F(0.5) + F(2.0) + out[10:, 1]                          # far above it
    up = pick(p, 20, seed + 3).copy()
    up[:, 2] += F(lifted_z)
    return _case(name, p, np.concatenate([inside, out, up]), K, r, header=header, need=need, ties=ties, fp64=True)


def _ragged(name, n, K, seed, ties):
    """frames of n, K + 1, K, K - 1 and 1 valid points, 17 centres each (the frame's own points, cyclically); r = 2 holds every
    valid point.  The frames of K + 1 and K points are on a lattice (the two farthest of K + 1 are often equally far: a tie
    exactly where finish() starts replaying, len >= K); the shorter ones are distinct points, as the slots the reference fills
    with its nearest pick would otherwise hang on which of two coincident points it picked"""
    lens = [n, K + 1, K, max(K - 1, 1), 1]
    pts = np.zeros((5, n, 3), F)
    pts[0] = lattice(n, 12, seed)
    pts[1, :K + 1] = lattice(K + 1, 3, seed + 1)
    pts[2, :K] = lattice(K, 3, seed + 2)
    pts[3, :lens[3]] = square(lens[3], seed + 3, zmax=0.5)
    pts[4, :1] = square(1, seed + 4, zmax=0.5)
    pts[1, K + 1:], pts[3, lens[3]:] = F(0.25), F(-0.125)     # padding the searches must not read as points
    ctr = np.stack([pts[b, np.arange(17) % lens[b]] for b in range(5)])
    return _case(name, pts, ctr, K, 2.0, lens=lens, ties=ties)


BUILDERS = {}


def builder(fn):
    BUILDERS[fn.__name__] = fn
    return fn


# ---- tie replays ------------------------------------------------------------------------------------------------------------
@builder
def grid_nth():          # knn_tie_nth_kernel: grid path, 64 K > N
    p = lattice(1536, 12, 101)
    return _case("grid_nth", p, pick(p, 300, 102), 32, 0.3, ties=150, need={"inner": 150, "overflow": 80, "widened": 15}, fp64=True)


@builder
def grid_heap_low_k16():  # knn_tie_kernel at the low edge of the heap regime
    p = lattice(1100, 12, 103)
    return _case("grid_heap_low_k16", p, pick(p, 300, 104), 16, 0.3, ties=150, need={"inner": 250, "border_fail": 20}, fp64=True)


@builder
def grid_heap_k64():      # K = KMAX, 64 K == N exactly
    p = lattice(4096, 24, 105)
    return _case("grid_heap_k64", p, pick(p, 300, 106), 64, 0.3, ties=150, need={"overflow": 250}, fp64=True)


@builder
def tieq_overflow_heap():  # more than TIE_CAP tied rows, heap regime: the rest is replayed in place by knn_grid_kernel
    p = lattice(8192, 24, 107)
    return _case("tieq_overflow_heap", p, p.copy(), 32, 0.25, ties=5500, fp64=True)


@builder
def tieq_overflow_nth():   # the same in the nth_element regime: the documented fallback (smallest indices)
    p = lattice(1536, 12, 101)
    return _case("tieq_overflow_nth", p, pick(p, 8000, 108, replace=True), 32, 0.3, ties=5000, fallback=True, fp64=True)


@builder
def brute_nth_600():       # nth_select_exact in dynamic LDS, brute path
    p = lattice(600, 10, 109)
    return _case("brute_nth_600", p, pick(p, 200, 110), 32, 0.35, ties=100, fp64=True)


@builder
def brute_nth_256():
    p = lattice(256, 8, 111)
    return _case("brute_nth_256", p, pick(p, 64, 112), 16, 0.4, ties=40, fp64=True)


# ---- the todo list ----------------------------------------------------------------------------------------------------------
@builder
def by_mark():             # S > N: more rows fail the fast kernel than the todo list (B N entries) holds
    p = square(1024, 113)
    up = pick(p, 1200, 114, replace=True).copy()
    up[:, 2] += F(5.0)
    ctr = np.concatenate([up, pick(p, 1300, 115, replace=True)])
    ctr = ctr[torch.randperm(2500, generator=_gen(116)).numpy()]
    return _case("by_mark", p, ctr, 16, 0.1, need={"empty": 1200}, by_mark=True, fp64=True)


# ---- layouts and fast exits -------------------------------------------------------------------------------------------------
@builder
def layout_h1():
    return _layout("layout_h1", 4096, 0.05, 120, (None, 1, 1), {"outside": 20, "empty": 20, "full": 450, "slots5": 100, "slots10": 300})


@builder
def layout_h3():           # centres lifted by 0.08 stay within the radius of a few points: the border test must fail for them
    c = _layout("layout_h3", 4096, 0.1, 130, (None, 3, 2), {"outside": 20, "inner": 500, "border_pass": 450, "border_fail": 8, "slots15": 300},
                lifted_z=0.08)
    return c


@builder
def layout_h2_dense():     # the 3x3 inner block of the H = 2 layout overflows the registers almost everywhere
    return _layout("layout_h2_dense", 4096, 0.25, 140, (None, 2, 1), {"outside": 20, "overflow": 450})


@builder
def layout_h2():           # ... and at half the density it does not: inner blocks, and 5x5 blocks at the corners of the frame
    p = square(2048, 150)
    corners = p[np.argsort(-(np.abs(p[:, 0]) + np.abs(p[:, 1])))[:120]]
    c = _layout("layout_h2", 2048, 0.25, 150, (None, 2, 1), {"outside": 20, "empty": 20, "inner": 500, "border_pass": 500,
                                                                "widened": 40, "slots20": 300})
    ctr = np.concatenate([c["ctr"][0], corners])
    return _case("layout_h2", p, ctr, 32, 0.25, header=c["header"], need=c["need"], fp64=True)


@builder
def cluster_overflow():    # 3000 points within sigma = 0.01: far above QCAP in one block, and above CAP in the full search
    g = _gen(160)
    cl = (torch.randn(3000, 3, generator=g) * 0.01).numpy().astype(F)
    p = np.concatenate([cl, square(1096, 161)])
    p = p[torch.randperm(4096, generator=g).numpy()]
    ctr = np.concatenate([pick(cl, 300, 162), pick(square(1096, 161), 200, 163)])
    return _case("cluster_overflow", p, ctr, 32, 0.2, need={"overflow": 300, "widened": 100}, fp64=True)


@builder
def gdim_floor():          # an elongated frame: the grid-size floor ext / 127 is the cell edge, far above the radius
    u = torch.rand(2048, 3, generator=_gen(170)).numpy().astype(F)
    p = u * np.array([100.0, 1.0, 0.04], F)
    return _case("gdim_floor", p, pick(p, 300, 171), 8, 0.3, header=(128, 1, 1), need={"full": 300, "slots5": 300})


# ---- row shapes -------------------------------------------------------------------------------------------------------------
@builder
def one_centre():          # S = 1
    p = square(2048, 180)
    return _case("one_centre", p, p[777:778], 32, 0.1, need={"full": 1}, fp64=True)


@builder
def s17_k64():             # S no multiple of 16: the fast kernel's last quarter waves are clamped to row S - 1
    p = lattice(4096, 24, 181)
    return _case("s17_k64", p, pick(p, 17, 182), 64, 0.3, ties=10, fp64=True)


@builder
def s17_k1():              # K = 1 on a lattice with coincident points: nearly every row is tied at distance zero
    p = lattice(1100, 12, 183)
    return _case("s17_k1", p, pick(p, 17, 184), 1, 0.3, ties=8, fp64=True)


@builder
def ragged_grid_heap():
    return _ragged("ragged_grid_heap", 1024, 16, 190, 15)


@builder
def ragged_grid_nth():
    return _ragged("ragged_grid_nth", 1024, 32, 191, 20)


@builder
def ragged_brute_heap():
    return _ragged("ragged_brute_heap", 512, 8, 192, 8)


@builder
def ragged_brute_nth():
    return _ragged("ragged_brute_nth", 512, 16, 193, 15)


@builder
def shifted_far():         # 71 units from the origin err2 = 0.1 exceeds rho^2: every border test must fail on err2 alone
    p = square(1024, 200, centre=(-65.4, -29.1, 0.0))
    return _case("shifted_far", p, pick(p, 300, 201), 32, 0.1, need={"border_fail": 200}, ties=50)


@builder
def shifted_near():        # 6.4 units from the origin err2 = 8e-4 is a tenth of rho^2: it decides some rows and not others
    p = square(4096, 202, centre=(5.0, -4.0, 0.3))
    return _case("shifted_near", p, pick(p, 300, 203), 32, 0.1, need={"border_pass": 250})


NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """everything the tests compare against, computed once per process from the oracle and the restatement:
      want, dk   (B, S, K) the oracle's rows and their distances (oracle.dpm_oracle.hybrid_query)
      spec       (B, S, K) the rows the search is specified to return, as sorted multisets: the oracle's members within the
                 radius, and in the K - members slots the reference fills with ITS nearest pick, the search's nearest pick
                 `first`.  The two picks are the same point wherever the row's minimum distance is attained once
      first      (B, S) smallest index among the points at the row's minimum distance;  min_tied (B, S) it is attained twice or
                 more;  dmin (B, S) that distance
      filler_differs  number of rows whose spec differs from the oracle's row (a tied minimum and fewer than K within the radius)
      tie        (B, S) tie_rows;  headers, cls, counts (summed over the frames): grid cases only"""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import knn_paths_restated as R
    from oracle import dpm_oracle as O
    c = case(name)
    B, N, _ = c["pts"].shape
    S, K = c["ctr"].shape[1], c["K"]
    r2 = F(c["r"] * c["r"])
    pad = torch.arange(N)[None, :] >= torch.tensor(c["lens"])[:, None]
    # (whole row groups of centres: see knn_paths_restated.pad_rows)
    want, dk = O.hybrid_query(c["r"], K, torch.from_numpy(c["pts"].copy()), torch.from_numpy(R.pad_rows(c["ctr"])), pad, return_dist=True)
    want, dk = want.numpy()[:, :S], dk.numpy()[:, :S]
    first, min_tied, dmin = np.zeros((B, S), np.int64), np.zeros((B, S), bool), np.zeros((B, S), F)
    tie = np.zeros((B, S), bool)
    headers, cls, total = [], [], {}
    for b in range(B):
        L = c["lens"][b]
        for s0 in range(0, S, R.CHUNK):
            d = R.expanded(c["ctr"][b, s0:s0 + R.CHUNK], c["pts"][b, :L])
            mn = d.min(1)
            at_min = d == mn[:, None]
            first[b, s0:s0 + R.CHUNK], min_tied[b, s0:s0 + R.CHUNK], dmin[b, s0:s0 + R.CHUNK] = at_min.argmax(1), at_min.sum(1) > 1, mn
            tie[b, s0:s0 + R.CHUNK] = R.tie_rows(None, L, None, K, r2, d=d)    # (the same distance matrix)
            if L >= K:   # the oracle's own call, in chunks of another size, saw the same distances
                assert (np.partition(d, K - 1, axis=1)[:, K - 1] == dk[b, s0:s0 + R.CHUNK, K - 1]).all(), (name, b)
        if c["path"] == "grid":
            hd = R.grid_header(c["pts"][b], L, c["r"])
            cl = R.classify(c["pts"][b], L, c["ctr"][b], hd, K, r2)
            headers.append(hd), cls.append(cl)
            for k, v in R.counts(cl).items():
                total[k] = total.get(k, 0) + v
    member = dk <= r2
    spec = np.sort(np.where(member, want, first[:, :, None]), axis=2)
    differs = int((spec != np.sort(want, axis=2)).any(2).sum())
    return dict(want=want, dk=dk, spec=spec, first=first, min_tied=min_tied, dmin=dmin, filler_differs=differs, tie=tie,
                headers=headers, cls=cls, counts=total)
