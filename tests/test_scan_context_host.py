"""CPU: the numpy restatement of Scan Context (tests/scan_context_restated.py) against constructed answers, and the POWER of
the GPU search cases (tests/test_gpu_scan_context.py draws its inputs from `search_case` here).

The GPU search is compared with the float64 restatement wherever the restatement's own decision is clear: where the gap
between the best and second-best shift of a pair, or between consecutive ranks of a query up to K + 1, exceeds 2 * bound,
bound = max(3 |r32 - r64|, (rings + 8) * 2^-24).  A comparison that skipped most decisions would say nothing, so the share of
skipped decisions on the fixed seeds is asserted here, without a GPU, to be at most 1 %.
"""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_context_restated as S  # noqa: E402

RINGS, SECTORS, ROWS, QUERIES, MAX_K = 20, 60, 130, 3, 8
SEEDS = (11, 12)
DS = (1, 63, 64, 65, 130)      # the database sizes of the GPU search test: prefixes of the ROWS rows
FLOOR = (RINGS + 8) * 2.0 ** -24   # a cosine is a RINGS-term fp32 dot product of unit columns, plus their normalisation


def normalised(raw):
    """(n,rings,sectors) raw float32 -> normalised float32 (n,rings,sectors), masks (n,) python ints"""
    out = [S.finish(r, np.float32) for r in raw]
    return np.stack([o[0] for o in out]), [o[1] for o in out]


@functools.lru_cache(maxsize=None)
def search_case(seed):
    """the fixed inputs of the GPU search test and what both restatements say about them, computed once: ROWS random database
    rows (60 % occupancy, heights up to 20, five empty columns each) and QUERIES queries -- a fresh random one, a noisy copy
    of row 7 turned by 13 columns, and one with 20 empty columns"""
    rng = np.random.default_rng(seed)
    raw = S.random_descriptors(rng, ROWS, RINGS, SECTORS)
    q_raw = S.random_descriptors(rng, QUERIES, RINGS, SECTORS)
    turned = np.roll(raw[7], -13, axis=1) * (1 + 0.05 * rng.standard_normal((RINGS, SECTORS))).astype(np.float32)
    q_raw[1] = np.maximum(turned, 0).astype(np.float32)
    q_raw[2][:, rng.choice(SECTORS, size=20, replace=False)] = 0
    db, db_mask = normalised(raw)
    qn, q_mask = normalised(q_raw)
    d64 = np.zeros((QUERIES, ROWS, SECTORS))
    d32 = np.zeros((QUERIES, ROWS, SECTORS), np.float32)
    for q in range(QUERIES):
        for c in range(ROWS):
            d64[q, c] = S.pair_distances_fast(qn[q], q_mask[q], db[c], db_mask[c], np.float64)
            d32[q, c] = S.pair_distances_fast(qn[q], q_mask[q], db[c], db_mask[c], np.float32)
    spread = np.abs(d32.astype(np.float64) - d64).max(axis=2)          # (Q, ROWS): |r32 - r64| of a pair, over its shifts
    bound = np.maximum(3 * spread, FLOOR)
    order = np.sort(d64, axis=2)
    return SimpleNamespace(db=db, db_mask=db_mask, qn=qn, q_mask=q_mask, d64=d64, d32=d32, spread=spread, bound=bound,
                           best=d64.min(axis=2), shift=d64.argmin(axis=2), shift_gap=order[:, :, 1] - order[:, :, 0])


def ranking(case, q, limit, K):
    """the float64 restatement's first K + 1 rows of query q among rows < limit: [(d, row, shift, bound, gap to the next)]"""
    rows = sorted(range(limit), key=lambda c: (case.best[q, c], c))[:K + 1]
    out = []
    for k, c in enumerate(rows):
        nxt = case.best[q, rows[k + 1]] - case.best[q, c] if k + 1 < len(rows) else np.inf
        b = max(case.bound[q, c], case.bound[q, rows[k + 1]]) if k + 1 < len(rows) else case.bound[q, c]
        out.append((case.best[q, c], c, int(case.shift[q, c]), b, nxt))
    return out


def test_fast_distances_are_the_triple_loops():
    case = search_case(SEEDS[0])
    for q, c in ((0, 0), (1, 7), (2, 129)):
        slow = S.pair_distances(case.qn[q], case.q_mask[q], case.db[c], case.db_mask[c], np.float64)
        assert np.abs(slow - case.d64[q, c]).max() < 1e-12
        slow32 = S.pair_distances(case.qn[q], case.q_mask[q], case.db[c], case.db_mask[c], np.float32)
        assert slow32.dtype == np.float32 and np.abs(slow32.astype(np.float64) - slow).max() < FLOOR


def test_turned_descriptor_is_found_at_its_shift():
    rng = np.random.default_rng(3)
    A, masks = normalised(S.random_descriptors(rng, 1, 6, 12, empty_columns=2))
    for m in (0, 1, 5, 11):
        B, bm = S.roll_columns(A[0], masks[0], m)
        for dtype in (np.float32, np.float64):
            d = S.pair_distances(A[0], masks[0], B, bm, dtype)
            assert int(np.argmin(d)) == m and d[m] <= 6 * 2.0 ** -23, (m, d)
        dist, row, shift = S.search(A, masks, B[None], [bm], [1], 2)
        assert row[0].tolist() == [0, -1] and shift[0].tolist() == [m, -1] and np.isinf(dist[0, 1])


def test_exact_unit_columns_give_zero_at_the_shift_and_one_elsewhere():
    """one point per column in its own ring: every normalised column is a unit vector e_ring, so S(s) counts agreeing rings"""
    rings, sectors = 8, 8
    raw = np.zeros((rings, sectors), np.float32)
    raw[np.arange(sectors), np.arange(sectors)] = 3.0
    A, m = S.finish(raw)
    assert m == 0xFF and np.array_equal(A, np.eye(8, dtype=np.float32))
    B, bm = S.roll_columns(A, m, 3)
    d = S.pair_distances(A, m, B, bm, np.float32)
    assert d[3] == 0 and all(d[s] == 1 for s in range(8) if s != 3)


def test_empty_descriptor_gives_one():
    rng = np.random.default_rng(4)
    A, masks = normalised(S.random_descriptors(rng, 2, 5, 8, empty_columns=1))
    Z = np.zeros_like(A[0])
    assert np.all(S.pair_distances(Z, 0, A[0], masks[0], np.float32) == 1)
    assert np.all(S.pair_distances(A[0], masks[0], Z, 0, np.float64) == 1)
    dist, row, shift = S.search(Z[None], [0], A, masks, [2], 3)
    assert dist[0].tolist() == [1.0, 1.0, np.inf] and row[0].tolist() == [0, 1, -1] and shift[0].tolist() == [0, 0, -1]


def test_duplicate_rows_tie_to_the_smaller_row_and_limits_hide_rows():
    rng = np.random.default_rng(5)
    A, masks = normalised(S.random_descriptors(rng, 3, 5, 8, empty_columns=1))
    db, dm = np.stack([A[1], A[0], A[2], A[0]]), [masks[1], masks[0], masks[2], masks[0]]
    dist, row, shift = S.search(A[:1], masks[:1], db, dm, [4], 2)
    assert row[0].tolist() == [1, 3] and shift[0].tolist() == [0, 0] and dist[0, 0] == dist[0, 1]
    dist, row, shift = S.search(A[:1], masks[:1], db, dm, [1], 2)
    assert row[0].tolist() == [0, -1]
    dist, row, shift = S.search(A[:1], masks[:1], db, dm, [0], 2)
    assert row[0].tolist() == [-1, -1] and np.isinf(dist).all()


def test_build_restatement_on_hand_placed_points():
    """8 sectors of 45 degrees, 4 rings of 10 m: points on sector boundaries belong to the sector that STARTS there, points
    on ring edges to the ring that starts there, the gates are closed below and open above"""
    kw = dict(rings=4, sectors=8, max_range=40.0, min_range=1.0, z_offset=2.0)
    pts = [(1, 1, 0), (0, 1, 0), (-1, 1, 0), (-1, 0, 0), (1, 0, 0), (-1, -1, 0), (0, -1, 0), (1, -1, 0)]
    want = [1, 2, 3, 4, 0, 5, 6, 7]
    for p, sector in zip(pts, want):
        raw, norm, mask = S.build(np.array([p], np.float32), 1, **kw)
        assert mask == 1 << sector and raw[0, sector] == 2.0 and norm[0, sector] == 1.0, (p, sector, mask)
    for x, ring in ((10.0, 1), (20.0, 2), (30.0, 3), (9.999, 0), (1.0, 0)):
        raw, _, mask = S.build(np.array([(x, 0, 0)], np.float32), 1, **kw)
        assert mask == 1 and raw[ring, 0] == 2.0, (x, ring)
    for x in (40.0, 0.99, 0.0):
        assert S.build(np.array([(x, 0, 0)], np.float32), 1, **kw)[2] == 0
    for z in (-2.0, -3.0, np.nan, np.inf):     # h == 0, h < 0 and non-finite rows leave no trace
        assert S.build(np.array([(5, 5, z)], np.float32), 1, **kw)[2] == 0
    raw, _, _ = S.build(np.array([(5, 5, 1), (5.1, 5, 3), (5, 5.1, 2)], np.float32), 2, **kw)   # count hides the third row
    assert raw[0, 0] == 5.0 and raw[0, 1] == 3.0 and raw.sum() == 8.0


def test_power_of_the_gpu_search_cases():
    shifts = skipped_shifts = ranks = skipped_ranks = 0
    worst = 0.0
    for seed in SEEDS:
        case = search_case(seed)
        shifts += case.shift_gap.size
        skipped_shifts += int(np.count_nonzero(case.shift_gap <= 2 * case.bound))
        worst = max(worst, float(case.spread.max()))
        for q in range(QUERIES):
            for d, c, s, b, gap in ranking(case, q, ROWS, MAX_K)[:MAX_K]:
                ranks += 1
                skipped_ranks += int(gap <= 2 * b)
            for D in DS[:-1]:           # the smaller databases rank differently: their decisions must be clear too
                assert all(gap > 2 * b for d, c, s, b, gap in ranking(case, q, D, MAX_K)[:MAX_K]), (seed, q, D)
    print(f"shift decisions {shifts}, below 2 * bound {skipped_shifts}; rank decisions {ranks}, below {skipped_ranks}; "
          f"worst |r32 - r64| {worst:.2e}, floor {FLOOR:.2e}")
    assert shifts == len(SEEDS) * QUERIES * ROWS and ranks == len(SEEDS) * QUERIES * MAX_K
    assert skipped_shifts <= 0.01 * shifts and skipped_ranks <= 0.01 * ranks
    assert worst < FLOOR      # the floor, not the fp32 restatement's noise, is what sets the bound on these inputs
