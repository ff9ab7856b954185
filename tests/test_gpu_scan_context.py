"""GPU: Scan Context descriptors and their search (csrc/scan_context.hip) against the numpy restatement
(tests/scan_context_restated.py).

Build: raw heights, normalised heights and mask must equal the float32 restatement BYTE FOR BYTE -- the kernel has no
transcendental and no floating-point atomic, and every operation of it is restated.  Search: every distance within
max(3 |r32 - r64|, (rings + 8) * 2^-24) of the float64 restatement, rows and shifts equal to its wherever its own gaps exceed
2 * bound (tests/test_scan_context_host.py asserts, without a GPU, that at most 1 % of the decisions fall below that), turned
copies at their exact shift, and the same bytes on every run.  Every observed error goes to test_logs/scan_context_errors.log.
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_context_restated as S  # noqa: E402
import test_scan_context_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GEOMETRY = dict(max_range=40.0, min_range=1.0, z_offset=2.0)


def log(line):
    os.makedirs(os.path.join(ROOT, "test_logs"), exist_ok=True)
    with open(os.path.join(ROOT, "test_logs", "scan_context_errors.log"), "a") as f:
        f.write(line + "\n")
    print(line)


def gpu_build(xyz, count, rings, sectors, **kw):
    from deeppointmap_amd import ops
    kw = dict(GEOMETRY, **kw)
    x = torch.from_numpy(np.ascontiguousarray(xyz, np.float32)).to(DEV).reshape(-1, 3)
    raw, norm, mask = ops.scan_context_build(x, torch.tensor([count], device=DEV, dtype=torch.int32), rings, sectors, **kw)
    return raw[0].cpu().numpy(), norm[0].cpu().numpy(), int(mask[0].item())


def same_bytes(got, want, what):
    raw, norm, mask = got
    wraw, wnorm, wmask = want
    assert raw.tobytes() == wraw.tobytes(), (what, "raw", np.argwhere(raw != wraw)[:5])
    assert norm.tobytes() == wnorm.tobytes(), (what, "norm", np.abs(norm - wnorm).max())
    assert mask == S.mask_to_int64(wmask), (what, "mask", hex(mask), hex(wmask))


def cloud(rng, n, spread=45.0):
    """n points over a disc wider than max_range (both gates are crossed), heights on both sides of -z_offset"""
    p = np.empty((n, 3), np.float32)
    p[:, :2] = (rng.random((n, 2)) * 2 - 1) * spread
    p[:, 2] = rng.random(n) * 8 - 3
    return p


@pytest.mark.parametrize("rings,sectors", [(4, 8), (20, 60)])
@pytest.mark.parametrize("cap", [0, 1, 63, 64, 65, 257])
def test_build_is_the_restatement_byte_for_byte(rings, sectors, cap):
    rng = np.random.default_rng(100 + cap)
    xyz = cloud(rng, cap)
    same_bytes(gpu_build(xyz, cap, rings, sectors), S.build(xyz, cap, rings, sectors, **GEOMETRY), (rings, sectors, cap))


@pytest.mark.parametrize("rings,sectors", [(4, 8), (20, 60), (32, 64), (1, 4)])
def test_count_below_cap_hides_nan_rows(rings, sectors):
    rng = np.random.default_rng(7)
    xyz = cloud(rng, 257)
    xyz[200:] = np.nan
    got = gpu_build(xyz, 200, rings, sectors)
    same_bytes(got, S.build(xyz, 200, rings, sectors, **GEOMETRY), "count < cap")
    same_bytes(got, S.build(xyz[:200], 200, rings, sectors, **GEOMETRY), "the rows past count do not exist")
    assert got[2] != 0


def edge_points(rings, sectors):
    """points with r2 EXACTLY on every squared ring edge (both gates among them), on every sector boundary direction the
    tables hold, and the 8-sector lattice directions; heights at and below zero; non-finite rows"""
    e2, cs = S.tables(rings, sectors, GEOMETRY["max_range"])
    pts = []
    for m, e in enumerate(e2):
        r = np.float32(np.sqrt(np.float64(e)))
        for v in (r, np.nextafter(r, np.float32(0)), np.nextafter(r, np.float32(1e9))):
            pts += [(v, 0, 1 + m), (0, v, 1.5 + m), (0, -v, 2 + m), (-v, 0, 2.5 + m)]
    for v in (np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(0)), np.nextafter(np.float32(1.0), np.float32(2))):
        pts += [(v, 0, 0.25), (0, -v, 0.5)]
    for c, s in cs:                                          # on the boundary as the table states it, and its negative
        for rad in (3.0, 17.0):
            pts += [(rad * c, rad * s, 1.0), (-rad * c, -rad * s, 1.25), (rad * c, rad * s * (1 + 1e-6), 1.5), (rad * c, rad * s * (1 - 1e-6), 1.75)]
    for x, y in ((1, 1), (0, 1), (-1, 1), (-1, 0), (1, 0), (-1, -1), (0, -1), (1, -1)):
        pts += [(2 * x, 2 * y, 0.5), (7 * x, 7 * y, 3.0)]
    pts += [(5, 5, -2.0), (5, 6, -2.5), (6, 5, -1.9999999), (0, 0, 5.0), (-0.0, 0.0, 5.0)]            # h == 0, h < 0, r2 == 0
    pts += [(np.nan, 1, 1), (1, np.inf, 1), (1, 1, -np.inf), (3e30, 3e30, 1), (1e-30, 1e-30, 1)]
    return np.array(pts, np.float32)


@pytest.mark.parametrize("rings,sectors", [(4, 8), (20, 60)])
def test_points_on_ring_edges_and_sector_boundaries(rings, sectors):
    xyz = edge_points(rings, sectors)
    want = S.build(xyz, len(xyz), rings, sectors, **GEOMETRY)
    same_bytes(gpu_build(xyz, len(xyz), rings, sectors), want, "edges")
    for k, p in enumerate(xyz):                              # and one at a time: which cell each point chose
        same_bytes(gpu_build(p[None], 1, rings, sectors), S.build(p[None], 1, rings, sectors, **GEOMETRY), ("edge point", k, p))


def test_lattice_directions_choose_the_stated_sectors():
    for p, sector in zip([(1, 1), (0, 1), (-1, 1), (-1, 0), (1, 0), (-1, -1), (0, -1), (1, -1)], [1, 2, 3, 4, 0, 5, 6, 7]):
        raw, norm, mask = gpu_build(np.array([[3 * p[0], 3 * p[1], 1.0]], np.float32), 1, 4, 8)
        assert mask == 1 << sector and raw[0, sector] == 3.0 and norm[0, sector] == 1.0, (p, sector, hex(mask))
    for x, ring in ((10.0, 1), (20.0, 2), (30.0, 3), (1.0, 0)):
        assert gpu_build(np.array([[x, 0, 0]], np.float32), 1, 4, 8)[0][ring, 0] == 2.0
    for x in (40.0, 0.99):
        assert gpu_build(np.array([[x, 0, 0]], np.float32), 1, 4, 8)[2] == 0


def test_permuted_rows_and_repeated_runs_give_the_same_bytes():
    rng = np.random.default_rng(9)
    xyz = cloud(rng, 4000, spread=30.0)
    first = gpu_build(xyz, len(xyz), 20, 60)
    same_bytes(first, S.build(xyz, len(xyz), 20, 60, **GEOMETRY), "4000 points")
    again = gpu_build(xyz, len(xyz), 20, 60)
    perm = gpu_build(xyz[rng.permutation(len(xyz))], len(xyz), 20, 60)
    for other in (again, perm):
        assert other[0].tobytes() == first[0].tobytes() and other[1].tobytes() == first[1].tobytes() and other[2] == first[2]


def test_batched_build_equals_the_single_one_frame_by_frame():
    from deeppointmap_amd import ops
    rng = np.random.default_rng(10)
    F, N = 5, 300
    pts = np.stack([cloud(rng, N) for _ in range(F)])
    lengths = [300, 0, 1, 257, 64]
    pts[3, 257:] = np.nan
    pcd = torch.from_numpy(np.ascontiguousarray(pts.transpose(0, 2, 1))).to(DEV)
    raw, norm, mask = ops.scan_context_build_batched(pcd, torch.tensor(lengths, device=DEV, dtype=torch.int32), 20, 60, **GEOMETRY)
    for f in range(F):
        single = gpu_build(pts[f], lengths[f], 20, 60)
        assert raw[f].cpu().numpy().tobytes() == single[0].tobytes() and norm[f].cpu().numpy().tobytes() == single[1].tobytes()
        assert int(mask[f].item()) == single[2]
    assert int(mask[1].item()) == 0 and not raw[1].any()


def test_build_writes_into_a_database_row_and_replays_in_a_graph():
    from deeppointmap_amd import ops
    rng = np.random.default_rng(12)
    a, b = cloud(rng, 500), cloud(rng, 500)
    raw = torch.full((3, 20, 60), 7.0, device=DEV)
    norm = torch.full((3, 20, 60), 7.0, device=DEV)
    mask = torch.full((3,), 7, device=DEV, dtype=torch.int64)
    xyz = torch.from_numpy(a).to(DEV)
    count = torch.tensor([500], device=DEV, dtype=torch.int32)
    out = (raw[1:2], norm[1:2], mask[1:2])
    tables = ops.scan_context_tables(20, 60, GEOMETRY["max_range"])
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.scan_context_build(xyz, count, 20, 60, tables=tables, out=out, **GEOMETRY)      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.scan_context_build(xyz, count, 20, 60, tables=tables, out=out, **GEOMETRY)
    same_bytes((raw[1].cpu().numpy(), norm[1].cpu().numpy(), int(mask[1].item())), S.build(a, 500, 20, 60, **GEOMETRY), "row 1")
    assert bool((raw[0] == 7).all()) and bool((raw[2] == 7).all()) and mask.tolist()[::2] == [7, 7]
    xyz.copy_(torch.from_numpy(b))
    count.fill_(400)
    graph.replay()
    torch.cuda.synchronize()
    same_bytes((raw[1].cpu().numpy(), norm[1].cpu().numpy(), int(mask[1].item())), S.build(b, 400, 20, 60, **GEOMETRY), "replay")


def test_build_refuses_what_the_header_says():
    from deeppointmap_amd import ops
    xyz = torch.zeros(4, 3, device=DEV)
    count = torch.tensor([4], device=DEV, dtype=torch.int32)
    tables = ops.scan_context_tables(4, 8, 40.0)
    for rings, sectors in ((0, 8), (33, 8), (4, 2), (4, 66), (4, 7)):
        with pytest.raises(ValueError):
            ops.scan_context_build(xyz, count, rings, sectors, 40.0, 1.0, 2.0, tables=tables)
    with pytest.raises(ValueError):
        ops.scan_context_build(xyz, count, 4, 8, 40.0, 41.0, 2.0)


# ------------------------------------------------------------------------------------------------------------ the search
def to_gpu(norm, masks):
    return (torch.from_numpy(np.ascontiguousarray(norm, np.float32)).to(DEV),
            torch.tensor([S.mask_to_int64(int(m)) for m in masks], device=DEV, dtype=torch.int64))


def gpu_search(qn, qm, dn, dm, limits, K, rows=None):
    from deeppointmap_amd import ops
    q, m = to_gpu(qn, qm)
    d, dmask = to_gpu(dn, dm)
    out = ops.scan_context_search(q, m, d, dmask, torch.tensor(limits, device=DEV, dtype=torch.int32), K, rows=rows)
    return [t.cpu().numpy() for t in out]


def check_against_the_restatement(case, limits, K, got, what):
    """distances within the bound of the float64 restatement's; rows and shifts equal where its gaps are clear -> (compared,
    skipped) decisions"""
    dist, row, shift = got
    compared = skipped = 0
    for q, limit in enumerate(limits):
        rank = H.ranking(case, q, limit, K)
        for k in range(K):
            if k >= limit:
                assert np.isinf(dist[q, k]) and row[q, k] == -1 and shift[q, k] == -1, (what, q, k)
                continue
            d, c, s, b, gap = rank[k]
            err = abs(float(dist[q, k]) - d)
            bound = max(b, rank[k - 1][3]) if k else b
            log(f"search {what} q {q} rank {k}: |gpu - r64| {err:.3e}, bound {bound:.3e}, |r32 - r64| {case.spread[q, c]:.3e}, "
                f"row {row[q, k]} (r64 {c}), shift {shift[q, k]} (r64 {s}), d {d:.6f}")
            assert err <= bound, (what, q, k, err, bound)
            clear = gap > 2 * b and (k == 0 or rank[k - 1][4] > 2 * rank[k - 1][3])
            if clear:
                assert row[q, k] == c, (what, q, k)
            if clear and case.shift_gap[q, c] > 2 * case.bound[q, c]:
                assert shift[q, k] == s, (what, q, k)
                compared += 1
            else:
                skipped += 1
    return compared, skipped


@pytest.mark.parametrize("seed", H.SEEDS)
@pytest.mark.parametrize("K", [1, 4, 8])
@pytest.mark.parametrize("D", H.DS)
def test_search_is_the_restatement(D, K, seed):
    case = H.search_case(seed)
    limits = [D] * H.QUERIES
    got = gpu_search(case.qn, case.q_mask, case.db[:D], case.db_mask[:D], limits, K)
    compared, skipped = check_against_the_restatement(case, limits, K, got, f"D {D} K {K} seed {seed}")
    assert skipped <= 0.01 * (compared + skipped)
    again = gpu_search(case.qn, case.q_mask, case.db[:D], case.db_mask[:D], limits, K)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


def test_limits_zero_below_k_and_unequal():
    case = H.search_case(H.SEEDS[0])
    limits = [0, 2, 77]
    got = gpu_search(case.qn, case.q_mask, case.db, case.db_mask, limits, 4)
    assert np.isinf(got[0][0]).all() and (got[1][0] == -1).all() and (got[2][0] == -1).all()
    assert (got[1][1][:2] >= 0).all() and (got[1][1][:2] < 2).all() and (got[1][1][2:] == -1).all() and np.isinf(got[0][1][2:]).all()
    assert (got[1][2] < 77).all() and (got[1][2] >= 0).all()
    check_against_the_restatement(case, limits, 4, got, "limits 0 2 77")
    # the `rows` argument hides the tail of a preallocated database like a limit does
    part = gpu_search(case.qn, case.q_mask, case.db, case.db_mask, [130, 130, 130], 4, rows=77)
    full = gpu_search(case.qn, case.q_mask, case.db, case.db_mask, [77, 77, 77], 4)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(part, full))


def test_empty_query_empty_rows_and_duplicates_tie_by_rule():
    case = H.search_case(H.SEEDS[1])
    Z = np.zeros((1, H.RINGS, H.SECTORS), np.float32)
    dist, row, shift = gpu_search(Z, [0], case.db, case.db_mask, [130], 8)
    assert (dist == 1).all() and row[0].tolist() == list(range(8)) and (shift == 0).all()
    db = np.concatenate([case.db[:5], Z, case.db[2:3], case.db[:3]])          # rows 2, 6 and 9 are one descriptor; row 5 is empty
    dm = case.db_mask[:5] + [0] + case.db_mask[2:3] + case.db_mask[:3]
    dist, row, shift = gpu_search(case.db[2:3], case.db_mask[2:3], db, dm, [len(db)], 4)
    assert row[0, :3].tolist() == [2, 6, 9] and (shift[0, :3] == 0).all() and dist[0, 0] == dist[0, 1] == dist[0, 2] <= H.FLOOR
    dist, row, shift = gpu_search(case.db[:1], case.db_mask[:1], Z, [0], [1], 2)
    assert dist[0].tolist() == [1.0, np.inf] and row[0].tolist() == [0, -1] and shift[0].tolist() == [0, -1]


@pytest.mark.parametrize("rings,sectors", [(20, 60), (5, 8), (32, 64), (3, 32), (7, 34)])
def test_turned_copies_are_found_at_their_exact_shift(rings, sectors):
    rng = np.random.default_rng(rings * 100 + sectors)
    A, masks = H.normalised(S.random_descriptors(rng, 3, rings, sectors, empty_columns=1))
    turns = [0, 1, sectors // 2, sectors - 1, 3 % sectors]
    db, dm = [A[1]], [masks[1]]
    for m in turns:
        B, bm = S.roll_columns(A[0], masks[0], m)
        db.append(B), dm.append(bm)
    db.append(A[2]), dm.append(masks[2])
    dist, row, shift = gpu_search(A[:1], masks[:1], np.stack(db), dm, [len(db)], len(turns))
    assert row[0].tolist() == list(range(1, len(turns) + 1)), (row, dist)       # equal distances: the smaller row first
    assert shift[0].tolist() == turns and (dist[0] <= (rings + 8) * 2.0 ** -24).all()
    log(f"turned copies {rings} x {sectors}: distances {dist[0].tolist()}")


def test_search_refuses_what_the_header_says():
    case = H.search_case(H.SEEDS[0])
    for K in (0, 9):
        with pytest.raises(ValueError):
            gpu_search(case.qn, case.q_mask, case.db, case.db_mask, [1, 1, 1], K)
