"""CPU: the restatements of the scan filters (tests/filters_restated.py) are right, and the cases (tests/filters_cases.py) have
power.  tests/test_gpu_filters_exact.py compares the HIP kernels with these restatements row by row and bit by bit; what is
proved here, without a GPU, is that such a comparison means something:

  * agreement with the oracle where the oracle is decisive (tie-free clouds), and an account of every row where it is not;
  * closed forms: plane normals, the cut's thresholds, mean_dist on a 3-4-5 line;
  * reach: the cases named after a code path (compaction, radius doubling, stretched cells, one-cell grid) get there;
  * power: the wrong tie rule, the inclusive radius and the other comparison of the cut each change what is compared;
  * the tolerance of the normals: two evaluations of the reference stay inside the per-row bound the GPU test uses."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filters_cases as C  # noqa: E402
import filters_restated as FR  # noqa: E402
from oracle import dpm_oracle as O  # noqa: E402

EXEMPT_BOUND = 1e-3      # rows whose bound on sin(angle) exceeds this are exempt ...
EXEMPT_SHARE = 0.01      # ... and may be at most this share of a random cloud (none on a lattice case)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------
# agreement with the oracle
# ------------------------------------------------------------------------------------------------------------------
def test_knn_equals_oracle_on_a_tie_free_cloud():
    rng = np.random.default_rng(7501)
    xyz = (20.0 * rng.random((3000, 3))).astype(np.float32)
    for K in (1, 16):
        got = FR.knn_self(xyz, K)
        widx, wd2 = O.knn_self(torch.from_numpy(xyz), K)
        d2 = got["dist2"]
        assert not (d2[:, 1:] == d2[:, :-1]).any()                       # tie-free: the oracle's shortlist cannot matter
        assert np.array_equal(got["idx"], widx.numpy()) and np.array_equal(bits(d2), bits(wd2.numpy()))
        assert np.array_equal(got["mean_dist"], FR.knn_prefix(FR.knn_self(xyz, 20), K)["mean_dist"])     # prefixes of a larger K


def test_real_frame_every_difference_from_the_oracle_is_a_tie_its_shortlist_lost():
    xyz = C.real_frame()
    assert xyz.shape[0] > 20000
    for K in (10, 16):
        ref = C.knn_reference("real", K)
        widx, wd2 = O.knn_self(torch.from_numpy(xyz), K)
        widx = widx.numpy()
        assert np.array_equal(bits(ref["dist2"]), bits(wd2.numpy()))    # the distances agree everywhere
        rows = np.nonzero((ref["idx"] != widx).any(1))[0]
        print(f"real frame, K = {K}: {len(rows)} of {xyz.shape[0]} rows differ from the oracle in idx: {rows.tolist()}")
        for r in rows:
            cols = np.nonzero(ref["idx"][r] != widx[r])[0]
            own = FR.direct_d2(xyz[r:r + 1], xyz[widx[r]])[0]
            # the oracle's picks are genuine points at bit-equal distances (a tie), and at the first column that differs the
            # brute force holds the SMALLER index: the oracle never saw that point -- it was outside its K + 5 shortlist
            assert np.array_equal(bits(own), bits(ref["dist2"][r])), (K, r)
            assert ref["idx"][r, cols[0]] < widx[r, cols[0]], (K, r)
            print(f"  row {r}: columns {cols.tolist()}, d^2 = {ref['dist2'][r, cols].tolist()}, "
                  f"brute force {ref['idx'][r, cols].tolist()}, oracle {widx[r, cols].tolist()}")


def test_oracle_normals_take_the_strict_fp32_radius():
    for name, (xyz, radius) in C.normals_cases().items():
        ref = C.normals_reference(name)
        got = O.point_normals(torch.from_numpy(xyz), radius).numpy().astype(np.float64)
        unit = np.array([0.0, 0.0, 1.0])
        low = ref["count"] < 3
        assert np.array_equal(got[low], np.tile(unit, (int(low.sum()), 1))), name
        ok = FR.normals_bound(ref) <= EXEMPT_BOUND
        assert (FR.sin_angle(got[ok], ref["normals"][ok]) <= 1e-6).all(), name
    xyz, rows, radius = C.on_radius()
    incl = FR.point_normals(xyz, radius, rule="<=")["normals"]
    got = O.point_normals(torch.from_numpy(xyz), radius).numpy()
    assert (FR.sin_angle(got[rows], incl[rows]) > 1e-2).all()           # ... and not the inclusive one


# ------------------------------------------------------------------------------------------------------------------
# closed forms
# ------------------------------------------------------------------------------------------------------------------
def test_plane_normals_in_closed_form():
    xyz, exact = C.planes()
    ref = C.normals_reference("planes")
    assert (ref["count"] >= 3).all() and ref["count"].max() <= 64
    assert (np.abs((ref["normals"] * exact).sum(1)) >= 1 - 1e-12).all()
    xyz, low, tri, run, direction = C.few()
    ref = C.normals_reference("few")
    assert ref["count"][low].tolist() == [1, 2, 2] and ref["count"][tri].tolist() == [3, 3, 3]
    assert np.array_equal(ref["normals"][low], np.tile([0.0, 0.0, 1.0], (3, 1)))
    assert (np.abs(ref["normals"][tri][:, 2]) >= 1 - 1e-12).all()
    assert (ref["count"][run] >= 3).all() and (np.abs(ref["normals"][run] @ direction) <= 1e-7).all()


@pytest.mark.parametrize("scale", [1.0, 2.0 ** -7, 2.0 ** 9])
def test_cut_thresholds_are_exact(scale):
    for N in C.CUT_N:
        stat, _, _ = C.cut_case(N, scale)
        for mode in (0, 1):
            mean_f, std_f, thr = FR.stat_threshold(stat, 1.0, mode)
            if N == 1:
                assert (mean_f, std_f, thr) == (scale, 0.0, scale)
            else:
                assert (mean_f, std_f, thr) == (scale, scale, 2 * scale if mode == 0 else 0.0), (N, mode)
    stat, _, _, k = C.cut_other("nan")
    assert np.isnan(FR.stat_threshold(stat, k, 0)[2]) and np.isnan(FR.stat_threshold(stat, k, 1)[2])


def test_mean_dist_on_the_345_line_is_exact():
    xyz = C.knn_case("line345")
    t = np.rint(xyz[:, 0].astype(np.float64) * 8 / 3).astype(np.int64)
    gap = np.sort(np.abs(t[:, None] - t[None, :]), axis=1)[:, 1:]        # |dt| to the others, ascending
    for K in (4, 16):
        ref = C.knn_reference("line345", K)
        exact = gap[:, :K].sum(1) * 0.625 / K
        assert np.array_equal(ref["mean_dist"].astype(np.float64), exact) and np.array_equal(ref["mean_dist64"], exact)


# ------------------------------------------------------------------------------------------------------------------
# reach
# ------------------------------------------------------------------------------------------------------------------
def test_cases_reach_the_paths_they_are_named_for():
    geo = {n: FR.grid_geometry(C.knn_case(n), C.KNN_CELL) for n in ("lattice_box", "column", "sparse", "wide", "line", "same", "stacks")}
    assert geo["column"]["block3"].min() > 448 * 3                      # every query compacts its list, several times
    col = geo["column"]
    assert col["g"] == 2 and col["count"].min() > 448 and (np.diff(col["cy"][:-1]) <= 0).all()     # grid row 1 first in the index order
    assert geo["lattice_box"]["block3"].max() <= 448 and geo["lattice_box"]["g"] == 9       # ... and the box never does
    assert geo["same"]["g"] == 1 and geo["same"]["count"][0, 0] == 1100
    assert geo["wide"]["cs"] > np.float32(C.KNN_CELL) and geo["wide"]["g"] == 128
    assert geo["line"]["cx"].max() == 0 and geo["line"]["g"] == 31
    assert geo["sparse"]["cs"] == np.float32(C.KNN_CELL) and geo["sparse"]["g"] > 64
    for K in C.KS:                                                       # rows whose K-th distance exceeds 1, 2, 4 and 8 cells
        kth = np.sqrt(C.knn_reference("sparse", K)["dist2"][:, K - 1].astype(np.float64)) / float(geo["sparse"]["cs"])
        assert (kth > 8).sum() >= 10 and ((kth < 1).sum() >= 1000 or K == 63), K
    kth = np.sqrt(C.knn_reference("stacks", 16)["dist2"][:, 15].astype(np.float64))
    assert (kth > 2).sum() > 500                                         # short stacks borrow from the stacks around them
    for n in C.KNN_BOX_N:
        assert C.knn_case(f"box{n}").shape[0] == n


# ------------------------------------------------------------------------------------------------------------------
# power
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lattice_box", "duplicates", "stacks", "column"])
def test_breaking_ties_by_the_largest_index_changes_half_of_the_rows(name):
    xyz = C.knn_case(name)
    for K in (10, 16):
        ref = C.knn_reference(name, K)
        wrong = FR.knn_self(xyz, K, tie="largest")
        assert np.array_equal(np.sort(bits(wrong["dist2"]), 1), np.sort(bits(ref["dist2"]), 1)) or name == "duplicates"
        changed = (wrong["idx"] != ref["idx"]).any(1).mean()
        print(f"{name}, K = {K}: ties by the largest index change {changed:.1%} of the rows")
        assert changed >= 0.5, (name, K)


def test_duplicates_make_a_point_its_own_neighbour():
    ref = C.knn_reference("duplicates", 10)
    own = (ref["idx"] == np.arange(ref["idx"].shape[0])[:, None]).any(1)
    assert 0.3 < own.mean() < 0.9                                       # every copy but the one of smallest index
    assert (ref["dist2"][own, 0] == 0).all()


def test_the_inclusive_radius_changes_every_on_radius_normal():
    xyz, rows, radius = C.on_radius()
    strict, incl = C.normals_reference("on_radius"), FR.point_normals(xyz, radius, rule="<=")
    assert len(rows) >= 30 and (incl["count"][rows] > strict["count"][rows]).all()
    assert np.array_equal(np.abs(strict["normals"][rows]), np.tile([0.0, 0.0, 1.0], (len(rows), 1)))    # strictly: the plane alone
    moved = FR.sin_angle(strict["normals"][rows], incl["normals"][rows])
    print(f"on_radius: {len(rows)} rows, the inclusive rule moves their normals by sin(angle) >= {moved.min():.3f}")
    assert (moved > 1e-2).all()
    # plane points ON the radius in the plane exist as well (offsets (3, 4, 0) / 8): counted by <=, invisible in the normal
    assert (incl["count"] > strict["count"]).sum() > 10 * len(rows)


def test_the_other_comparison_changes_the_survivor_count():
    for N in C.CUT_N:
        stat, xyz, idx = C.cut_case(N)
        m = N // 2
        for mode, other, want, wrong in ((0, "<", N, N - m), (1, ">=", m + (N > 1), N)):
            n_ok = FR.stat_filter(stat, 1.0, mode, xyz, idx)[2]
            n_bad = FR.stat_filter(stat, 1.0, mode, xyz, idx, cut=other)[2]
            if N == 1:
                want, wrong = (1, 0) if mode == 0 else (0, 1)           # the lone point is ON both thresholds
            assert (n_ok, n_bad) == (want, wrong) and n_ok != n_bad, (N, mode)
    stat, xyz, idx, k = C.cut_other("nan")
    assert FR.stat_filter(stat, k, 0, xyz, idx)[2] == 0 and FR.stat_filter(stat, k, 1, xyz, idx)[2] == 0
    stat, xyz, idx, k = C.cut_other("two")
    assert FR.stat_filter(stat, k, 0, xyz, idx)[1].tolist() == [11] and FR.stat_filter(stat, k, 1, xyz, idx)[1].tolist() == [5]
    # the cloud that carries the cut pattern through the outlier chain
    cloud = C.cut_chain_cloud()
    ref = FR.knn_self(cloud, 1)
    assert sorted(np.unique(ref["mean_dist"], return_counts=True)[1].tolist()) == [1, 400, 400]
    assert FR.stat_threshold(ref["mean_dist"], 1.0, 0) == (1.0, 1.0, 2.0)
    assert FR.stat_filter(ref["mean_dist"], 1.0, 0, cloud)[2] == 801 and FR.stat_filter(ref["mean_dist"], 1.0, 0, cloud, cut="<")[2] == 401


def test_ball_query_cases_have_their_edges():
    pts, lengths, ctr = C.ball_batch()
    for radius in C.BALL_RADII:
        full = FR.ball_query(pts, lengths, ctr, 300, radius)
        r2 = np.float32(radius * radius)
        for b in (0, 2):
            d2 = FR.expanded_d2(ctr[b], pts[b, :lengths[b]])
            hits = (~(d2 > r2)).sum(1)
            assert (d2 == r2).any(1)[10:16].all()                       # points EXACTLY on the radius, which `>` keeps
            assert hits[9] == 0 and not full[b, 9].any()                # nothing in range: zeros
            assert (hits[:8] >= 1).all()
            if radius == 2.5:
                assert hits.max() > 100 and (full[b, :, 99].max() >= 256 or b == 2)     # K = 100 reaches the last chunk
                assert ((hits > 16) & (full[b, :, 15] % 64 != 63)).any()
            else:
                assert 0 < np.median(hits) < 16                         # a handful of hits: the padding loop runs
        assert not full[1].any()                                        # a frame of length 0


def test_ball_query_restatement_equals_the_reference_where_a_centre_has_a_hit():
    """tests/golden/ball_query.npz: the reference's own torch Querier.ball_query on the same batch (make_golden_ball_query.py).
    A centre without a hit is index N in every slot there (an out-of-range gather downstream) and 0 here: not compared."""
    from conftest import load_golden
    g = load_golden("ball_query.npz")
    pts, lengths, ctr = C.ball_batch()
    for radius in C.BALL_RADII:
        for K in C.BALL_K:
            want, hit = g[f"r{radius}_K{K}.idx"], g[f"r{radius}_K{K}.hit"]
            got = FR.ball_query(pts, lengths, ctr, K, radius)
            assert hit.sum() > 100 and not hit[1].any()
            assert np.array_equal(got[hit], want[hit]) and not got[~hit].any() and (want[~hit] == pts.shape[1]).all()


# ------------------------------------------------------------------------------------------------------------------
# the tolerance of the normals
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["planes", "on_radius", "few", "random", "random_2km"])
def test_two_evaluations_of_the_normals_stay_inside_the_bound(name):
    xyz, radius = C.normals_cases()[name]
    ref = C.normals_reference(name)
    other = FR.point_normals_centred(xyz, radius)
    bound = FR.normals_bound(ref)
    if name == "few":
        bound[C.few()[3]] = np.inf                                      # the collinear run: no unique normal
    exempt = bound > EXEMPT_BOUND
    sin = FR.sin_angle(ref["normals"], other)
    live = ~exempt & (bound > 0)
    worst = float((sin[live] / bound[live]).max())
    print(f"{name}: {int(exempt.sum())} of {len(bound)} rows exempt, worst sin(angle) / bound = {worst:.3g}")
    assert (sin[~exempt] <= bound[~exempt]).all()
    if name.startswith("random"):
        assert exempt.mean() <= EXEMPT_SHARE
    elif name == "few":
        assert exempt.sum() == len(C.few()[3])
    else:
        assert not exempt.any()
