"""CPU: what the exact information-matrix tests (tests/test_gpu_infomat_exact.py) rest on.

 * the restatement (tests/infomat_restated.py) agrees with the oracle on the reference's own fixture cases and with the hand
   case of the GPU suite;
 * SENSITIVITY: in every case, every query that has a second target within the radius is given that target instead of its
   nearest one, one query at a time; each of these swaps must change the 36 floats.  The cap is 100 %, and it is a property of
   the cases and the reference alone: the sizing rule of tests/golden/infomat_exact_cases.py keeps a change of one lattice step
   in a first moment above the final fp32 rounding.  (A target that COINCIDES with the match has the same moments and is no
   other answer; `second` is the nearest target at another position.)
 * every case reaches the property it exists for; the counts go to profiles/infomat_exactness.md."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, T
from oracle import dpm_oracle as O

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import infomat_exact_cases as C  # noqa: E402
import infomat_restated as IR  # noqa: E402

NAMES = list(C.SINGLE)


def test_restatement_vs_oracle_on_reference_fixture():
    """the infomat.npz cases (general poses, fp32 clouds): the queries are transformed in fp64, both clouds snapped to the
    2^-19 m lattice and the restatement runs with the identity.  Same matched count as the oracle, entries within the bound
    tests/test_oracle_golden.py holds the oracle to.  Why 2^-19: the snap moves a squared distance near r^2 = 1 by at most
    2 sqrt(3) 2^-19 = 6.6e-6, and the fixture's closest call is a neighbour at d^2 = 1 + 2.0e-5 (synthetic35_poor; at 2^-13
    the snap takes it in); squared distances of 120 m are still integers below 2^53 there, so the search stays exact.  The
    moment sums are not (60 m squared, thousands of times): exact=False, the comparison is at a tolerance anyway."""
    from test_oracle_golden import _infomat_cases
    g, cases = _infomat_cases()
    s = 19
    for name, (a, b) in cases.items():
        SE3 = g[name + ".SE3"].astype(np.float64)
        q = SE3[:3, :3] @ a.numpy().astype(np.float64) + SE3[:3, 3:]
        snap = lambda v: np.rint(v * (1 << s)) / (1 << s)
        ref = IR.restate(snap(q), snap(b.numpy().astype(np.float64)), C.IDENTITY, 1.0, s, exact=False)
        want = O.information_matrix(a, b, T(g[name + ".SE3"])).numpy()
        print(f"{name}: matched {ref['G'][3, 3]:.0f} (oracle {want[3, 3]:.0f}), max |diff| {np.abs(ref['G'] - want).max():.3e}, "
              f"bound {2e-4 * np.abs(want).max():.3e}")
        assert ref["G"][3, 3] == want[3, 3], name
        np.testing.assert_allclose(ref["G"], want, rtol=2e-4, atol=2e-4 * np.abs(want).max(), err_msg=name)


def test_restatement_hand_case():
    """the hand case of tests/test_gpu_decoder.py::test_information_matrix_vs_oracle"""
    a = np.array([[0.0, 10, 20], [0, 0, 0], [1, 2, 3]], dtype=np.float32)
    G = IR.restate(a, a, C.IDENTITY, 1.0, 5)["G"]
    assert G[3, 3] == 3.0 and G[0, 4] == -6.0 and G[1, 5] == -30.0
    assert G[0, 0] == 14.0 and G[1, 1] == 14.0 + 500.0 and G[0, 2] == -(10 * 2 + 20 * 3)
    Z = IR.restate(a, a + 50.0, C.IDENTITY, 1.0, 5)
    assert not Z["G"].any() and (Z["match"] == -1).all()
    # ties go to the smallest index, the radius is inclusive, one step beyond is out
    t = np.array([[1.0, -1.0, 0, 0], [0, 0, 1.0, 2.0], [0, 0, 0, 0]], dtype=np.float32)
    q = np.array([[0.0, 0.0], [0.0, 3.03125], [0.0, 0.0]], dtype=np.float32)
    r = IR.restate(q, t, C.IDENTITY, 1.0, 5)
    assert r["match"].tolist() == [0, -1] and r["tied"].tolist() == [True, False] and r["d2"].tolist() == [1024, 33 * 33]


def stats(name):
    """the reference-side counts of one case"""
    c, ref = C.case(name), C.reference(name)
    g = C.grid_shape(c["pcd2"], c["radius"])
    R = IR.radius_units(c["radius"], c["s"])
    m = ref["match"] >= 0
    qrow, qcol = C.query_cells(g, ref["q"] / float(1 << c["s"]))
    drow = np.abs(g["row"][ref["match"][m]] - qrow[m])
    dcol = np.abs(g["col"][ref["match"][m]] - qcol[m])
    dq = np.abs(ref["t"][ref["match"][m]] - ref["q"][m])
    x, y = c["pcd2"][0], c["pcd2"][1]
    lo, hi = ref["t"].min(0), ref["t"].max(0)
    outside = ((ref["q"][:, :2] < lo[:2]) | (ref["q"][:, :2] > hi[:2])).any(1)
    return dict(N1=c["pcd1"].shape[1], N2=c["pcd2"].shape[1], r=c["radius"], extent=(float(x.max() - x.min()), float(y.max() - y.min())),
                H=g["H"], gx=g["gx"], gy=g["gy"], chunks=g["chunks"], longest_row=int(np.bincount(g["row"]).max()),
                matched=int(m.sum()), unmatched=int((~m).sum()), on_radius=int((m & (ref["d2"] == R * R)).sum()),
                just_beyond=int(((ref["d2"] > R * R) & (ref["d2"] <= (R + 1) ** 2)).sum()), tied=int(ref["tied"].sum()),
                ring2=float(((drow >= 2) | (dcol >= 2)).mean()) if m.any() else 0.0,
                far_y=float((dq[:, 1] > 0.51 * R).mean()) if m.any() else 0.0,
                far_x=float((dq[:, 0] > 0.51 * R).mean()) if m.any() else 0.0,
                outside_matched=int((outside & m).sum()), swaps=int((ref["second"] >= 0).sum()))


@pytest.mark.parametrize("name", NAMES)
def test_every_swap_to_the_second_target_is_visible(name):
    c, ref = C.case(name), C.reference(name)
    assert C.case(name)["pcd1"].shape[1] * float(np.abs(c["pcd2"]).max()) * 4 < 2 ** 23 * 2.0 ** -c["s"]  # the sizing rule
    G, who = IR.swapped_matrices(ref)
    seen = (G.view(np.uint32) != ref["G"].view(np.uint32)[None]).any((1, 2))
    print(f"{name}: {len(who)} swaps, {int(seen.sum())} change the matrix")
    assert seen.all(), (name, who[~seen][:10])


@pytest.mark.parametrize("n_pairs", list(C.PAIR_LISTS))
def test_every_swap_is_visible_in_the_batched_pairs(n_pairs):
    assert C.N_BATCH * float(np.abs(C.frames()).max()) * 4 < 2 ** 23 * 2.0 ** -5
    for p in range(n_pairs):
        ref = C.pair_reference(n_pairs, p)
        G, who = IR.swapped_matrices(ref)
        seen = (G.view(np.uint32) != ref["G"].view(np.uint32)[None]).any((1, 2))
        print(f"P = {n_pairs}, pair {p} {C.PAIR_LISTS[n_pairs][p]}: matched {ref['G'][3, 3]:.0f}, {len(who)} swaps, {int(seen.sum())} change the matrix")
        assert seen.all() and ref["G"][3, 3] > 500, (n_pairs, p)


def test_cases_reach_their_properties():
    st = {n: stats(n) for n in NAMES}
    for n, v in st.items():
        print(n, v)
    v = st["fine_partial_chunks"]
    assert (v["N1"], v["N2"], v["H"], v["chunks"]) == (3000, 4097, 2, 2) and v["N1"] % 256 and v["N2"] % C.GB_CHUNK == 1
    assert v["matched"] > 0 and v["unmatched"] > 0 and v["outside_matched"] >= 100
    v = st["second_ring"]
    assert v["H"] == 2 and v["far_y"] >= 0.25 and v["far_x"] >= 0.25 and v["unmatched"] >= 0.20 * v["N1"]
    v = st["on_radius_and_ties"]
    assert v["on_radius"] >= 100 and v["just_beyond"] >= 100 and v["tied"] >= 100
    ref = C.reference("on_radius_and_ties")
    assert (ref["match"][ref["d2"] == 1024] >= 0).all() and (ref["match"][ref["d2"] > 1024] == -1).all()
    v = st["coarse_grid"]
    assert v["H"] == 1 and max(v["extent"]) / v["r"] >= 511 and v["matched"] > 1000 and v["on_radius"] >= 100
    v = st["full_grid_fine"]
    assert v["H"] == 2 and 256 < max(v["extent"]) / v["r"] < 511 and min(v["gx"], v["gy"]) > 256
    assert v["extent"][0] == v["extent"][1] == 40.0
    v = st["long_rows"]
    c, ref = C.case("long_rows"), C.reference("long_rows")
    in_band = lambda p: (p[:, 1] >= C.BAND_Y0) & (p[:, 1] < C.BAND_Y0 + 16)       # a 0.5 m band of y that holds the built one
    assert (v["N2"], v["chunks"]) == (9001, 3) and v["N2"] % C.GB_CHUNK
    assert in_band(ref["t"]).sum() >= 2000 and v["longest_row"] > 512 and in_band(ref["q"]).sum() >= 200
    v = st["far_from_origin"]
    assert v["N1"] <= 400 and v["N1"] > 256 and float(np.abs(C.case("far_from_origin")["pcd2"]).max()) > 2000 and v["matched"] > 100
    for n in ("permuted_rot_z", "permuted_cyclic"):
        assert np.array_equal(C.reference(n)["q"], C.reference("fine_partial_chunks")["q"])  # the pose lands on the base case's queries
        assert np.array_equal(C.reference(n)["match"], C.reference("fine_partial_chunks")["match"])
        assert not np.array_equal(C.case(n)["Rt"], C.IDENTITY)
    assert st["one_target"]["N2"] == 1 and 0 < st["one_target"]["matched"] < 300
    assert st["one_query"]["N1"] == 1 and st["one_query"]["matched"] == 1
    v = st["coincident_targets"]
    assert v["N2"] == 50 and v["extent"] == (0.0, 0.0) and 0 < v["matched"] < 300 and (v["gx"], v["gy"]) == (1, 1)
    v = st["vertical_line"]
    assert v["N2"] == 2000 and (v["gx"], v["gy"]) == (1, 1) and v["longest_row"] == 2000 and v["matched"] > 100 and v["unmatched"] > 0
    v = st["stacks"]
    c, ref = C.case("stacks"), C.reference("stacks")
    g = C.grid_shape(c["pcd2"], c["radius"])
    per_cell = np.bincount(g["row"] * g["gx"] + g["col"])
    assert set(per_cell[per_cell > 0].tolist()) == set(range(1, 25))              # stacks of 1 .. 24 targets, one cell each
    assert v["unmatched"] == 0 and np.array_equal(np.sort(ref["match"]), np.arange(v["N2"]))  # every target wins exactly once
    drow = g["row"][ref["match"]] - C.query_cells(g, ref["q"] / 32.0)[0]
    deep = per_cell[g["row"] * g["gx"] + g["col"]][ref["match"]] > 8             # the stack goes past the first eight candidates
    assert all(((drow == k) & deep).sum() >= 50 for k in (-2, -1, 0, 1, 2))       # ... in every row of the 5 x 5 block
    v = st["no_match"]
    assert v["matched"] == 0 and not C.reference("no_match")["G"].any()
    # batched: in every list some source is another pair's target, frame 4 is nobody's, and a self pair matches all N points
    for P, pairs in C.PAIR_LISTS.items():
        dst = {b for _, b in pairs}
        assert len(pairs) == P and any(a not in dst for a, _ in pairs)
        assert any(a == b2 for p, (a, _) in enumerate(pairs) for p2, (_, b2) in enumerate(pairs) if p2 != p)
        selfp = [p for p, (a, b) in enumerate(pairs) if a == b]
        assert selfp and C.N_BATCH % 256
        assert C.pair_reference(P, selfp[0])["G"][3, 3] == C.N_BATCH
    _write_report(st)


def _write_report(st):
    lines = ["# Exact information-matrix cases: what the reference side counts",
             "",
             "Written by `tests/test_infomat_host.py` (CPU, from seeds; `tests/golden/infomat_exact_cases.py`).  Every case lies on a",
             "dyadic lattice, so the expected matrix is `float32(exact value)` and `tests/test_gpu_infomat_exact.py` compares raw bits.",
             "`swaps` = queries with a second target (at another position) within the radius; giving any one of them that target",
             "changes the 36 floats -- checked for every one of them (100 %).  `ring 2` = share of the matched queries whose match lies",
             "two grid rows or columns away; `|dy|>.51r` / `|dx|>.51r` = share whose match is further than 0.51 r away along that axis.",
             "",
             "| case | N1 | N2 | r | extent x, y (m) | H | gx x gy | longest row | matched | unmatched | on radius | just beyond | tied "
             "| ring 2 | \\|dy\\|>.51r | \\|dx\\|>.51r | swaps | reaches |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for n, v in st.items():
        lines.append(f"| {n} | {v['N1']} | {v['N2']} | {v['r']:g} | {v['extent'][0]:g}, {v['extent'][1]:g} | {v['H']} | {v['gx']} x {v['gy']} | "
                     f"{v['longest_row']} | {v['matched']} | {v['unmatched']} | {v['on_radius']} | {v['just_beyond']} | {v['tied']} | "
                     f"{v['ring2']:.3f} | {v['far_y']:.3f} | {v['far_x']:.3f} | {v['swaps']} | {C.case(n)['branch']} |")
    lines += ["", f"Batched: {C.F_FRAMES} frames of {C.N_BATCH} points, pair lists of " +
              ", ".join(str(k) for k in C.PAIR_LISTS) + " (8 and 16: XCD-aware block mapping); frame 4 is never a target, so its pairs",
              "walk the queries in index order while the others walk them in the cell order of another pair's grid.", ""]
    try:
        with open(os.path.join(ROOT, "profiles", "infomat_exactness.md"), "w") as f:
            f.write("\n".join(lines))
    except OSError:
        pass
