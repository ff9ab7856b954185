"""GPU: the hybrid neighbour search (csrc/knn.hip) exit by exit.

Every case of tests/knn_paths_cases.py exists for named exits of the search -- the tie replays of both torch.topk regimes on both
paths, a full tie queue, a full todo list, the five exits of knn_grid_fast_kernel, the three grid layouts, the grid-size floor,
the edge row shapes -- and tests/test_knn_paths_host.py proves on the CPU, from the reference's arithmetic alone, that its rows
take them.  Here each case runs and must give

  result   every row the multiset the search is specified to return (reference(name)["spec"]): the oracle's members within the
           radius, the remaining slots filled with the nearest point.  Where the row's minimum distance is attained once that IS
           the oracle's row; where two points tie for nearest, the search takes the smaller index and the reference whatever its
           sort put first -- the same point twice in the frame or, far from the origin, two points whose float32 distances
           coincide ("Exits of the neighbour search").  Slot 0: the oracle's index where the minimum is untied, a
           point at the minimum distance otherwise.  No row is excused.
  fallback the one exception, tieq_overflow_nth: tied rows beyond the queue's 4096 keep the smaller indices in the
           nth_element regime (the deviation finish() documents).  A row may differ from the oracle only in members at the
           row's K-th distance, only if it is a tied row, and at most (census tie count - 4096) rows may.
  census   ops.knn_grid_census after the prebuilt form: g, H, h, lox, loy equal to the restated header, inv_cs and err2 within
           a relative 1e-5 (float sqrt and division only; the largest difference is printed), at least as many rows left to the
           full search and offered to the tie queue as the restatement is sure of -- and no more left to the full search than
           it allows, so a fast kernel that hands everything on fails too.
  forms    the one-call form and, on grid cases in the heap regime, brute=True give the same; so does a second call (the grid is
           scattered with atomics).  The forced brute search in the nth regime above ~1900 points has a documented deviation of
           its own (no LDS row for the replay: dpm_knn_hybrid_reuse) and is left out; no case here has such a shape anyway.
  fp64     on the cases inside the unit cube, test_gpu_ops.knn_rows_ok's band check against exact fp64 distances at its
           documented 4e-6 (the expanded form's error there is below 1.5e-6: three roundings of numbers below 8): the guard
           against the float32 oracle and the kernel being wrong together.  Centres inside that cube only (the lifted and the
           far ones are not what the margin was derived for); long cases check 600 evenly spaced rows.

A failing row is reported with the exit the restatement assigns to it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_paths_cases as C  # noqa: E402
import knn_paths_restated as R  # noqa: E402
from test_gpu_ops import knn_rows_ok  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from deeppointmap_amd import ops as _ops
    return _ops


def dev(a, dtype=None):
    return torch.tensor(np.asarray(a), dtype=dtype).to(DEV)   # a copy: the cases are read-only and shared


def where(c, ref, b, s):
    """the exit the restatement assigns to row (b, s)"""
    if c["path"] != "grid":
        return "brute path"
    cl = ref["cls"][b]
    border = ("", ", border test must pass", ", border test must fail", ", border test may go either way")[int(cl["border"][s])]
    return (f"exit {R.EXITS[int(cl['exit'][s])]}{' (widened)' if cl['widened'][s] else ''}{' (tie in the block)' if cl['block_tie'][s] else ''}"
            f"{border}, {int(cl['tot'][s])} points in the block")


def distances_of(c, b, rows, idx):
    """expanded distances of the (len(rows), K) members `idx` of rows `rows` of frame b"""
    L = c["lens"][b]
    out = np.zeros(idx.shape, np.float32)
    for i0 in range(0, len(rows), R.CHUNK):
        d = R.expanded(c["ctr"][b, rows[i0:i0 + R.CHUNK]], c["pts"][b, :L])
        out[i0:i0 + R.CHUNK] = np.take_along_axis(d, np.clip(idx[i0:i0 + R.CHUNK], 0, L - 1), 1)
    return out


def check_rows(c, ref, got, form, excess_ties=None):
    """got (B, S, K) against the specification; excess_ties: the fallback case's allowance (None: every row exact)"""
    name, K = c["name"], c["K"]
    B, S = got.shape[:2]
    for b in range(B):
        assert ((got[b] >= 0) & (got[b] < c["lens"][b])).all(), (name, form, b, "an index outside the frame")
    bad = (np.sort(got, axis=2) != ref["spec"]).any(2)
    if excess_ties is None:
        if bad.any():
            b, s = np.argwhere(bad)[0]
            pytest.fail(f"{name} [{form}]: {int(bad.sum())} of {B * S} rows differ from the specified multiset; first: frame {b} row {s} "
                        f"({where(c, ref, b, s)}, tied row: {bool(ref['tie'][b, s])})\n got  {np.sort(got[b, s]).tolist()}\n want {ref['spec'][b, s].tolist()}")
    else:
        n_bad = int(bad.sum())
        print(f"{name} [{form}]: {n_bad} rows keep the smaller indices (allowed: {excess_ties})")
        assert n_bad <= excess_ties, (name, form, n_bad, excess_ties)
        assert not (bad & ~ref["tie"]).any(), (name, form, "a row without a boundary tie differs")
        for b in range(B):
            rows = np.flatnonzero(bad[b])
            if len(rows):
                kth = ref["dk"][b, rows, K - 1]
                dg, dw = distances_of(c, b, rows, got[b, rows]), ref["dk"][b, rows]
                # members strictly below the K-th distance are the oracle's, one for one; the rest sit AT the K-th distance
                assert (np.sort(np.where(dg < kth[:, None], got[b, rows], -1), 1) ==
                        np.sort(np.where(dw < kth[:, None], ref["want"][b, rows], -1), 1)).all(), (name, form, b)
                assert (dg <= kth[:, None]).all() and ((dg < kth[:, None]).sum(1) == (dw < kth[:, None]).sum(1)).all(), (name, form, b)
    # slot 0
    untied = ~ref["min_tied"]
    assert (got[..., 0][untied] == ref["want"][..., 0][untied]).all(), (name, form, "slot 0 is not the reference's nearest")
    for b in range(B):
        rows = np.flatnonzero(ref["min_tied"][b])
        if len(rows):
            d0 = distances_of(c, b, rows, got[b, rows, :1])[:, 0]
            assert (d0 == ref["dmin"][b, rows]).all(), (name, form, b, "slot 0 is not at the row's minimum distance")


def check_census(c, ref, cen):
    name = c["name"]
    B, S = c["ctr"].shape[:2]
    worst = 0.0
    for b, (hd, got) in enumerate(zip(ref["headers"], cen["frames"])):
        assert (got["g"], got["H"], got["h"]) == (hd["g"], hd["H"], hd["h"]), (name, b, got, hd["g"], hd["H"], hd["h"])
        assert got["lox"] == float(hd["lox"]) and got["loy"] == float(hd["loy"]), (name, b)
        for key in ("inv_cs", "err2"):
            rel = abs(got[key] - float(hd[key])) / float(hd[key])
            worst = max(worst, rel)
            assert rel <= 1e-5, (name, b, key, got[key], float(hd[key]))
    n = ref["counts"]
    n_tie = int(ref["tie"].sum())
    todo_max = n["todo_min"] + n["border_either"] + (n["block_tie"] if cen["tie"] > R.TIE_CAP else 0)
    print(f"{name}: census tie {cen['tie']} (restated tied rows {n_tie}), todo {cen['todo']} (restated {n['todo_min']}..{todo_max} of {B * S}), "
          f"frames " + "; ".join(f"g {f['g']} H {f['H']} h {f['h']} edge {1.0 / f['inv_cs']:.6g} err2 {f['err2']:.4g}" for f in cen["frames"]) +
          f"; largest header difference {worst:.2e}")
    assert n["todo_min"] <= cen["todo"] <= todo_max, (name, cen["todo"], n["todo_min"], todo_max)
    assert cen["tie"] >= n_tie, (name, cen["tie"], n_tie)
    if c["by_mark"]:
        assert cen["todo"] > B * c["pts"].shape[1], (name, "the todo list did not overflow")
    if c["fallback"] or name == "tieq_overflow_heap":
        assert cen["tie"] > R.TIE_CAP, (name, "the tie queue did not overflow")


@pytest.mark.parametrize("name", C.NAMES)
def test_case(ops, name):
    c, ref = C.case(name), C.reference(name)
    B, N, _ = c["pts"].shape
    K, r = c["K"], c["r"]
    pts, ctr, lens = dev(c["pts"]), dev(c["ctr"]), dev(c["lens"], torch.int32)
    runs = {}
    allowance = None
    if c["path"] == "grid":
        ws = ops.knn_grid(pts, lens, r)
        runs["prebuilt"] = ops.knn_hybrid(pts, lens, ctr, K, r, grid=ws).cpu().numpy()
        cen = ops.knn_grid_census(ws, B, N)
        check_census(c, ref, cen)
        if c["fallback"]:
            allowance = cen["tie"] - R.TIE_CAP
    runs["one call"] = ops.knn_hybrid(pts, lens, ctr, K, r).cpu().numpy()
    runs["one call again"] = ops.knn_hybrid(pts, lens, ctr, K, r).cpu().numpy()
    if c["path"] == "grid" and c["regime"] == "heap":
        runs["brute"] = ops.knn_hybrid(pts, lens, ctr, K, r, brute=True).cpu().numpy()
    for form, got in runs.items():
        # (the fallback's allowance is the prebuilt run's census; which rows find the queue full may differ from call to call, how
        # many offers there are does not: every tied row is offered once by the fast kernel or the full search, and once more
        # where the fast kernel found the queue full)
        check_rows(c, ref, got, form, allowance if form != "brute" else None)
    if c["fp64"]:
        got = runs["prebuilt" if c["path"] == "grid" else "one call"]
        for b in range(B):
            L = c["lens"][b]
            rows = np.flatnonzero((c["ctr"][b].astype(np.float64) ** 2).sum(-1) <= 3.0)   # (not the centres lifted or moved away)
            rows = rows[np.unique(np.linspace(0, len(rows) - 1, min(len(rows), 600)).astype(np.int64))]
            assert knn_rows_ok(got[b, rows], c["pts"][b, :L], c["ctr"][b, rows], r) == 0, (name, b)


def test_census_refuses_what_is_not_a_grid_workspace(ops):
    pts = dev(C.case("one_centre")["pts"])
    ws = ops.knn_grid(pts, dev([2048], torch.int32), 0.1)
    with pytest.raises(ValueError):
        ops.knn_grid_census(ws, 1, 4096)        # built for another N
    with pytest.raises(ValueError):
        ops.knn_grid_census(ws[:-1], 1, 2048)
