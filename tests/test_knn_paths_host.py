"""CPU: pins tests/knn_paths_cases.py, the cases of tests/test_gpu_knn_paths.py, by the reference's arithmetic alone
(tests/knn_paths_restated.py and the oracle): every case holds at least the rows it is named for of each exit of the hybrid
neighbour search, the tie-queue cases hold more tied rows than the queue, the by_mark case more failed rows than the todo list,
and every frame's grid layout sits away from the thresholds at which a float rounding could flip it.  Together the cases name every
exit: the last test is the list.  The counts are printed (pytest -s) -- profiles/knn_paths.md quotes them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_paths_cases as C  # noqa: E402
import knn_paths_restated as R  # noqa: E402


@pytest.mark.parametrize("name", C.NAMES)
def test_case_reaches_the_exits_it_is_named_for(name):
    c, ref = C.case(name), C.reference(name)
    B, N, _ = c["pts"].shape
    S = c["ctr"].shape[1]
    assert N <= 8192 and S <= 8192 and 1 <= c["K"] <= R.KMAX
    assert c["path"] == ("grid" if N >= R.GRID_MIN_N else "brute") and c["regime"] == ("heap" if 64 * c["K"] <= N else "nth")
    n_tie = int(ref["tie"].sum())
    print(f"{name}: {c['path']} / {c['regime']}, B = {B}, N = {N}, S = {S}, K = {c['K']}, r = {c['r']}; tie rows {n_tie}, "
          f"rows whose filler differs from the oracle's {ref['filler_differs']}; " +
          ", ".join(f"{k} {v}" for k, v in ref["counts"].items() if v))
    assert n_tie >= c["ties"], (n_tie, c["ties"])
    for key, least in c["need"].items():
        assert ref["counts"][key] >= least, (key, ref["counts"][key], least)
    if c["fallback"] or name == "tieq_overflow_heap":
        assert n_tie > R.TIE_CAP + 500, n_tie          # the oracle alone produces more tied rows than the queue holds
    if c["by_mark"]:
        assert S > N and ref["counts"]["todo_min"] > B * N + 100, ref["counts"]["todo_min"]
    if c["fp64"]:
        assert float((c["pts"].astype(np.float64) ** 2).sum(-1).max()) <= 3.0
    # the oracle's rows are what the specification says wherever no filler hangs on a tied minimum
    same = (ref["spec"] == np.sort(ref["want"], axis=2)).all(2)
    assert (same | (ref["min_tied"] & ((ref["dk"] > np.float32(c["r"] * c["r"])).any(2)))).all()


@pytest.mark.parametrize("name", C.NAMES)
def test_oracle_distances_are_the_fma_chain(name):
    """the oracle's matmul, called with whole row groups of centres (knn_paths_restated.pad_rows), against the fma chain the
    kernels are specified as, bit for bit: the first and the last 256 centres of every frame against all its points.  Where
    this fails the host BLAS rounds differently and no GPU comparison of tied rows means anything."""
    c = C.case(name)
    for b in range(c["pts"].shape[0]):
        L, S = c["lens"][b], c["ctr"].shape[1]
        for rows in {(0, min(S, 256)), (max(S - 256, 0), S)}:
            ctr = c["ctr"][b, rows[0]:rows[1]]
            got, want = R.expanded(ctr, c["pts"][b, :L]), R.chain_sqdist(ctr, c["pts"][b, :L])
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, b, rows, int((got != want).sum()))


@pytest.mark.parametrize("name", [n for n in C.NAMES if C.case(n)["path"] == "grid"])
def test_grid_layout_is_the_intended_one_and_robust(name):
    c, ref = C.case(name), C.reference(name)
    for b, hd in enumerate(ref["headers"]):
        rel, frac = R.header_margin(hd)
        print(f"{name}[{b}]: g {hd['g']}, H {hd['H']}, h {hd['h']}, edge {float(hd['cs']):.6g}, err2 {float(hd['err2']):.4g}, "
              f"layout margin {rel:.3f}, ext / edge {float(hd['cells']):.5f}")
        assert rel >= 0.03, (b, rel, hd["compared"])          # a few percent: no float rounding flips H
        # g = int(ext / edge) + 1: ext / edge keeps 1e-4 (a thousand float32 roundings) from an integer -- below 1/2 it
        # cannot reach one at all (ext > 0)
        assert frac is None or float(hd["cells"]) < 0.5 or frac >= 1e-4 * max(1.0, float(hd["cells"])), (b, frac)
        assert 1 <= hd["g"] <= R.GDIM and (hd["H"], hd["h"]) in ((1, 1), (2, 1), (3, 2))
    if c["header"] is not None:
        g, H, h = c["header"]
        hd = ref["headers"][0]
        assert (hd["H"], hd["h"]) == (H, h) and (g is None or hd["g"] == g), (hd["g"], hd["H"], hd["h"])
    if name == "gdim_floor":
        hd = ref["headers"][0]
        assert float(hd["cs"]) == float(hd["floor_cs"]) and abs(float(hd["cs"]) - 100.0 / 127.0) < 1e-3 and hd["g"] == R.GDIM


def test_every_exit_is_named_by_a_case():
    """the list of the issue: which case pins which exit (the GPU test asserts the census of exactly these cases)"""
    named = {
        "knn_tie_nth_kernel (grid path, 64 K > N)": [n for n in C.NAMES if C.case(n)["path"] == "grid" and C.case(n)["regime"] == "nth"
                                                     and C.case(n)["ties"] >= 20 and not C.case(n)["fallback"]],
        "nth_select_exact on the brute path": [n for n in C.NAMES if C.case(n)["path"] == "brute" and C.case(n)["regime"] == "nth"
                                               and C.case(n)["ties"] >= 15],
        "tie queue overflow, heap regime": ["tieq_overflow_heap"],
        "tie queue overflow, nth regime": [n for n in C.NAMES if C.case(n)["fallback"]],
        "by_mark": [n for n in C.NAMES if C.case(n)["by_mark"]],
        "gdim floor": [n for n in C.NAMES if C.case(n)["header"] is not None and C.case(n)["header"][0] == R.GDIM],
    }
    for key in ("outside", "overflow", "empty", "border_fail", "border_pass", "widened", "full", "inner", "slots5", "slots10", "slots15",
                "slots20"):
        named[key] = [n for n in C.NAMES if C.case(n)["need"].get(key, 0) > 0]
    for layout in ((1, 1), (2, 1), (3, 2)):
        named[f"layout H, h = {layout}"] = [n for n in C.NAMES if C.case(n)["header"] is not None and C.case(n)["header"][1:] == layout]
    for what, names in named.items():
        print(f"{what}: {', '.join(names)}")
        assert names, what
    shapes = [(C.case(n)["ctr"].shape[1], C.case(n)["K"]) for n in C.NAMES]
    assert any(S == 1 for S, _ in shapes) and any(S % 16 for S, _ in shapes if S > 1)
    assert any(K == 1 for _, K in shapes) and any(K == R.KMAX for _, K in shapes)
    for path in ("grid", "brute"):
        for regime in ("heap", "nth"):
            rag = [C.case(n) for n in C.NAMES if n.startswith("ragged") and C.case(n)["path"] == path and C.case(n)["regime"] == regime]
            assert rag and all(c["lens"][1:] == [c["K"] + 1, c["K"], c["K"] - 1, 1] for c in rag), (path, regime)
