"""CPU: what tests/test_gpu_registration_tail.py rests on.

 * the restatement of the correspondence sets (tests/registration_tail_restated.py) is the oracle's correspondence_sets with
   the offset head taken out, and its round-recording copy of the Kabsch loop returns the oracle's bits;
 * every Kabsch case meets the condition it exists for (survivor counts per copy, the 256-entry round it crosses, a tie at
   the 64th place, weights above 0.5, ...), its offsets are nowhere near the cut, its covariance has full rank, and
 * MARGIN: every round of every case whose pose is asserted decides its inliers at least 1e-4 (relative) away from the cut
   mean + 3 std -- rounding level is below 1e-5 (oracle.dpm_oracle.solve_svd), so no GPU summation order can flip one.  The
   case 1000 m from the origin carries residual rounding of 1000 m coordinates (2^-24 * 1000 * a few terms ~ 2e-4 m against
   a cut near 2 m): it is held to 1e-2.  Cases without a defined cut (one survivor: std of one value; k = 1 with both
   copies: two mirror-image residuals, the cut sits on both) are listed by name and assert counts only on the GPU;
 * the fp64 restatements of the other kernels are the torch expressions they claim to be."""
import os
import sys
import types
import warnings

import pytest
import torch

from oracle import dpm_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import registration_tail_restated as RT  # noqa: E402

POSE = [n for n, s in RT.KABSCH.items() if s["check"] == "pose"]
NO_CUT_DEFINED = {"k1": "n_corr", "one_survivor": "counts", "empty": "empty"}


def _ref(name, num_iter=3):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # std() of one value: the reference's own NaN
        return RT.kabsch_reference(name, num_iter)


def test_constants_and_case_list():
    from deeppointmap_amd import ops
    assert RT.RES_HDR == ops.RES_HDR
    assert {n: s["check"] for n, s in RT.KABSCH.items() if s["check"] != "pose"} == NO_CUT_DEFINED
    assert {RT.KABSCH[n]["k"] for n in ("k1", "k20", "k127", "k128", "k129", "k640", "k2048", "k4096")} == \
        {1, 20, 127, 128, 129, 640, 2048, 4096}
    assert len({RT.KABSCH[n]["k"] for n in RT.BATCH + RT.BATCH_WITH_EMPTY}) == 1


@pytest.mark.parametrize("name", ["k20", "k640", "copy_a_cut", "empty"])
def test_correspondences_is_the_oracles_without_the_head(name, monkeypatch):
    c = RT.kabsch_case(name)
    k = c["k"]
    # the oracle runs its head on cat[xs, yd] and on cat[yd, xs]: mark the two directions in the features
    monkeypatch.setattr(O, "offset_head", lambda sd, f: c["off"][:k] if float(f[0, 0]) == 0.0 else c["off"][k:])
    cfg = types.SimpleNamespace(loss=types.SimpleNamespace(eps_offset=c["eps"]))
    src, dst, w = O.correspondence_sets(None, cfg, torch.zeros(k, 1), c["xyz_s"][c["si"].long()], torch.ones(k, 1),
                                        c["xyz_d"][c["di"].long()], c["conf"])
    s2, d2, w2, keep = RT.correspondences(c["off"], c["xyz_s"], c["xyz_d"], c["si"], c["di"], c["conf"], c["eps"])
    assert torch.equal(src, s2) and torch.equal(dst, d2) and torch.equal(w, w2) and int(keep.sum()) == w.numel()


@pytest.mark.parametrize("name", list(RT.KABSCH))
def test_case_is_what_it_claims(name):
    c = RT.kabsch_case(name)
    sp, k = RT.KABSCH[name], c["k"]
    assert tuple(c["off"].shape) == (2 * k, 3) and c["si"].dtype == torch.int32 and c["conf"].dtype == torch.float32
    assert bool((c["conf"][:-1] >= c["conf"][1:]).all()) and float(c["conf"].min()) >= 0     # a top-k output
    for idx, pts in ((c["si"], c["xyz_s"]), (c["di"], c["xyz_d"])):
        assert 0 <= int(idx.min()) and int(idx.max()) < pts.shape[0] and idx.unique().numel() == k
    # the cut: nowhere near eps (a fused multiply-add in the squared length cannot move an entry across)
    q = (c["off"].double() ** 2).sum(1) / c["eps"] ** 2
    assert float((q - 1).abs().min()) > 0.5
    keep = RT.offset_cut(c["off"], c["eps"])
    assert torch.equal(keep, q <= 1)
    nA, nB = int(keep[:k].sum()), int(keep[k:].sum())
    assert nA == (k if sp["keep_a"] is None else sp["keep_a"]) and nB == (k if sp["keep_b"] is None else sp["keep_b"])
    assert nA + nB == c["n"]
    if 2 * k > 256 and c["n"] > 256:     # survivors on both sides of the first 256-entry round: the running base is used
        assert bool(keep[:256].any()) and bool(keep[256:].any())
    # consistent with one rigid motion: the uncut pairs sit within noise + outliers of it
    R0, t0 = RT._motion()
    sh = sp["shift"]
    resid = ((c["xyz_s"][c["si"].long()].double() - sh) @ R0.T + t0 - (c["xyz_d"][c["di"].long()].double() - sh)).norm(dim=1)
    assert k < 20 or float(resid.median()) < 3 * sp["noise"]      # (a lone pair may be one of the displaced tenth)


def test_case_conditions():
    n = {name: RT.kabsch_case(name)["n"] for name in RT.KABSCH}
    assert n["nothing_cut"] == 2 * RT.KABSCH["nothing_cut"]["k"]
    assert RT.KABSCH["copy_a_cut"]["keep_a"] == 0 and RT.KABSCH["copy_b_cut"]["keep_b"] == 0
    assert n["under64"] < 64 and 30 <= n["under64"]
    assert n["under30"] < 30 and _ref("under30")["iterations"] == 1
    assert n["one_survivor"] == 1 and n["empty"] == 0 and n["k1"] == 2
    assert len({n[b] for b in RT.BATCH}) == 3
    for name in RT.TIED:
        assert RT.straddling_tie(_ref(name)["w"]), name
    for name in ("tie6_wave", "tie40_wave"):     # min(64, n) * 64 > n: the wave's nth-element replay
        assert 64 < n[name] < 4096
        assert float(_ref(name)["w"].sort(descending=True).values[63]) <= 0.5
    for name in ("tie6_heap", "tie40_heap"):     # ... <= n: the heap replay
        assert n[name] >= 4096
        assert float(_ref(name)["w"].sort(descending=True).values[63]) <= 0.5
    assert float(_ref("high_tied")["w"].sort(descending=True).values[64]) > 0.5      # tied, and the 0.5 rule decides
    w = _ref("high")["w"]
    assert int((w > 0.5).sum()) > 64 and int((w <= 0.5).sum()) > 64
    for name in POSE:                            # direct mode is compared on the untied cases: conf distinct
        if name not in RT.TIED:
            assert RT.kabsch_case(name)["conf"].unique().numel() == RT.KABSCH[name]["k"], name
    assert not RT.straddling_tie(_ref("nothing_cut")["w"])
    # the loop's exits all occur: round limit, fewer than 30 inliers
    its = {name: _ref(name)["iterations"] for name in POSE}
    assert 3 in its.values() and 1 in its.values()
    assert _ref("one_survivor")["iterations"] == 1 and int(_ref("one_survivor")["inl"].sum()) == 0
    assert _ref("k1")["iterations"] == 1


@pytest.mark.parametrize("num_iter", [3, 1])
@pytest.mark.parametrize("name", [n for n in RT.KABSCH if n != "empty"])
def test_rounds_copy_returns_the_oracles_bits(name, num_iter):
    r = _ref(name, num_iter)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        R, T, inl, rmse, masks = RT.solve_svd_rounds(r["w"], r["src"], r["dst"], num_iter=num_iter)
    assert torch.equal(R, r["R"]) and torch.equal(T, r["T"]) and torch.equal(inl, r["inl"])
    assert rmse == r["rmse"] or (rmse != rmse and r["rmse"] != r["rmse"])
    assert len(masks) - 1 == len(r["margins"]) and torch.equal(masks[-1], inl)
    assert int(masks[0].sum()) >= min(64, r["w"].numel())


@pytest.mark.parametrize("name", POSE)
def test_margin_and_rank(name):
    """no case is excused: every round of every pose-asserting case stays clear of its inlier cut"""
    r = _ref(name)
    need = 1e-2 if RT.KABSCH[name]["shift"] else 1e-4
    assert len(r["margins"]) == r["iterations"] and min(r["margins"]) >= need, (name, r["margins"])
    assert _ref(name, 1)["margins"][0] == r["margins"][0]          # the one-round run decides on the same residuals
    R64, T64, rmse64, sv = RT.solve_svd64(r["w"], r["src"], r["dst"], r["masks"])
    assert float(sv[2] / sv[0]) > 1e-3, (name, sv)                 # R = V U^T is well defined
    eT, eR, er = float((r["T"].double() - T64).norm()), _angle(r["R"], R64), abs(r["rmse"] - rmse64)
    print(f"{name}: n {r['w'].numel()}, inliers {int(r['inl'].sum())}, rounds {r['iterations']}, margins "
          f"{['%.1e' % m for m in r['margins']]}, oracle fp32 vs fp64: T {eT:.2e} m, R {eR:.2e} rad, rmse {er:.2e}")
    if not RT.KABSCH[name]["shift"]:   # at this coordinate scale the reference is within the bounds the GPU tests grant
        assert eT < 2e-5 and eR < 1e-5 and er < 2e-5


def _angle(Ra, Rb):
    M = Ra.double().T @ Rb.double()
    return float(torch.atan2(torch.linalg.norm(M - M.T) / (2 * 2 ** 0.5), (torch.trace(M) - 1) / 2))


def test_gather_pairs_cases():
    for shape in RT.GATHER_PAIRS:
        B, M, N, E, k = shape
        x, y, flat = RT.gather_pairs_case(*shape)
        assert flat.dtype == torch.int32 and int(flat.min()) == 0 and int(flat.max()) == M * N - 1
        assert k < 4 or flat[0].unique().numel() < k                       # a repeat
        X, si, di = RT.gather_pairs(x, y, flat)
        assert tuple(X.shape) == (B, 2 * k, 2 * E) and int(si.max()) == M - 1 and int(di.max()) == N - 1
        b, p = B - 1, k // 2
        assert torch.equal(X[b, p], torch.cat([x[b, si[b, p]], y[b, di[b, p]]]))
        assert torch.equal(X[b, k + p], torch.cat([y[b, di[b, p]], x[b, si[b, p]]]))


@pytest.mark.parametrize("name", list(RT.MAP_TILE))
def test_map_tile_cases(name):
    kp, poses, centre, sel = RT.map_tile_case(name)
    n, C, S, _ = RT.MAP_TILE[name]
    K = n if sel is None else len(sel)
    t64, t32 = RT.map_tile64(kp, poses, centre, sel), RT.map_tile32(kp, poses, centre, sel)
    assert tuple(t64.shape) == (C, K * S) == tuple(t32.shape)
    assert torch.equal(t32[:-3], t64[:-3].float())                          # feature rows: copies
    e = float((t32[-3:].double() - t64[-3:]).abs().max())
    assert float(poses[:, :3, 3].norm(dim=1).min()) > 300 and float(t64[-3:].abs().max()) < 200   # large in, small out
    assert any(torch.equal(centre, p) for p in poses)
    assert e < 1e-3
    print(f"map tile {name}: oracle fp32 vs fp64 {e:.2e} m")
    if sel is not None and name == "repeat_back":
        assert len(set(sel)) < len(sel) and sel != sorted(sel)


def test_small_restatements():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(5, 255, generator=g)
    assert float((RT.l2_normalize64(x) - torch.nn.functional.normalize(x.double(), dim=-1)).abs().max()) < 1e-15
    z = torch.zeros(2, 8)
    z[1, 3] = 1e-20
    want = RT.l2_normalize64(z)
    assert float(want[0].abs().max()) == 0 and float(want[1, 3]) == float(z[1, 3]) / 1e-12   # both rows: x / 1e-12
    assert RT.l2_bound(1) == 9 * 2.0 ** -24 and RT.l2_bound(256) == 12 * 2.0 ** -24
    lv = RT.nested_levels(torch.randn(4, 300, 3, generator=g), torch.tensor([0, 1, 256, 300], dtype=torch.int32), [300, 257, 256, 1])
    assert [int(v) for v in lv[1][2]] == [0, 1, 256, 257] and lv[2][0][2].tolist() == list(range(256))
    assert lv[3][0].flatten().tolist() == [-1, 0, 0, 0] and lv[0][0][1].tolist() == [0] + [-1] * 299
    coor, feat, pad, desc = RT.emit_descriptors(torch.randn(2, 33, 3, generator=g), torch.randn(2, 33, 29, generator=g),
                                                torch.tensor([0, 33], dtype=torch.int32), 0.5)
    assert bool(pad[0].all()) and not bool(pad[1].any()) and tuple(desc.shape) == (2, 32, 33)
    assert RT.emit_descriptors(torch.randn(1, 1, 3), torch.randn(1, 1, 1), torch.tensor([1], dtype=torch.int32), 0.0)[3] is None
    assert torch.equal(RT.dim_t(256), 10000 ** (2 * torch.div(torch.arange(84, dtype=torch.float32), 2, rounding_mode="trunc") / 84))
    assert float(RT.mean_rows_bound(torch.ones(1, 1, 1))) == 0.0
