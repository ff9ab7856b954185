"""CPU: pins tests/group_train_cases.py, the cases of tests/test_gpu_group_train_edges.py.

The restated launch plan against the library's own workspace size; per width, the plan facts each shape exists for (if make_plan
changes, this says which shape stopped reaching its edge); and every case through the dense fp64 restatement
(tests/encoder_train_restated.py): the ungathered points really are unnamed, the constructed ties are exact and decide a good
share of the maxima, the dead cases are dead, and the identity the GPU test's exact dbeta assertion rests on holds."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_train_cases as G  # noqa: E402
from test_workspace_sizes_host import SHAPES as WS_SHAPES  # noqa: E402

ALL_SHAPES = G.PLAN_SHAPES + G.TINY_SHAPES + G.SHIPPED_SMALL + G.PERM_SHAPES + list(G.TIE_SHAPES.values()) + G.VARIANT_SHAPES


@pytest.fixture(scope="module")
def lib():
    from deeppointmap_amd import _lib
    from deeppointmap_amd.csrc import build
    build.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_plan_bytes_match_the_library(lib):
    f = lib.dpm_group_train_workspace_bytes
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int] * 5
    rows = [(B, N, S, K, Cout) for Cout, B, N, S, K in ALL_SHAPES] + list(WS_SHAPES["dpm_group_train_workspace_bytes"][1])
    assert len(WS_SHAPES["dpm_group_train_workspace_bytes"][1]) == 9
    for B, N, S, K, Cout in rows:
        assert G.plan(B, N, S, K, Cout).bytes == int(f(B, N, S, K, Cout)), (B, N, S, K, Cout)


def test_plan_table():
    """the table of the shapes' derivation, written out: (points, rpw, groups, ppw, waves) per PLAN_SHAPES row"""
    want = {32: (32775, 8, 4097, 2, 2049), 64: (8193, 4, 2049, 2, 1025), 128: (2049, 2, 1025, 2, 513), 256: (513, 1, 513, 2, 257),
            512: (259, 1, 259, 2, 130)}
    for Cout, B, N, S, K in G.PLAN_SHAPES:
        p = G.plan(B, N, S, K, Cout)
        assert (B * N, p.rpw, p.groups, p.ppw, p.waves) == want[Cout], (Cout, p)
    p = G.plan(3, 13, 5, 16, 32)
    assert (p.groups, p.ppw, p.waves, p.ragged) == (5, 1, 5, 7)


@pytest.mark.parametrize("Cout", [32, 64, 128, 256, 512])
def test_plan_edges_per_width(Cout):
    shapes = [s for s in G.PLAN_SHAPES if s[0] == Cout]
    assert shapes and {s[4] for s in shapes} == ({16, 32} if Cout == 32 else {16} if Cout == 512 else {32})
    for _, B, N, S, K in shapes:
        p = G.plan(B, N, S, K, Cout)
        assert p.ppw == 2 and p.dead_iterations == 1 and p.waves_mod4 != 0, p
        assert p.ragged != 0 or p.rpw == 1, p
        assert B in (3, 7) and N % 2 == 1 and (B * S) % 4 != 0 and (B * S) % 256 != 0
        if p.rpw > 1:
            assert any((b * N) % p.rpw for b in range(1, B)), "no wave straddles two frames"
    for _, B, N, S, K in [s for s in G.TINY_SHAPES if s[0] == Cout]:
        assert G.plan(B, N, S, K, Cout).ppw == 1
    assert all(G.plan(B, N, S, K, C).bytes > 0 for C, B, N, S, K in ALL_SHAPES)


def test_scan_edges_are_present():
    """n < 1024 (idle threads, chunk 1), n = 1024 m + 1, n = 1, and the plan shapes' n of no multiple of 1024"""
    ns = [B * N for _, B, N, _, _ in G.PLAN_SHAPES + G.TINY_SHAPES]
    assert 1 in ns and 1025 in ns and any(1 < n < 1024 for n in ns) and any(n > 1024 and n % 1024 == 1 for n in ns)
    assert all(n % 1024 for n in ns)


CASES = G.all_cases()


@pytest.mark.parametrize("name,t,kind,extra", CASES, ids=[c[0] for c in CASES])
def test_case_through_the_fp64_restatement(name, t, kind, extra):
    Cout, B, N, S, K = t["shape"]
    idx = t["idx"].long()
    assert idx.min() >= 0 and idx.max() < N and t["idx"].dtype == torch.int32
    assert torch.equal(t["dout"], t["dout"].round()) and t["dout"].abs().max() <= 4
    assert (t["gamma"] > 0).any() and (t["gamma"] < 0).any()
    # the never-gathered points
    nv = G.never(t)
    assert int(nv[0].sum()) == t["ungathered"] >= (N // 4 if N > 2 else 0) and (t["ungathered"] > 0) == (N > 2)
    named = torch.zeros(B, N, dtype=torch.bool)
    named[torch.arange(B).view(B, 1, 1).expand_as(idx), idx] = True
    if kind != "clamped":
        assert not (named & nv).any()
    max64, pts64, y64, g = G.restate(t, torch.float64, grads=True)
    assert torch.isfinite(y64).all() and all(torch.isfinite(x).all() for x in g)
    if kind == "poison":
        assert torch.isnan(t["P"][nv]).all() and torch.isnan(t["xyz"][nv]).all() and not torch.isnan(t["P"][~nv]).any()
    # the identity the exact dbeta assertion rests on: one winner per live (s, c), integer terms
    assert torch.equal(g[3], (t["dout"].double() * (max64 > 0)).sum((0, 1)))
    if kind == "tie":
        k1, k2 = extra
        assert torch.equal(y64[:, :, k1], y64[:, :, k2])
        assert all(len(set(idx[b].flatten().tolist())) == S * K for b in range(B))
        assert not torch.equal(idx[:, :, k1], idx[:, :, k2])
        live = max64 > 0
        won = ((y64[:, :, k1] == max64) & live).sum().item() / max(live.sum().item(), 1)
        assert won >= 0.25, f"the tied pair wins {won:.2f} of the live maxima"
        # nothing else ties with the winner: the first maximum is the only one besides slot k2
        assert ((y64 == max64.unsqueeze(2)).sum(2)[live & (y64[:, :, k1] == max64)] == 2).all()
    elif name.startswith(("distinct", "permuted")):
        assert all(len(set(row.tolist())) == K for row in idx.view(-1, K))
    if kind == "all_dead":
        assert y64.max() == 0 and max64.max() == 0 and all((x == 0).all() for x in g)
    elif kind == "dead_channel":
        assert max64[:, :, extra].max() == 0 and (max64 > 0).any()
    elif name.startswith("flat_rows"):
        assert (t["W_rel"] == 0).all() and torch.equal(t["P"], t["P"][:, :, :1].expand_as(t["P"]))
        assert torch.equal(y64, torch.relu(t["beta"].double()).expand_as(y64))
    else:
        assert (max64 > 0).any()


def test_variants_keep_what_they_do_not_construct():
    t = G.inputs(G.VARIANT_SHAPES[0])
    raw, clamped = G.out_of_range(t)
    N = t["shape"][2]
    bad = (raw["idx"] < 0) | (raw["idx"] >= N)
    assert 0 < int(bad.sum()) and {int(v) for v in raw["idx"][bad]} <= {-1, -7, N, N + 5}
    big = G.out_of_range(G.inputs(G.VARIANT_SHAPES[1]))[0]["idx"]
    assert {int(v) for v in big[(big < 0) | (big >= 683)]} == {-1, -7, 683, 688}
    assert torch.equal(raw["idx"][~bad], t["idx"][~bad]) and torch.equal(clamped["idx"][~bad], t["idx"][~bad])
    d = G.distinct(G.inputs(G.PERM_SHAPES[0]))
    p, perm = G.permute_slots(d)
    assert torch.equal(torch.gather(p["idx"], 2, perm), d["idx"]) and not torch.equal(p["idx"], d["idx"])
    f = G.frame(t, 1)
    assert f["shape"][1] == 1 and torch.equal(f["P"][0], t["P"][1]) and torch.equal(f["idx"][0], t["idx"][1])
    for k in ("xyz", "P", "idx", "beta"):
        assert torch.equal(G.inputs(G.VARIANT_SHAPES[0])[k], t[k]), "inputs are not a function of (shape, seed)"
