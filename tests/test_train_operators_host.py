"""CPU only: pins tests/train_operators_restated.py, the comparator of tests/test_gpu_train_operators.py, so that it cannot be
wrong together with a kernel: known answers written out, torch.nonzero of the dense float32 mask, and mutants of the pair list
and of the ordered sum that at least one case must tell from the restatement."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_operators_restated as R  # noqa: E402

F32 = np.float32


def _cases():
    """every case of section A that has a pair list: name -> case"""
    out = {f"ragged{s}": R.ragged_case(*s) for s in R.RAGGED_SHAPES}
    out.update({f"lattice_{k}": c for k, (c, _) in R.lattice_cases().items()})
    clean, bad, _, _ = R.nan_case()
    out["nan_clean"], out["nan"] = clean, bad
    out.update({f"scan{r}_{w}": R.scan_case(r, w)[0] for r in R.SCAN_ROWS for w in R.SCAN_WHERE})
    out["hub"] = R.hub_case()
    return out


CASES = _cases()


def variant(xa, xb, pad_a, pad_b, eps, lt=False, ignore_pad_b=False, b_major=False, eps_f32=False):
    """the pair list written a second time, with loops, and with the four mistakes it must be told from as switches"""
    eps2 = F32(F32(eps) * F32(eps)) if eps_f32 else F32(np.float64(eps) * np.float64(eps))
    B, _, M = xa.shape
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            rows = []
            for i in range(M):
                if pad_a[b, i]:
                    continue
                dx, dy, dz = xa[b, 0, i] - xb[b, 0], xa[b, 1, i] - xb[b, 1], xa[b, 2, i] - xb[b, 2]
                d2 = (dx * dx + dy * dy) + dz * dz
                hit = (d2 < eps2) if lt else (d2 <= eps2)
                if not ignore_pad_b:
                    hit = hit & ~pad_b[b]
                rows += [(b, i, int(j)) for j in np.nonzero(hit)[0]]
            out += sorted(rows, key=lambda t: (t[2], t[1])) if b_major else rows
    return np.array(out, np.int32).reshape(-1, 3)


@pytest.mark.parametrize("name", sorted(CASES))
def test_pair_list_equals_dense_nonzero(name):
    c = CASES[name]
    xa, xb = torch.from_numpy(c["xa"]), torch.from_numpy(c["xb"])
    d = xa.unsqueeze(3) - xb.unsqueeze(2)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    eps2 = torch.tensor(float(c["eps"]), dtype=torch.float64).square().to(torch.float32)
    want = torch.nonzero((d2 <= eps2) & ~torch.from_numpy(c["pad_a"]).unsqueeze(2) & ~torch.from_numpy(c["pad_b"]).unsqueeze(1))
    triples, off_a, off_b, perm_b = R.pair_list(**c)
    assert triples.dtype == np.int32 and np.array_equal(triples, want.numpy())
    assert np.array_equal(triples, variant(**c))
    B, _, M = c["xa"].shape
    N = c["xb"].shape[2]
    t = triples.astype(np.int64)
    assert np.array_equal(np.diff(off_a), np.bincount(t[:, 0] * M + t[:, 1], minlength=B * M)) and off_a[0] == 0
    assert np.array_equal(np.diff(off_b), np.bincount(t[:, 0] * N + t[:, 2], minlength=B * N)) and off_b[0] == 0
    key = (t[:, 0] * N + t[:, 2])[perm_b]
    assert np.all(np.diff(key) >= 0) and np.all(np.diff(perm_b)[np.diff(key) == 0] > 0)
    assert sorted(perm_b.tolist()) == list(range(len(t)))


def test_ragged_cases_are_what_they_claim():
    """every shape has pairs, a handful per row; pads exist on both sides and every padded token would pair if its pad were
    ignored; the chunk-edge columns are padded with a live a point exactly on them"""
    for s in R.RAGGED_SHAPES:
        c = R.ragged_case(*s)
        B, M, N = s
        K = len(R.pair_list(**c)[0])
        live_rows = int((~c["pad_a"]).sum())
        assert 1 <= K and K <= 12 * live_rows, (s, K)
        if M > 16:
            assert c["pad_a"].any() and c["pad_b"].any() and not c["pad_a"][0, -1]
            none = np.zeros_like(c["pad_a"]), np.zeros_like(c["pad_b"])
            t = R.pair_list(c["xa"], c["xb"], *none, c["eps"])[0]
            assert set(map(tuple, np.argwhere(c["pad_a"]))) <= {(b, i) for b, i, _ in t.tolist()}
            assert set(map(tuple, np.argwhere(c["pad_b"]))) <= {(b, j) for b, _, j in t.tolist()}
        if N in R.CHUNK_EDGE_N:
            for b in range(B):
                for i, j in enumerate((255, 256, N - 1)):
                    assert c["pad_b"][b, j] and not c["pad_a"][b, i] and np.array_equal(c["xa"][b, :, i], c["xb"][b, :, j])


def test_lattice_known_answers():
    cases = R.lattice_cases()
    counts = {k: len(R.pair_list(**c)[0]) for k, (c, _) in cases.items()}
    assert counts == {"near": 2, "far": 2, "eps_zero": 1, "eps_inf": 12 * 9 + 8 * 6, "eps_0.1": 0, "eps_0.7": 1}
    for k, (c, want) in cases.items():
        assert R.pair_list(**c)[0].tolist() == [list(t) for t in want], k
    for k in ("near", "far"):
        c = cases[k][0]
        d = (c["xb"].astype(np.float64) - c["xa"].astype(np.float64))[0]          # exact differences
        assert d[0].tolist() == [0.75] * 3 and d[2].tolist() == [0.0] * 3
        up, down = (2.0 ** -23, 2.0 ** -24) if k == "near" else (2.0 ** -11, 2.0 ** -11)
        assert d[1].tolist() == [1.0, 1.0 + up, 1.0 - down]
    c = cases["eps_zero"][0]
    assert c["xb"][0, 0, 1] == np.nextafter(F32(5), F32(6)) and c["eps"] == 0.0


def test_nan_rows_name_no_pair_and_change_nothing_else():
    clean, bad, ra, rb = R.nan_case()
    t0, t1 = R.pair_list(**clean)[0].tolist(), R.pair_list(**bad)[0].tolist()
    named = lambda t: (t[0], t[1]) == ra or (t[0], t[2]) == rb   # noqa: E731
    assert any((t[0], t[1]) == ra for t in t0) and any((t[0], t[2]) == rb for t in t0)
    assert t1 == [t for t in t0 if not named(t)] and len(t1) < len(t0)


def test_scan_case_counts_are_the_constructed_ones():
    for r in R.SCAN_ROWS:
        for w in R.SCAN_WHERE:
            c, counts = R.scan_case(r, w)
            assert R.pair_list(**c)[1].tolist() == R.offsets_clipped(counts), (r, w)
            if w != "mixed":
                assert sum(counts) == (0 if w == "none" else 4) and (w != "last" or counts[-1] == 4)
    assert R.scan_case(1000, "mixed")[1][:6] == [3, 1, 4, 2, 0, 3]


def test_hub_case_has_rows_with_0_1_and_300_pairs():
    c = R.hub_case()
    _, off_a, off_b, _ = R.pair_list(**c)
    for off in (off_a, off_b):
        assert {0, 1, 300} <= set(np.diff(off).tolist())
    assert np.diff(off_a)[0] == 300 and np.diff(off_b)[300] == 300


MUTANTS = {
    "lt": ("lattice_near", "lattice_far", "lattice_eps_zero", "lattice_eps_0.7"),   # d2 == eps2 exactly
    "ignore_pad_b": ("ragged(2, 255, 257)", "ragged(2, 256, 513)", "ragged(2, 300, 700)", "hub"),
    "b_major": ("ragged(1, 600, 256)", "ragged(3, 257, 255)"),
    "eps_f32": ("lattice_eps_0.1", "lattice_eps_0.7"),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_pair_list_mutant_is_rejected(mutant):
    """each mistake changes the list of the cases built against it -- and the unmutated second writing changes none"""
    for name in MUTANTS[mutant]:
        c = CASES[name]
        want = R.pair_list(**c)[0]
        assert np.array_equal(variant(**c), want), name
        assert not np.array_equal(variant(**c, **{mutant: True}), want), (mutant, name)


def test_eps_rounding_cases_split_both_ways():
    for name, keeps in (("lattice_eps_0.1", False), ("lattice_eps_0.7", True)):
        c = CASES[name]
        d = c["xa"][0, :, 0] - c["xb"][0, :, 0]
        d2 = F32(F32(F32(d[0] * d[0]) + F32(d[1] * d[1])) + F32(d[2] * d[2]))
        true2, mut2 = F32(np.float64(c["eps"]) ** 2), F32(F32(c["eps"]) * F32(c["eps"]))
        assert d2 == max(true2, mut2) and true2 != mut2 and (true2 > mut2) == keeps
        assert len(R.pair_list(**c)[0]) == int(keeps) and len(variant(**c, eps_f32=True)) == int(not keeps)
    assert F32(np.float64(0.3) * np.float64(0.3)) == F32(F32(0.3) * F32(0.3))     # why the issue's example eps is not used


def test_offsets_clipped():
    assert R.offsets_clipped([]) == [0]
    assert R.offsets_clipped([2, 0, 3]) == [0, 2, 2, 5]
    n = R.OVERFLOW_N
    assert n * n == 2_147_488_281 and (n - 1) * n == 2_147_441_940 and R.INT32_MAX == 2_147_483_647
    full = R.offsets_clipped([n] * n)
    assert len(full) == n + 1 and full[-1] == -1 and full[-2] == (n - 1) * n and full[1] == n
    assert all(full[r] == r * n for r in (0, 1, 255, 256, n - 1))
    fits = R.offsets_clipped([n] * (n - 1))
    assert fits[-1] == 2_147_441_940
    over = R.offsets_clipped([n] * (n + 1))      # one more row: its offset is past the range and clipped, the total is -1
    assert over[-1] == -1 and over[-2] == R.INT32_MAX and over[-3] == (n - 1) * n
    assert R.offsets_clipped([R.INT32_MAX, 0, 1]) == [0, R.INT32_MAX, R.INT32_MAX, -1]
    assert R.offsets_clipped([R.INT32_MAX]) == [0, R.INT32_MAX]


def test_segment_sum_order_decides_the_bytes():
    big = F32(1e8)
    g = np.array([[big, 1], [1, big], [-big, -big], [0.5, -0.0]], F32)
    off = [0, 3, 3, 4]
    fwd = R.segment_sum_ordered(g, off, None)
    # column 0: (1e8 + 1) - 1e8 = 0 in float32 (1 is below half the spacing of 8 at 1e8); column 1: (1 + 1e8) - 1e8 = 0
    assert fwd.tolist() == [[0.0, 0.0], [0.0, 0.0], [0.5, 0.0]]
    assert not np.signbit(fwd[1]).any() and not np.signbit(fwd[2, 1])            # an empty row is +0, and +0 + -0 = +0
    rev = R.segment_sum_ordered(g, off, [2, 1, 0, 3])                                # (-1e8 + 1) + 1e8 = 0; (-1e8 + 1e8) + 1 = 1
    assert rev.tolist() == [[0.0, 1.0], [0.0, 0.0], [0.5, 0.0]]
    assert fwd.tobytes() != rev.tobytes()
    mid = R.segment_sum_ordered(g, off, [0, 2, 1, 3])                                # (1e8 - 1e8) + 1 = 1; (1 - 1e8) + 1e8 = 0
    assert mid.tolist() == [[1.0, 0.0], [0.0, 0.0], [0.5, 0.0]]
    # a mixed-magnitude draw like the GPU test's: reversing the order of a 300-term row changes bytes
    rng = np.random.default_rng(0)
    g = (rng.standard_normal((300, 8)) * 10.0 ** rng.integers(-4, 4, size=(300, 8))).astype(F32)
    a = R.segment_sum_ordered(g, [0, 300], None)
    b = R.segment_sum_ordered(g, [0, 300], np.arange(299, -1, -1))
    assert a.tobytes() != b.tobytes()
    want = g.astype(np.float64).sum(0)
    assert np.abs(a[0] - want).max() <= 1e-6 * np.abs(want).max()


def test_attention_dense_is_softmax_attention():
    """against a per-head loop written out, heads as a parameter, mask and lse included"""
    gen = torch.Generator().manual_seed(0)
    B, M, N, heads = 2, 5, 7, 3
    q, k, v = (torch.randn(B * n, 32 * heads, generator=gen, dtype=torch.float64) for n in (M, N, N))
    mask = torch.zeros(B, N, dtype=torch.uint8)
    mask[0, 5:] = 1
    mask[1, 2] = 1
    out, lse = R.attention_dense(q, k, v, B, M, N, heads, mask, torch.float64)
    assert out.shape == (B * M, 96) and lse.shape == (B, heads, M)
    for b in range(B):
        live = [n for n in range(N) if not mask[b, n]]
        for h in range(heads):
            c = slice(32 * h, 32 * h + 32)
            for m in range(M):
                s = torch.stack([q[b * M + m, c] @ k[b * N + n, c] for n in live]) / 32 ** 0.5
                p = torch.exp(s - s.max())
                want = sum(w * v[b * N + n, c] for w, n in zip(p / p.sum(), live))
                assert torch.allclose(out[b * M + m, c], want, rtol=1e-12, atol=1e-14)
                assert abs(float(lse[b, h, m]) - float(s.max() + p.sum().log())) < 1e-12
    o32, _ = R.attention_dense(q.float(), k.float(), v.float(), B, M, N, heads, None, torch.float32)
    assert o32.dtype == torch.float32
