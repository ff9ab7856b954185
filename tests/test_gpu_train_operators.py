"""GPU: the decoder's training operators kernel by kernel at their tile and chunk edges -- csrc/offset_pairs.hip (walk, scan,
fill, gather, segment sum) and csrc/attention_train.hip (forward, delta, dQ, dK/dV) -- through their own entry points.

Section A compares bytes: pair lists, offsets, permutations, gathered rows and the ordered gradient sums against
tests/train_operators_restated.py (numpy float32, one rounding per operation; pinned on the CPU by
tests/test_train_operators_host.py) and against answers written out.  Section B uses the rule of test_gpu_decoder_train.py,
max |got - fp64| / max |fp64| <= max(3 e, FLOOR): fp64 is the dense formula on the device, e the error of the same formula in fp32
evaluated on the CPU (the shapes are small; the device's default fp32 GEMM backend is kept out of the bound, see that file's
docstring).  Observed errors and run times: profiles/train_operator_edges.md.
"""
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_operators_restated as R  # noqa: E402
from test_decoder_train_host import rel_err  # noqa: E402
from test_gpu_decoder_train import FLOOR, check  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
assert FLOOR == 1.4e-5


# ---- A. offset pairs -------------------------------------------------------------------------------------------------------

def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def hip_pairs(c):
    from deeppointmap_amd import ops
    return ops.offset_pairs(_t(c["xa"]), _t(c["xb"]), _t(c["pad_a"]), _t(c["pad_b"]), c["eps"])


def assert_pairs_equal(c, what):
    """triples, both offset arrays and the permutation equal the restatement's, element for element -> (pairs, restated).
    The offsets of the count entry point are compared first: the fill writes from them on, and it is not run from wrong ones."""
    from deeppointmap_amd import ops
    want = R.pair_list(**c)
    off = ops._offset_pairs_offsets(_t(c["xa"]), _t(c["xb"]), _t(c["pad_a"]), _t(c["pad_b"]), c["eps"])
    assert np.array_equal(off.cpu().numpy(), want[1]), f"{what}: the counted offsets differ"
    got = hip_pairs(c)
    assert [g.dtype for g in got] == [torch.int32] * 4, what
    for name, g, w in zip(("triples", "offsets_a", "offsets_b", "perm_b"), got, want):
        g = g.cpu().numpy()
        assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {name} differs"
    return got, want


@pytest.mark.parametrize("B,M,N", R.RAGGED_SHAPES)
def test_pairs_ragged(B, M, N):
    """A1: the second LDS chunk and its tail, M past one block and no multiple of it, pads on chunk boundaries"""
    _, want = assert_pairs_equal(R.ragged_case(B, M, N), f"ragged {B} x {M} x {N}")
    assert len(want[0]) >= 1


@pytest.mark.parametrize("name", sorted(R.lattice_cases()))
def test_pairs_lattice(name):
    """A2: the comparison at equality, one float32 either side, far from the origin, eps = 0, eps = inf, and the rounding of eps^2"""
    c, expected = R.lattice_cases()[name]
    got, _ = assert_pairs_equal(c, f"lattice {name}")
    assert got[0].cpu().tolist() == [list(t) for t in expected]


def test_pairs_nan():
    """A2: a NaN coordinate in one a row and one b column: no pair names them, every other pair stays"""
    clean, bad, ra, rb = R.nan_case()
    t0 = assert_pairs_equal(clean, "nan (clean)")[0][0].cpu().tolist()
    t1 = assert_pairs_equal(bad, "nan")[0][0].cpu().tolist()
    assert t1 == [t for t in t0 if (t[0], t[1]) != ra and (t[0], t[2]) != rb] and len(t1) < len(t0)


@pytest.mark.parametrize("where", R.SCAN_WHERE)
@pytest.mark.parametrize("rows", R.SCAN_ROWS)
def test_scan_offsets(rows, where):
    """A3: fewer rows than scan threads, a row count the block does not divide, everything in the first / the last row, nothing
    at all: the offsets of the count entry point alone against counts known by construction"""
    from deeppointmap_amd import ops
    c, counts = R.scan_case(rows, where)
    off = ops._offset_pairs_offsets(_t(c["xa"]), _t(c["xb"]), _t(c["pad_a"]), _t(c["pad_b"]), c["eps"])
    assert off.dtype == torch.int32 and off.cpu().tolist() == R.offsets_clipped(counts)


@pytest.mark.parametrize("where", R.SCAN_WHERE)
@pytest.mark.parametrize("rows", R.SCAN_ROWS)
def test_scan_lists(rows, where):
    """A3: the lists filled from those offsets; without any pair: K = 0, an empty list, all-zero offsets, and offset_pair_rows
    gives empty rows forward and exact zeros backward"""
    from deeppointmap_amd import ops
    c, _ = R.scan_case(rows, where)
    pairs, _ = assert_pairs_equal(c, f"scan {rows} {where}")
    if where != "none":
        return
    triples, off_a, off_b, perm_b = pairs
    assert tuple(triples.shape) == (0, 3) and perm_b.numel() == 0 and not off_a.any() and not off_b.any()
    E, N = 8, c["xb"].shape[2]
    x = torch.randn(rows, E, device=DEV).requires_grad_(True)
    y = torch.randn(N, E, device=DEV).requires_grad_(True)
    with torch.enable_grad():
        ox, oy = ops.offset_pair_rows(x, y, pairs, rows, N)
        gx, gy = torch.autograd.grad((ox, oy), (x, y), (torch.ones_like(ox), torch.ones_like(oy)))
    assert tuple(ox.shape) == (0, E) and tuple(oy.shape) == (0, E)
    for g, n in ((gx, rows), (gy, N)):
        assert tuple(g.shape) == (n, E) and not g.view(torch.int32).any(), "no pair: every gradient row is +0"


def test_scan_overflow():
    """A4: 46341 coincident points against 46341: 2 147 488 281 pairs do not fit an int32 -- the total reads -1, offset_pairs
    raises before it sizes a list; 46340 rows give 2 147 441 940 exactly; 46342 rows have a row offset past the range, clipped.
    No list is ever built (the second one would take 25 GB)."""
    from deeppointmap_amd import ops
    n = R.OVERFLOW_N
    z = torch.zeros(1, 3, n + 1, device=DEV)
    pad = torch.zeros(1, n + 1, dtype=torch.bool, device=DEV)
    pts = lambda m: (z[:, :, :m].contiguous(), pad[:, :m].contiguous())   # noqa: E731
    (xa, pa), (xb, pb) = pts(n), pts(n)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    off = ops._offset_pairs_offsets(xa, xb, pa, pb, 1.0)
    torch.cuda.synchronize()
    print(f"offset-pair count + scan over {n} x {n} coincident points: {1e3 * (time.perf_counter() - t0):.1f} ms")
    off = off.cpu().tolist()
    assert off[-1] == -1 and off == R.offsets_clipped([n] * n)
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with pytest.raises(ValueError, match="2\\^31"):
        ops.offset_pairs(xa, xb, pa, pb, 1.0)
    # two count arrays and two offset arrays of 46 341 int32, not 3 x 2^31 int32
    assert torch.cuda.max_memory_allocated() - base < 2 ** 22
    xa, pa = pts(n - 1)
    off = ops._offset_pairs_offsets(xa, xb, pa, pb, 1.0).cpu().tolist()
    assert off[-1] == 2_147_441_940 and off == R.offsets_clipped([n] * (n - 1))
    xa, pa = pts(n + 1)
    off = ops._offset_pairs_offsets(xa, xb, pa, pb, 1.0).cpu().tolist()
    assert off[-2:] == [R.INT32_MAX, -1] and off == R.offsets_clipped([n] * (n + 1))


@pytest.mark.parametrize("E", [4, 32, 260])
def test_gather(E):
    """A5: rows narrower and wider than a block, x and y column slices of wider buffers, a last block that is not full"""
    from deeppointmap_amd import ops
    c = R.nan_case()[0]
    B, _, M = c["xa"].shape
    N = c["xb"].shape[2]
    pairs = hip_pairs(c)
    t = pairs[0].long()
    K = t.shape[0]
    assert K > 0 and (K * E // 4) % 256 != 0
    gen = torch.Generator().manual_seed(E)
    bx, by = (torch.randn(B * n, E + 8, generator=gen).to(DEV) for n in (M, N))
    x, y = bx[:, 4:4 + E], by[:, 4:4 + E]
    assert x.stride(0) == E + 8 and not x.is_contiguous()
    ox, oy = ops.offset_pair_rows(x, y, pairs, M, N)
    assert ox.is_contiguous() and torch.equal(ox, x[t[:, 0] * M + t[:, 1]]) and torch.equal(oy, y[t[:, 0] * N + t[:, 2]])


@pytest.mark.parametrize("E", [4, 260, 512])
def test_segment_sum(E):
    """A6: the gradient rows added per token in the documented order -- a side: list order, b side: stably sorted by b -- byte for
    byte; rows with 0, 1 and 300 pairs, gradients of mixed magnitude so that another order changes bytes"""
    from deeppointmap_amd import ops
    c = R.hub_case()
    B, _, M = c["xa"].shape
    N = c["xb"].shape[2]
    pairs, (triples, off_a, off_b, perm_b) = assert_pairs_equal(c, "hub")
    K = len(triples)
    rng = np.random.default_rng(E)
    ga, gb = ((rng.standard_normal((K, E)) * 10.0 ** rng.integers(-4, 4, size=(K, E))).astype(np.float32) for _ in range(2))
    x = torch.zeros(B * M, E, device=DEV).requires_grad_(True)
    y = torch.zeros(B * N, E, device=DEV).requires_grad_(True)
    with torch.enable_grad():
        ox, oy = ops.offset_pair_rows(x, y, pairs, M, N)
        gx, gy = torch.autograd.grad((ox, oy), (x, y), (_t(ga), _t(gb)))
    t = triples.astype(np.int64)
    for name, got, g, off, perm, row in (("gx", gx, ga, off_a, np.arange(K), t[:, 0] * M + t[:, 1]),
                                         ("gy", gy, gb, off_b, perm_b, t[:, 0] * N + t[:, 2])):
        got = got.cpu().numpy()
        want = R.segment_sum_ordered(g, off, None if name == "gx" else perm)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), f"{name}: not the ordered float32 sum"
        n = np.diff(off)
        assert {0, 1, 300} <= set(n.tolist())
        assert not got[n == 0].view(np.int32).any(), f"{name}: a token without pairs gets +0"
        # the order matters: every token's rows taken backwards give other bytes
        back = np.concatenate([perm[off[r]:off[r + 1]][::-1] for r in range(len(n))])
        assert R.segment_sum_ordered(g, off, back).tobytes() != want.tobytes()
        w64 = np.zeros(got.shape, np.float64)
        np.add.at(w64, row, g.astype(np.float64))
        err = np.abs(got - w64).max() / np.abs(w64).max()
        print(f"segment sum {name} E={E}: {err:.2e} of max from the float64 sum")
        assert err <= 1e-6


# ---- B. training attention -------------------------------------------------------------------------------------------------

NAMES = ("out", "lse", "dq", "dk", "dv")


def _inputs(B, M, N, heads, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(B * n, 32 * heads, generator=gen) for n in (M, N, N, M)]   # q, k, v, dout on the CPU


def _ragged_mask(B, N):
    """ragged tails and one key inside, at least one live key per sequence; all-zero (but given) where N leaves no room"""
    km = torch.zeros(B, N, dtype=torch.uint8)
    for b in range(B):
        tail = (7 * (b + 1)) % max(1, N // 2)
        if tail:
            km[b, N - tail:] = 1
        if N >= 4:
            km[b, (3 * b + 1) % (N // 2)] = 1
    assert (km == 0).any(dim=1).all()
    return km


def hip_run(q, k, v, do, B, M, N, heads, km):
    """ops.attention_train under autograd + the forward's lse -> {out, lse, dq, dk, dv} on the device"""
    from deeppointmap_amd import ops
    km = None if km is None else km.to(DEV)
    leaves = [t.to(DEV).clone().requires_grad_(True) for t in (q, k, v)]
    with torch.enable_grad():
        out = ops.attention_train(*leaves, B, M, N, heads, km)
        dq, dk, dv = torch.autograd.grad(out, leaves, do.to(DEV))
    out2, lse = ops.attention_train_forward(*(t.detach() for t in leaves), B, M, N, heads, km)
    assert torch.equal(out2.view(torch.int32), out.detach().view(torch.int32))
    return dict(out=out.detach(), lse=lse, dq=dq, dk=dk, dv=dv)


def dense_run(q, k, v, do, B, M, N, heads, km, dtype, device):
    km = None if km is None else km.to(device)
    leaves = [t.to(device, dtype).requires_grad_(True) for t in (q, k, v)]
    with torch.enable_grad():
        out, lse = R.attention_dense(*leaves, B, M, N, heads, km, dtype)
        grads = torch.autograd.grad(out, leaves, do.to(device, dtype))
    return {n: t.detach().cpu().numpy() for n, t in zip(NAMES, (out, lse, *grads))}


def check_against_dense(what, got, q, k, v, do, B, M, N, heads, km):
    """every tensor of `got` within max(3 e, FLOOR) of the fp64 dense formula, e from the fp32 dense formula on the CPU"""
    r64 = dense_run(q, k, v, do, B, M, N, heads, km, torch.float64, DEV)
    r32 = dense_run(q, k, v, do, B, M, N, heads, km, torch.float32, "cpu")
    for n in NAMES:
        g = got[n].cpu().numpy()
        assert np.isfinite(g).all(), f"{what} {n}: not finite"
        check(f"train_ops {what} {n}", g, r64[n], rel_err(r32[n], r64[n]))
    return r64


def assert_same_bytes(a, b, what, names=NAMES):
    for n in names:
        assert a[n].shape == b[n].shape and torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), f"{what}: {n} differs"


SHAPES = [(1, 1, 1), (3, 15, 17), (2, 16, 64), (2, 17, 65), (3, 64, 63), (2, 65, 129), (1, 129, 1), (2, 1, 130)]


@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("heads", [8, 1, 3])
@pytest.mark.parametrize("B,M,N", SHAPES)
def test_attention_shapes(B, M, N, heads, mask):
    """B1: fewer rows than a wave's 16 and than a 64-row tile, one short of and one past a tile, on either side; 8, 1 and 3 heads"""
    q, k, v, do = _inputs(B, M, N, heads, 11)
    km = _ragged_mask(B, N) if mask else None
    got = hip_run(q, k, v, do, B, M, N, heads, km)
    assert_same_bytes(got, hip_run(q, k, v, do, B, M, N, heads, km), "two runs")
    check_against_dense(f"B1 {B}x{M}x{N} heads={heads} mask={mask}", got, q, k, v, do, B, M, N, heads, km)
    if mask:
        dead = km.bool().reshape(-1).to(DEV)
        assert not got["dk"][dead].any() and not got["dv"][dead].any()


def _tile_mask(kind, N):
    """B = 2; (a) first tile, (b) second tile, (c) last tile (the partial one at N = 130) all masked; (d) one live key: in a middle
    tile with every tile before and after it masked (in the partial last tile at N = 130), and in the first tile"""
    km = torch.zeros(2, N, dtype=torch.uint8)
    if kind == "a":
        km[:, :64] = 1
    elif kind == "b":
        km[:, 64:128] = 1
    elif kind == "c":
        km[:, 128:] = 1
    else:
        km[:] = 1
        km[0, 129 if N == 130 else 100] = 0
        km[1, 5] = 0
    return km


@pytest.mark.parametrize("kind", ["a", "b", "c", "d"])
@pytest.mark.parametrize("N", [192, 130])
def test_attention_whole_tile_masks(N, kind):
    """B2: a key tile without any live key before, between and after live ones (the empty running state: alpha = 0, reference 0)"""
    B, M, heads = 2, 70, 8
    q, k, v, do = _inputs(B, M, N, heads, 13)
    km = _tile_mask(kind, N)
    got = hip_run(q, k, v, do, B, M, N, heads, km)
    what = f"B2 N={N} ({kind})"
    r64 = check_against_dense(what, got, q, k, v, do, B, M, N, heads, km)
    dead = km.bool().reshape(-1).to(DEV)
    assert dead.any() and not got["dk"][dead].any() and not got["dv"][dead].any(), "masked keys get exactly zero dK and dV"
    # the same call on the live keys alone
    live = (~km.bool()).reshape(-1)
    L = int(live.sum()) // B
    assert (km == 0).sum(dim=1).tolist() == [L] * B
    red = hip_run(q, k[live], v[live], do, B, M, L, heads, None)
    r32 = dense_run(q, k, v, do, B, M, N, heads, km, torch.float32, "cpu")
    pick = lambda n, t: t[live.numpy()] if n in ("dk", "dv") else t   # noqa: E731
    for n in NAMES:
        check(f"train_ops {what} {n} against the live keys alone", pick(n, got[n].cpu().numpy()), red[n].cpu().numpy(),
              rel_err(pick(n, r32[n]), pick(n, r64[n])))
    if kind == "d":
        for b, key in enumerate((129 if N == 130 else 100, 5)):
            row = v[b * N + key].to(DEV)
            assert torch.equal(got["out"][b * M:(b + 1) * M], row.expand(M, 32 * heads)), "one live key: out is its V row, bit for bit"


@pytest.mark.parametrize("mask", [False, True])
def test_attention_large_scores(mask):
    """B3: scores up to 60: in half of the rows the running maximum rises with every key tile (each rescale matters), in the
    other half the first tile sets it and everything later underflows against it"""
    B, M, N, heads = 2, 40, 200, 8
    gen = torch.Generator().manual_seed(17)
    u = torch.nn.functional.normalize(torch.randn(heads, 32, generator=gen), dim=1).reshape(1, 32 * heads)
    a = (60.0 * 32 ** 0.5) ** 0.5
    ramp = (torch.arange(N, dtype=torch.float32) / N).repeat(B)[:, None]
    k = ramp * a * u + 0.05 * torch.randn(B * N, 32 * heads, generator=gen)
    sign = torch.where(torch.arange(M) < M // 2, 1.0, -1.0).repeat(B)[:, None]
    q = sign * a * u
    v, do = torch.randn(B * N, 32 * heads, generator=gen), torch.randn(B * M, 32 * heads, generator=gen)
    km = _ragged_mask(B, N) if mask else None
    got = hip_run(q, k, v, do, B, M, N, heads, km)
    r64 = check_against_dense(f"B3 mask={mask}", got, q, k, v, do, B, M, N, heads, km)
    assert 45.0 < float(r64["lse"].max()) < 75.0


def test_attention_batch_is_its_sequences():
    """B4: a batch of three equals its three single-sequence calls, bit for bit"""
    B, M, N, heads = 3, 65, 129, 8
    q, k, v, do = _inputs(B, M, N, heads, 19)
    km = _ragged_mask(B, N)
    got = hip_run(q, k, v, do, B, M, N, heads, km)
    one = [hip_run(q[b * M:(b + 1) * M], k[b * N:(b + 1) * N], v[b * N:(b + 1) * N], do[b * M:(b + 1) * M], 1, M, N, heads,
                   km[b:b + 1]) for b in range(B)]
    assert_same_bytes(got, {n: torch.cat([o[n] for o in one], dim=0) for n in NAMES}, "batch against single sequences")


def test_attention_layouts():
    """B5: q / k / v column slices of one (rows, 3 E) buffer, out and dout column slices of (rows, 2 E) buffers whose other
    columns hold NaN, handed to the backward as they are"""
    from deeppointmap_amd import ops
    B, M, N, heads = 2, 65, 65, 3
    E = 32 * heads
    q, k, v, do = (t.to(DEV) for t in _inputs(B, M, N, heads, 23))
    km = _ragged_mask(B, N).to(DEV)
    out, lse = ops.attention_train_forward(q, k, v, B, M, N, heads, km)
    want = ops.attention_train_backward(q, k, v, out, lse, do, B, M, N, heads, km)
    qkv = torch.cat([q, k, v], dim=1)
    qs, ks, vs = qkv[:, :E], qkv[:, E:2 * E], qkv[:, 2 * E:]
    ob, db = (torch.full((B * M, 2 * E), float("nan"), device=DEV) for _ in range(2))
    ob[:, E:], db[:, :E] = out, do
    o2, l2 = ops.attention_train_forward(qs, ks, vs, B, M, N, heads, km)
    assert torch.equal(o2, out) and torch.equal(l2, lse)
    got = ops.attention_train_backward(qs, ks, vs, ob[:, E:], lse, db[:, :E], B, M, N, heads, km)
    for n, g, w in zip(("dq", "dk", "dv"), got, want):
        assert torch.isfinite(g).all() and torch.equal(g, w), f"{n}: the strided call differs"
    r = dict(zip(NAMES, (out, lse, *got)))
    check_against_dense("B5", r, q.cpu(), k.cpu(), v.cpu(), do.cpu(), B, M, N, heads, km)


def test_attention_all_padding_sequence():
    """B6: a sequence whose keys are all padding violates the documented precondition: its out rows are NaN, its lse -inf, its dK
    and dV exactly zero -- and it leaves the other sequences of the batch untouched, bit for bit"""
    from deeppointmap_amd import ops
    B, M, N, heads = 3, 65, 70, 8
    q, k, v, do = _inputs(B, M, N, heads, 29)
    km = _ragged_mask(B, N)
    km[1] = 1
    leaves = [t.to(DEV).clone().requires_grad_(True) for t in (q, k, v)]
    with torch.enable_grad():
        out = ops.attention_train(*leaves, B, M, N, heads, km.to(DEV))
        dq, dk, dv = torch.autograd.grad(out, leaves, do.to(DEV))
    _, lse = ops.attention_train_forward(q.to(DEV), k.to(DEV), v.to(DEV), B, M, N, heads, km.to(DEV))
    got = dict(out=out.detach(), lse=lse, dq=dq, dk=dk, dv=dv)
    assert torch.isnan(got["out"][M:2 * M]).all() and (got["lse"][1] == float("-inf")).all()
    assert not got["dk"][N:2 * N].view(torch.int32).any() and not got["dv"][N:2 * N].view(torch.int32).any()
    rows = lambda t, n: torch.cat([t[:n], t[2 * n:]])   # noqa: E731
    two = hip_run(rows(q, M), rows(k, N), rows(v, N), rows(do, M), 2, M, N, heads, km[[0, 2]])
    others = dict(out=rows(got["out"], M), lse=got["lse"][[0, 2]], dq=rows(got["dq"], M), dk=rows(got["dk"], N), dv=rows(got["dv"], N))
    assert_same_bytes(others, two, "the sequences next to an all-padding one")
    assert all(torch.isfinite(t).all() for t in two.values())
