"""GPU: the encoder's grouping training operator (csrc/group_train.hip, ops.group_train) at the edges of its launch plan, its
lane layout, its single-block scan and its tie rule, and on constructed inputs with an exact answer.

Cases: tests/group_train_cases.py, pinned on the CPU by tests/test_group_train_cases_host.py.  Reference: the dense plain-torch
restatement (tests/encoder_train_restated.py) in fp64 on the device, for gradients with the kernel's routes forced.  Bounds are
those of tests/test_gpu_encoder_train.py and nothing else: assert_features_close for the forward, the gap of the chosen
neighbour to the fp64 maximum, and `check` = max(3 e, FLOOR) for every gradient, e the dense fp32 restatement's error on the
device against the same fp64 run.  Everything else here is an exact statement: bytes, integers, zeros.
profiles/encoder_train_accuracy.md has the observed errors.
"""
import functools
import os
import sys

import pytest
import torch

from conftest import FEATURE_TOL, assert_features_close

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import group_train_cases as G  # noqa: E402
from test_encoder_train_host import rel_err  # noqa: E402
from test_gpu_encoder_train import check, note  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("dP", "dW_rel", "dgamma", "dbeta")
ids = G.shape_id


def hip(t, dout="given"):
    """ops.group_train on a case, forward and backward -> (out, slots, dP, dW_rel, dgamma, dbeta) on the device"""
    from deeppointmap_amd import ops
    d = {k: v.to(DEV) for k, v in t.items() if torch.is_tensor(v)}
    leaves = [d[k].clone().requires_grad_(True) for k in ("P", "W_rel", "gamma", "beta")]
    keep = []
    with torch.enable_grad():
        out = ops.group_train(leaves[0], d["xyz"], d["centers"], d["idx"], leaves[1], leaves[2], leaves[3], t["radius"], layer="edges",
                              keep_slots=keep)
        if dout == "sum":
            grads = torch.autograd.grad(out.sum(), leaves)
        else:
            grads = torch.autograd.grad(out, leaves, d["dout"])
    return (out.detach(), keep[0]) + tuple(grads)


def assert_same_bytes(a, b, what, names=("out", "slots") + NAMES):
    for n, x, y in zip(names, a, b):
        assert x.dtype == y.dtype and x.shape == y.shape, f"{what}: {n}"
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), f"{what}: {n} differs"


def winners_of(t, slots):
    from deeppointmap_amd import ops
    return ops.group_train_winners(t["idx"].to(DEV), slots)


def named_by(win, N):
    """(B,N) bool: the points that win some maximum"""
    named = torch.zeros(win.shape[0], N, dtype=torch.bool, device=win.device)
    rows = torch.arange(win.shape[0], device=win.device).view(-1, 1, 1).expand_as(win)
    named[rows[win >= 0], win[win >= 0]] = True
    return named


def forced(t, slots):
    """the dense restatement with the kernel's routes in fp64 and fp32 on the device ->
    ({name: fp64 gradient ndarray}, {name: e}, fp64 out ndarray)"""
    win = winners_of(t, slots)
    o64, _, _, g64 = G.restate(t, torch.float64, DEV, winners=win, grads=True)
    _, _, _, g32 = G.restate(t, torch.float32, DEV, winners=win, grads=True)
    w64 = {n: g.cpu().numpy() for n, g in zip(NAMES, g64)}
    return w64, {n: rel_err(g.cpu().numpy(), w64[n]) for n, g in zip(NAMES, g32)}, o64.cpu().numpy()


def check_gradients(what, t, run):
    """out against the forced fp64 run by the feature rule, the four gradients by `check`"""
    w64, e, o64 = forced(t, run[1])
    assert_features_close(run[0].cpu().numpy(), o64, f"group_train edges {what}: out vs forced fp64")
    for n, g in zip(NAMES, run[2:]):
        check(f"group_train edges {what} {n}", g.cpu().numpy(), w64[n], e[n])


def check_forward(what, t, run):
    """out against the unforced fp64 maximum; every chosen slot's fp64 value within FEATURE_TOL x max(1, |max64|) of it; the
    routes that differ from the fp64 argmax are printed, not capped: a few hundred maxima make one near-tie a large share"""
    K = t["shape"][4]
    out, slots = run[0], run[1]
    max64, pts64, y64, _ = G.restate(t, torch.float64, DEV)
    assert_features_close(out.cpu().numpy(), max64.cpu().numpy(), f"group_train edges {what}: out vs fp64")
    assert bool(((slots < K) | (slots == G.NO_WINNER)).all())
    live_k = slots != G.NO_WINNER
    at = torch.gather(y64, 2, slots.long().clamp(max=K - 1).unsqueeze(2)).squeeze(2)
    at = torch.where(live_k, at, torch.zeros_like(at))
    gap = ((max64 - at) / max64.abs().clamp(min=1.0)).max().item()
    assert gap <= FEATURE_TOL, f"{what}: a chosen neighbour is {gap:.2e} below the fp64 maximum"
    live = max64 > 0
    differ = int(((winners_of(t, slots) != pts64) & live).sum())
    note(f"group_train edges {what}: {differ} routes differing from the fp64 argmax of {int(live.sum())} live maxima, largest gap "
         f"to the fp64 maximum {gap:.2e}")
    return max64, y64


@functools.lru_cache(maxsize=None)
def base(shape):
    """the plain case of a shape and the kernel's answer on it, computed once and never written to"""
    t = G.inputs(shape)
    return t, hip(t)


# ---- 1. the plan's edges and the tiny shapes against fp64 ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", G.PLAN_SHAPES + G.TINY_SHAPES, ids=ids)
def test_plan_and_tiny_shapes_against_fp64(shape):
    """PLAN_SHAPES: ppw = 2, a dead t iteration in the last wave, a last block with idle waves, lane groups past the last point,
    waves across frames; B S no multiple of the forward's or the mask kernel's block.  TINY_SHAPES: the scan below one element
    per thread, at 1024 + 1 and at 1; one point; K slots of one point."""
    t, run = base(shape)
    what = ids(shape)
    N = shape[2]
    assert_same_bytes(run, hip(t), f"{what}: two runs")
    check_forward(what, t, run)
    check_gradients(what, t, run)
    named = named_by(winners_of(t, run[1]), N)
    assert not (named & G.never(t).to(DEV)).any()
    assert (run[2][~named] == 0).all(), "a dP row no winner names is not zero"
    assert int((~named).sum()) >= shape[1] * G.ungathered_count(N)
    assert bool((run[2][named].abs().sum(-1) > 0).any())


# ---- 2. exact statements about the list machinery ------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", G.PLAN_SHAPES + G.TINY_SHAPES + G.SHIPPED_SMALL, ids=ids)
def test_dbeta_is_exact(shape):
    """dout holds small integers, so dbeta = sum over the live (b, s) of dout in ANY order of fp32 additions: an (s, c) whose
    winning row is visited zero times or twice changes an integer"""
    t, run = base(shape)
    out, slots, dP, _, _, dbeta = run
    K = shape[4]
    assert bool(((slots < K) | (slots == G.NO_WINNER)).all())
    assert torch.equal((slots != G.NO_WINNER), out > 0)
    want = (t["dout"].to(DEV) * (slots != G.NO_WINNER)).sum((0, 1))
    assert torch.equal(dbeta, want), f"dbeta differs in {int((dbeta != want).sum())} channels, by up to {(dbeta - want).abs().max():.0f}"
    named = named_by(winners_of(t, slots), shape[2])
    assert bool(((dP.abs().sum(-1) > 0) <= named).all())


# ---- 3. frames are independent, bit for bit --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [s for s in G.PLAN_SHAPES if s != (32, 3, 10925, 37, 32)], ids=ids)
def test_frames_are_independent(shape):
    """A frame run alone lands in other waves and lane groups than inside the batch; a row's arithmetic uses its own lane group
    only and a point's list is ordered inside its frame, so out, slots and dP are the same bytes.  The parameter gradients are
    sums over the frames in another order: the per-frame ones add up to the batch's within the `check` bound."""
    t, run = base(shape)
    what = ids(shape)
    alone = [hip(G.frame(t, b)) for b in range(shape[1])]
    for i, n in enumerate(("out", "slots", "dP")):
        assert_same_bytes((run[i],), (torch.cat([a[i] for a in alone]),), f"{what}: frames alone", names=(n,))
    _, e, _ = forced(t, run[1])
    for i, n in ((3, "dW_rel"), (4, "dgamma"), (5, "dbeta")):
        total = sum(a[i].double() for a in alone)
        check(f"group_train edges {what}: {n} of the batch vs the sum over frames", run[i].cpu().numpy(), total.cpu().numpy(), e[n])


# ---- 4. the order of the slots ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", G.PERM_SHAPES, ids=ids)
def test_slot_permutation(shape):
    """K different points per centre, their slots permuted.  out: the same bytes (a maximum over the same rows); slots map
    through the permutation; dP: the same bytes (a centre gives a point at most one winning row and a point's list is ordered
    by centre first); the parameter gradients: the same bytes (which wave owns a point and the order of every list are
    unchanged)."""
    t = G.distinct(G.inputs(shape))
    p, perm = G.permute_slots(t)
    a, b = hip(t), hip(p)
    what = ids(shape)
    assert_same_bytes((a[0],), (b[0],), what, names=("out",))
    live = a[1] != G.NO_WINNER
    assert bool(live.any()) and torch.equal(live, b[1] != G.NO_WINNER)
    mapped = torch.gather(perm.to(DEV), 2, a[1].long().clamp(max=shape[4] - 1))
    assert torch.equal(mapped[live], b[1].long()[live]), f"{what}: the slots do not follow the permutation"
    assert_same_bytes(a[2:], b[2:], what, names=NAMES)
    check_forward(what, t, a)


# ---- 5. ties between two different points -------------------------------------------------------------------------------------------------

TIES = [(Cout, k1, k2) for Cout, s in G.TIE_SHAPES.items() for k1, k2 in G.tie_pairs(Cout, s[4])]


@pytest.mark.parametrize("Cout,k1,k2", TIES)
def test_ties_go_to_the_earlier_slot(Cout, k1, k2):
    """Two different points with equal rows at slots k1 < k2 of every centre: in two lane groups of one iteration, in one lane
    group of two iterations, at the first and last slots.  The strict > and the merge's smaller-slot rule give k1 every time."""
    shape = G.TIE_SHAPES[Cout]
    t = G.tie(G.inputs(shape), k1, k2)
    run = hip(t)
    what = f"tie {k1},{k2} {ids(shape)}"
    slots, dP = run[1], run[2]
    check_forward(what, t, run)
    assert not bool((slots == k2).any()), "a tie went to the later slot"
    assert bool((slots == k1).any()), "the tied pair decides no maximum: the case means nothing"
    idx = t["idx"].to(DEV).long()
    bi = torch.arange(shape[1], device=DEV).view(-1, 1)
    assert (dP[bi, idx[:, :, k2]] == 0).all(), "the later point of a tie got a gradient"
    assert bool((dP[bi, idx[:, :, k1]].abs().sum(-1) > 0).any())
    check_gradients(what, t, run)


# ---- 6. dead and flat ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", G.VARIANT_SHAPES, ids=ids)
def test_all_dead(shape):
    """no maximum above the ReLU floor: zeros everywhere, through count, scan, fill and rank with every list empty"""
    out, slots, dP, dW, dg, db = hip(G.all_dead(G.inputs(shape)))
    assert (out == 0).all() and (slots == G.NO_WINNER).all()
    for n, g in zip(NAMES, (dP, dW, dg, db)):
        assert (g == 0).all(), n


@pytest.mark.parametrize("shape", G.VARIANT_SHAPES, ids=ids)
def test_dead_channel(shape):
    c0 = 5
    t = G.dead_channel(G.inputs(shape), c0)
    run = hip(t)
    out, slots, _, _, dg, db = run
    assert (out[:, :, c0] == 0).all() and (slots[:, :, c0] == G.NO_WINNER).all() and bool((slots != G.NO_WINNER).any())
    assert dg[c0] == 0 and db[c0] == 0
    check_forward(f"dead_channel {ids(shape)}", t, run)
    check_gradients(f"dead_channel {ids(shape)}", t, run)


@pytest.mark.parametrize("shape", G.VARIANT_SHAPES, ids=ids)
def test_flat_rows(shape):
    """zero variance in every row: rs = 1 / sqrt(eps) = 316, n = 0, y = beta for all K neighbours -- a K-fold tie that slot 0
    keeps -- and dgamma = 0"""
    t = G.flat_rows(G.inputs(shape))
    run = hip(t)
    out, slots, _, _, dg, _ = run
    what = f"flat_rows {ids(shape)}"
    assert torch.equal(out, torch.relu(t["beta"].to(DEV)).expand_as(out))
    assert torch.equal(slots != G.NO_WINNER, (t["beta"].to(DEV) > 0).expand_as(out)) and not bool(((slots != 0) & (slots != G.NO_WINNER)).any())
    assert (dg == 0).all()
    check_forward(what, t, run)
    check_gradients(what, t, run)


# ---- 7. what must not matter --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", G.VARIANT_SHAPES, ids=ids)
def test_ungathered_points_are_not_read_into_any_result(shape):
    """NaN in P and xyz of the points idx never names (the last point of the last frame, which the lane groups past the end
    load, among them; they sit in waves that walk other points' lists): every output keeps its bytes, their dP rows are zero"""
    t, clean = base(shape)
    got = hip(G.poison_ungathered(t))
    assert_same_bytes(clean, got, f"poisoned {ids(shape)}")
    nv = G.never(t).to(DEV)
    assert int(nv.sum()) > 0 and (got[2][nv] == 0).all() and (clean[2][nv] == 0).all()
    assert bool((clean[2].abs().sum(-1) > 0).any())


@pytest.mark.parametrize("shape", G.VARIANT_SHAPES, ids=ids)
def test_out_of_range_indices_are_read_clamped(shape):
    raw, clamped = G.out_of_range(G.inputs(shape))
    a, b = hip(raw), hip(clamped)
    assert_same_bytes(a, b, f"out of range {ids(shape)}")
    assert bool((a[1] != G.NO_WINNER).any())
    # the clamped points are gathered now and win somewhere: the comparison is not vacuous
    N = shape[2]
    bad = ((raw["idx"] < 0) | (raw["idx"] >= N)).to(DEV)
    assert bool((torch.gather(bad, 2, a[1].long().clamp(max=shape[4] - 1)) & (a[1] != G.NO_WINNER)).any())


@pytest.mark.parametrize("shape", [G.VARIANT_SHAPES[0], G.VARIANT_SHAPES[2]], ids=ids)
def test_broadcast_dout(shape):
    """group_train(...).sum() differentiated hands the backward a stride-0 dout: the same bytes as dout = ones"""
    t = G.inputs(shape)
    t["dout"] = torch.ones_like(t["dout"])
    assert_same_bytes(hip(t), hip(t, dout="sum"), f"broadcast dout {ids(shape)}")
