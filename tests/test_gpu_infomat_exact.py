"""GPU: the information matrix (csrc/infomat.hip) on lattice inputs, compared BIT FOR BIT with tests/infomat_restated.py.

The search kernel returns no per-point answer, only ten sums, and at the tolerance of the other infomat tests a wrong neighbour
is invisible (every query with a second target in reach given that target: 0.16 of the tolerance).  Here every coordinate is a
multiple of 2^-s, the radius a power of two and the pose a signed permutation with a lattice shift, so the kernel's arithmetic
is exact up to its one final rounding and the expected 36 floats are known exactly; tests/test_infomat_host.py proves per case
that giving ANY single query its second-nearest target changes them.  The cases (tests/golden/infomat_exact_cases.py) reach
what the other tests do not: the H = 1 branch, grids of more than 256 rows, partly filled chunks, grid rows of more than 512
points, d^2 == r^2, exact ties, queries outside the grid, large coordinates, and batched launches in which some pairs walk their
queries in another pair's cell order and some do not.  After a mismatch -- never before -- `localise` names the first slice
of 256 queries whose matrix differs and prints what the reference matched there."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import infomat_exact_cases as C  # noqa: E402
import infomat_restated as IR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from deeppointmap_amd import ops as _ops
    return _ops


def dev(a):
    return torch.tensor(np.asarray(a)).to(DEV)   # a copy: the cases are read-only and shared between tests


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def localise(ops, pcd1, pcd2, Rt, radius, s):
    """after a mismatch: the same target against the queries in slices of 256 -> a description of the first slice that differs"""
    p2, rt = dev(pcd2), dev(Rt)
    for lo in range(0, pcd1.shape[1], 256):
        part = np.ascontiguousarray(pcd1[:, lo:lo + 256])
        got = ops.information_matrix(dev(part), p2, rt, radius).cpu().numpy()
        ref = IR.restate(part, pcd2, Rt, radius, s)
        if not np.array_equal(bits(got), bits(ref["G"])):
            rows = [f"  query {lo + i}: q = {ref['q'][i].tolist()} -> target {m} at {ref['t'][m].tolist() if m >= 0 else None}, "
                    f"d^2 = {ref['d2'][i]} (r^2 = {ref['r2']}) lattice units" for i, m in enumerate(ref["match"].tolist())]
            return (f"first differing slice: queries [{lo}, {lo + part.shape[1]}); matched {got[3, 3]:.0f}, reference {ref['G'][3, 3]:.0f}\n"
                    f"got\n{got}\nwant\n{ref['G']}\nreference matches of the slice:\n" + "\n".join(rows))
    return "every slice of 256 queries agrees on its own: the difference needs the whole query set (block mapping, partial sums)"


@pytest.mark.parametrize("name", list(C.SINGLE))
def test_single_pair_bit_exact(ops, name):
    c, ref = C.case(name), C.reference(name)
    got = ops.information_matrix(dev(c["pcd1"]), dev(c["pcd2"]), dev(c["Rt"]), c["radius"]).cpu().numpy()
    print(f"{name}: matched {got[3, 3]:.0f} (reference {ref['G'][3, 3]:.0f}), {int((bits(got) != bits(ref['G'])).sum())} of 36 entries differ")
    if not np.array_equal(bits(got), bits(ref["G"])):
        pytest.fail(f"{name}: the matrix differs from the exact one\n" + localise(ops, c["pcd1"], c["pcd2"], c["Rt"], c["radius"], c["s"]))
    if name == "no_match":
        assert not got.any()


@pytest.mark.parametrize("n_pairs", list(C.PAIR_LISTS))
def test_batched_bit_exact(ops, n_pairs):
    """3 pairs (plain block mapping), 8 and 16 (XCD-aware); Rt_rows and out_rows are column views of one (P, 56) table"""
    pairs, frames, poses = C.PAIR_LISTS[n_pairs], C.frames(), C.pair_poses(n_pairs)
    pts = dev(frames)
    src = torch.tensor([a for a, _ in pairs], dtype=torch.int32, device=DEV)
    dst = torch.tensor([b for _, b in pairs], dtype=torch.int32, device=DEV)
    start = np.full((n_pairs, 56), -7.0, dtype=np.float32)
    start[:, :12] = poses
    start[:, 12:20] = 100.0 + np.arange(n_pairs * 8, dtype=np.float32).reshape(n_pairs, 8)
    table = dev(start)
    ops.information_matrix_batched(pts, src, dst, table[:, :12], table[:, 20:])
    split = dev(start)
    grids = ops.information_matrix_grids(pts, dst)
    ops.information_matrix_batched(pts, src, dst, split[:, :12], split[:, 20:], grids=grids)
    one, two = table.cpu().numpy(), split.cpu().numpy()
    assert np.array_equal(bits(one[:, :20]), bits(start[:, :20]))       # the columns outside [20:56] are untouched
    assert np.array_equal(bits(two), bits(one))                         # grids built ahead: the same computation bit for bit
    for p, (a, b) in enumerate(pairs):
        ref = C.pair_reference(n_pairs, p)
        got = one[p, 20:].reshape(6, 6)
        print(f"P = {n_pairs}, pair {p} ({a}, {b}): matched {got[3, 3]:.0f} (reference {ref['G'][3, 3]:.0f})")
        if a == b:
            assert got[3, 3] == C.N_BATCH
        if not np.array_equal(bits(got), bits(ref["G"])):
            pytest.fail(f"P = {n_pairs}, pair {p} ({a}, {b}): the matrix differs from the exact one; as a single pair:\n" +
                        localise(ops, frames[a], frames[b], np.array(poses[p]), 1.0, 5))
