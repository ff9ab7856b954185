"""GPU: the kernels of OutlierFilter / LowPassFilter (csrc/knn.hip: knn_self_kernel, point_normals_kernel, ball_query_kernel;
csrc/preprocess.hip: lowpass_sim_kernel, stat_filter_kernel) each through its own entry point, compared ROW BY ROW with the
brute-force restatements of tests/filters_restated.py on the cases of tests/filters_cases.py -- lattice inputs on which equal
distances are bit-equal and "on the radius" / "on the cut" are exact.  tests/test_filters_host.py proves without a GPU that the
restatements are right and that a wrong tie rule, an inclusive radius or the other comparison of the cut changes what is
compared here.  Every input is finite except the one NaN of the cut's NaN case, which the kernel meets in a comparison only."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filters_cases as C  # noqa: E402
import filters_restated as FR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EUNSUPPORTED = -2
U = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a):
    return torch.tensor(np.asarray(a)).to(DEV)       # a copy: the cases are shared between tests


@pytest.fixture(scope="module")
def api():
    from deeppointmap_amd import _lib, ops
    return _lib.load(), _lib, ops


# ---- the four kernel-level entry points, numpy in, numpy out ---------------------------------------------------------
def run_knn(api, xyz, K, cell=C.KNN_CELL):
    lib, L, ops = api
    g = dev(xyz)
    N = g.shape[0]
    ws = torch.empty(lib.dpm_knn_self_workspace_bytes(N), device=DEV, dtype=torch.uint8)
    idx = torch.full((N, K), -9, device=DEV, dtype=torch.int32)
    d2 = torch.full((N, K), -9.0, device=DEV)
    md = torch.full((N,), -9.0, device=DEV)
    L.check(lib.dpm_knn_self(ops._ptr(g), N, K, float(cell), ops._ptr(idx), ops._ptr(d2), ops._ptr(md), ops._ptr(ws), ops._stream(g)),
            "dpm_knn_self")
    return idx.cpu().numpy(), d2.cpu().numpy(), md.cpu().numpy()


def run_normals(api, xyz, radius):
    lib, L, ops = api
    g = dev(xyz)
    N = g.shape[0]
    ws = torch.empty(lib.dpm_knn_self_workspace_bytes(N), device=DEV, dtype=torch.uint8)
    out = torch.full((N, 3), -9.0, device=DEV)
    L.check(lib.dpm_point_normals(ops._ptr(g), N, float(radius), ops._ptr(out), ops._ptr(ws), ops._stream(g)), "dpm_point_normals")
    return out.cpu().numpy()


def run_sim(api, normals, idx, flux):
    lib, L, ops = api
    n, i = dev(normals), dev(idx)
    out = torch.full((n.shape[0],), -9.0, device=DEV)
    L.check(lib.dpm_lowpass_similarity(ops._ptr(n), ops._ptr(i), n.shape[0], i.shape[1], flux, ops._ptr(out), ops._stream(n)), "sim")
    return out.cpu().numpy()


def run_cut(api, stat, k_std, mode, xyz, idx_in, ratio):
    lib, L, ops = api
    s, x = dev(stat), dev(xyz)
    i = None if idx_in is None else dev(idx_in)
    N = s.shape[0]
    xo, io = torch.full((N, 3), -9.0, device=DEV), torch.full((N,), -9, device=DEV, dtype=torch.int32)
    n = torch.full((1,), -9, device=DEV, dtype=torch.int32)
    L.check(lib.dpm_stat_filter(ops._ptr(s), N, float(k_std), mode, float(ratio), ops._ptr(x), ops._ptr(i), ops._ptr(xo), ops._ptr(io),
                                ops._ptr(n), ops._stream(s)), "dpm_stat_filter")
    m = int(n.item())
    assert 0 <= m <= N
    return xo[:m].cpu().numpy(), io[:m].cpu().numpy(), m


# ------------------------------------------------------------------------------------------------------------------
# kNN
# ------------------------------------------------------------------------------------------------------------------
def check_knn(api, name, K, exact_mean=False):
    xyz, ref = C.knn_case(name), C.knn_reference(name, K)
    idx, d2, md = run_knn(api, xyz, K)
    bad = np.nonzero((idx != ref["idx"]).any(1))[0]
    rel = np.abs(md.astype(np.float64) - ref["mean_dist64"]) / np.maximum(ref["mean_dist64"], 1e-300)
    rel[ref["mean_dist64"] == 0] = np.abs(md[ref["mean_dist64"] == 0])
    print(f"{name}, K = {K}, N = {xyz.shape[0]}: {len(bad)} rows differ in idx, {int((bits(d2) != bits(ref['dist2'])).any(1).sum())} in dist2; "
          f"mean_dist worst relative error {rel.max() / U:.2f} x 2^-24 (bound {K + 2}), "
          f"{int((bits(md) != bits(ref['mean_dist'])).sum())} rows off the fp32 sequence")
    if len(bad):
        r = bad[0]
        pytest.fail(f"{name}, K = {K}: {len(bad)} rows differ, first row {r} at {xyz[r].tolist()}:\n got  {idx[r].tolist()}\n want {ref['idx'][r].tolist()}\n"
                    f" got d^2  {d2[r].tolist()}\n want d^2 {ref['dist2'][r].tolist()}")
    assert np.array_equal(bits(d2), bits(ref["dist2"]))
    assert (rel <= (K + 2) * U).all()
    if exact_mean:
        assert np.array_equal(bits(md), bits(ref["mean_dist"])) and np.array_equal(md.astype(np.float64), ref["mean_dist64"])


@pytest.mark.parametrize("K", C.KS)
@pytest.mark.parametrize("name", list(C.KNN_CASES))
def test_knn_every_row(api, name, K):
    check_knn(api, name, K)


@pytest.mark.parametrize("N", C.KNN_BOX_N)
def test_knn_around_the_grid_threshold(api, N):
    for K in (1, 16):
        check_knn(api, f"box{N}", K)


@pytest.mark.parametrize("K", C.KS)
def test_knn_smallest_cloud(api, K):
    check_knn(api, f"smallest{K}", K)


@pytest.mark.parametrize("K", [4, 16])
def test_knn_mean_dist_exact_on_the_345_line(api, K):
    check_knn(api, "line345", K, exact_mean=True)


def test_knn_limits_of_the_entry_point(api):
    lib, L, ops = api
    xyz = dev(C.knn_case("box1023"))
    ws = torch.empty(lib.dpm_knn_self_workspace_bytes(1023), device=DEV, dtype=torch.uint8)
    out = torch.empty(1023, 64, device=DEV, dtype=torch.int32)
    assert lib.dpm_knn_self(ops._ptr(xyz), 1023, 64, 1.0, ops._ptr(out), None, None, ops._ptr(ws), ops._stream(xyz)) == EUNSUPPORTED
    # a cloud smaller than K + 1, reachable through the C entry point only: the others in order, then (q, 0)
    three = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.0, 2.0]], dtype=np.float32)
    idx, d2, md = run_knn(api, three, 5)
    ref = FR.knn_self(three, 5)
    assert ref["idx"].tolist() == [[1, 2, 0, 0, 0], [0, 2, 1, 1, 1], [0, 1, 2, 2, 2]]
    assert np.array_equal(idx, ref["idx"]) and np.array_equal(bits(d2), bits(ref["dist2"])) and np.array_equal(bits(md), bits(ref["mean_dist"]))


def test_knn_real_frame_every_row(api):
    """every row of the 82 092-point frame against brute force over all pairs (no shortlist): replaces what the 99.9 % of
    test_preprocess.py::test_hip_filters_vs_oracle leaves open.  The brute force is the cost of this test (6.7e9 pairs, once)."""
    for K in (16, 10):
        check_knn(api, "real", K)


# ------------------------------------------------------------------------------------------------------------------
# normals
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["planes", "on_radius", "few", "random", "random_2km"])
def test_normals(api, name):
    xyz, radius = C.normals_cases()[name]
    ref = C.normals_reference(name)
    got = run_normals(api, xyz, radius).astype(np.float64)
    assert (np.abs(np.linalg.norm(got, axis=1) - 1.0) <= 4 * U).all()
    low = ref["count"] < 3
    assert np.array_equal(bits(got[low]), bits(np.tile([0.0, 0.0, 1.0], (int(low.sum()), 1))))
    bound = FR.normals_bound(ref)
    if name == "few":
        _, _, tri, run, direction = C.few()
        assert (np.abs(got[tri][:, 2]) >= 1 - 4 * U).all()
        assert (np.abs(got[run] @ direction) <= 4 * U).all()             # collinear: any unit vector across the line
        bound[run] = np.inf
    if name == "planes":
        assert (np.abs((got * C.planes()[1]).sum(1)) >= 1 - 4 * U).all()
    if name == "on_radius":
        rows = C.on_radius()[1]
        assert (np.abs(got[rows][:, 2]) >= 1 - 4 * U).all()             # strictly inside the radius: the plane alone
    exempt = bound > 1e-3
    sin = FR.sin_angle(got, ref["normals"])
    live = ~exempt & (bound > 0)
    print(f"{name}: {int(exempt.sum())} of {len(bound)} rows exempt; worst sin(angle) {sin[~exempt].max():.3g}, "
          f"worst sin(angle) / bound {float((sin[live] / bound[live]).max()):.3g}")
    assert (sin[~exempt] <= bound[~exempt]).all()
    assert exempt.mean() <= 0.01 if name.startswith("random") else exempt.sum() == (5 if name == "few" else 0)


# ------------------------------------------------------------------------------------------------------------------
# similarity
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,flux", C.SIM_EXACT)
def test_similarity_exact(api, N, K, flux):
    normals, idx = C.sim_case(N, K)
    want = FR.lowpass_similarity(normals, idx, flux)
    assert np.array_equal(want, want.astype(np.float32)) and len(np.unique(want)) >= 2      # exact values, and not all the same
    assert np.array_equal(bits(run_sim(api, normals, idx, flux)), bits(want))


def test_similarity_random_and_limits(api):
    lib, L, ops = api
    normals, idx, flux = C.sim_random()
    want = FR.lowpass_similarity(normals, idx, flux)
    err = np.abs(run_sim(api, normals, idx, flux).astype(np.float64) - want).max()
    print(f"similarity, random: worst error {err / U:.2f} x 2^-24 (bound {3 * flux})")
    assert err <= 3 * flux * U
    n, i = dev(normals), dev(idx)
    out = torch.empty(1000, device=DEV)
    assert lib.dpm_lowpass_similarity(ops._ptr(n), ops._ptr(i), 1000, 16, 9, ops._ptr(out), ops._stream(n)) == EUNSUPPORTED


# ------------------------------------------------------------------------------------------------------------------
# the cut
# ------------------------------------------------------------------------------------------------------------------
def check_cut(api, stat, k_std, xyz, idx_in, what):
    for mode in (0, 1):
        for ratio in (1.0, 60.0):
            for ii in (idx_in, None):
                wx, wi, wn = FR.stat_filter(stat, k_std, mode, xyz, ii, ratio)
                gx, gi, gn = run_cut(api, stat, k_std, mode, xyz, ii, ratio)
                assert gn == wn, (what, mode, ratio, gn, wn)
                assert np.array_equal(gi, wi) and np.array_equal(bits(gx), bits(wx)), (what, mode, ratio)
    return wn


@pytest.mark.parametrize("N", C.CUT_N)
def test_cut_with_every_element_on_it(api, N):
    for scale in (1.0, 2.0 ** -7):
        stat, xyz, idx = C.cut_case(N, scale)
        check_cut(api, stat, 1.0, xyz, idx, f"N = {N}, scale {scale}")
    if N == 1:
        assert run_cut(api, stat, 1.0, 0, xyz, idx, 1.0)[2] == 1 and run_cut(api, stat, 1.0, 1, xyz, idx, 1.0)[2] == 0


@pytest.mark.parametrize("name", ["two", "nan", "random0", "random1"])
def test_cut_other(api, name):
    stat, xyz, idx, k = C.cut_other(name)
    n = check_cut(api, stat, k, xyz, idx, name)
    if name == "nan":
        assert n == 0


# ------------------------------------------------------------------------------------------------------------------
# ball query
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", C.BALL_RADII)
@pytest.mark.parametrize("K", C.BALL_K)
@pytest.mark.parametrize("S", C.BALL_S)
def test_ball_query(api, S, K, radius):
    _, _, ops = api
    pts, lengths, _ = C.ball_batch()
    ctr = C.ball_centers(S)
    want = FR.ball_query(pts, lengths, ctr, K, radius)
    got = ops.ball_query(dev(pts), dev(lengths), dev(ctr), K, radius).cpu().numpy()
    assert np.array_equal(got, want)
    if S == 64:                                                          # the reference's own torch Querier.ball_query
        g = load_golden("ball_query.npz")
        hit = g[f"r{radius}_K{K}.hit"]
        assert hit.sum() > 100 and np.array_equal(got[hit], g[f"r{radius}_K{K}.idx"][hit]) and not got[~hit].any()


# ------------------------------------------------------------------------------------------------------------------
# the device-count chains
# ------------------------------------------------------------------------------------------------------------------
def poisoned(xyz, cap, poison):
    full = np.full((cap, 3), poison, dtype=np.float32)
    full[:xyz.shape[0]] = xyz
    idx = np.full(cap, -12345, dtype=np.int32)
    idx[:xyz.shape[0]] = np.arange(xyz.shape[0]) * 3 + 7
    return full, idx


def run_chain(api, which, xyz, poison, args, ratio):
    lib, L, ops = api
    n = xyz.shape[0]
    cap = n + 300
    full, idx = poisoned(xyz, cap, poison)
    g, gi = dev(full), dev(idx)
    count = torch.tensor([n], device=DEV, dtype=torch.int32)
    K = args[0] if which == "outlier" else args[1]
    ws = torch.empty(lib.dpm_filter_dc_workspace_bytes(cap, K), device=DEV, dtype=torch.uint8)
    xo, io = torch.full((cap, 3), -9.0, device=DEV), torch.full((cap,), -9, device=DEV, dtype=torch.int32)
    no = torch.full((1,), -9, device=DEV, dtype=torch.int32)
    if which == "outlier":
        st = lib.dpm_outlier_filter_dc(ops._ptr(g), ops._ptr(gi), ops._ptr(count), cap, args[0], float(args[1]), C.KNN_CELL, float(ratio),
                                       ops._ptr(xo), ops._ptr(io), ops._ptr(no), ops._ptr(ws), ops._stream(g))
    else:
        st = lib.dpm_lowpass_filter_dc(ops._ptr(g), ops._ptr(gi), ops._ptr(count), cap, float(args[0]), args[1], float(args[2]), args[3],
                                       C.KNN_CELL, float(ratio), ops._ptr(xo), ops._ptr(io), ops._ptr(no), ops._ptr(ws), ops._stream(g))
    L.check(st, which)
    m = int(no.item())
    assert 0 <= m <= n
    return xo[:m].cpu().numpy(), io[:m].cpu().numpy(), m, idx[:n]


OUTLIER_CHAINS = {"lattice_box": (10, 3.0), "duplicates": (10, 3.0), "cut": (1, 1.0)}


@pytest.mark.parametrize("poison", [float("nan"), 1e30], ids=["nan", "1e30"])
@pytest.mark.parametrize("name", list(OUTLIER_CHAINS))
def test_outlier_chain_with_a_device_count(api, name, poison):
    K, k_std = OUTLIER_CHAINS[name]
    xyz = C.cut_chain_cloud() if name == "cut" else C.knn_case(name)
    ref = FR.knn_self(xyz, K) if name == "cut" else C.knn_reference(name, K)
    for ratio in (1.0, 60.0):
        gx, gi, m, idx = run_chain(api, "outlier", xyz, poison, (K, k_std), ratio)
        wx, wi, wn = FR.stat_filter(ref["mean_dist"], k_std, 0, xyz, idx, ratio)
        print(f"outlier chain, {name}: {m} of {xyz.shape[0]} kept (restated {wn})")
        assert m == wn and np.array_equal(gi, wi) and np.array_equal(bits(gx), bits(wx))
    assert m == 801 if name == "cut" else 0 < m < xyz.shape[0]          # the cut case: every point is ON the cut or below


@pytest.mark.parametrize("poison", [float("nan"), 1e30], ids=["nan", "1e30"])
def test_lowpass_chain_with_a_device_count_on_the_radius(api, poison):
    xyz, rows, radius = C.on_radius()
    K, k_std, flux = 16, 2.0, 4
    normals = C.normals_reference("on_radius")["normals"].astype(np.float32)
    sim = FR.lowpass_similarity(normals, FR.knn_self(xyz, K)["idx"], flux).astype(np.float32)
    _, _, thr = FR.stat_threshold(sim, k_std, 1)
    assert np.abs(sim - thr).min() > 1e-4                                # nothing near the cut: rounding cannot decide a survivor
    incl = FR.point_normals(xyz, radius, rule="<=")["normals"].astype(np.float32)
    sim_incl = FR.lowpass_similarity(incl, FR.knn_self(xyz, K)["idx"], flux).astype(np.float32)
    other = FR.stat_filter(sim_incl, k_std, 1, xyz)[1]
    gx, gi, m, idx = run_chain(api, "lowpass", xyz, poison, (radius, K, k_std, flux), 60.0)
    wx, wi, wn = FR.stat_filter(sim, k_std, 1, xyz, idx, 60.0)
    print(f"lowpass chain, on_radius: {m} of {xyz.shape[0]} kept (restated {wn}; with an inclusive radius {len(other)})")
    assert 0 < wn < xyz.shape[0] and len(other) != wn                    # the inclusive radius would keep another set
    assert m == wn and np.array_equal(gi, wi) and np.array_equal(bits(gx), bits(wx))
