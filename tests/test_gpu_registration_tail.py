"""GPU: the registration tail kernel by kernel against the restatements of tests/registration_tail_restated.py --
corr_kabsch in the mode the decoder calls it in (from offsets), gather_pairs, the map-tile assembly and the copy / reduce
kernels around them, each at the shapes where its code takes another path.  The cases and their conditions (margins, ties,
survivor counts) are asserted on the host by tests/test_registration_tail_host.py; nothing here is skipped or loosened.

Toleranced comparisons print the reference's own fp32-vs-fp64 distance e, the bound and the observed error, and append them
to test_logs/registration_tail_accuracy.log where that directory can be written (profiles/registration_tail_accuracy.md)."""
import os
import sys
import warnings

import pytest
import torch

from conftest import ROOT, rot_angle
from oracle import dpm_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import registration_tail_restated as RT  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = RT.RES_HDR
POSE = [n for n, s in RT.KABSCH.items() if s["check"] == "pose" and not s["shift"]]
# fixed by the case list: direct mode orders equal weights differently (the tied cases), and its k is n, which at k4096's 6800
# survivors is past what the kernel's LDS holds
UNTIED = [n for n in POSE if n not in RT.TIED and n != "k4096"]


@pytest.fixture(scope="module")
def ops():
    from deeppointmap_amd import ops as _ops
    return _ops


def _log(line):
    print(line)
    try:
        os.makedirs(os.path.join(ROOT, "test_logs"), exist_ok=True)
        with open(os.path.join(ROOT, "test_logs", "registration_tail_accuracy.log"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def _ref(name, num_iter=3):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return RT.kabsch_reference(name, num_iter)


def _run(ops, c, num_iter=3, wide=False):
    """one case through the kernel's offsets mode; wide: coordinates as the xyz columns of 131-float rows"""
    xs, xd = c["xyz_s"], c["xyz_d"]
    if wide:
        xs, xd = RT.wide_rows(xs).to(DEV)[:, RT.XYZ_COL:RT.XYZ_COL + 3], RT.wide_rows(xd).to(DEV)[:, RT.XYZ_COL:RT.XYZ_COL + 3]
    else:
        xs, xd = xs.to(DEV), xd.to(DEV)
    res = ops.corr_kabsch(c["off"].to(DEV), xs, xd, c["si"].to(DEV), c["di"].to(DEV), c["conf"].to(DEV), c["eps"],
                          num_iter=num_iter).cpu()
    assert res.dim() == 1 and res.numel() == H + 2 * c["k"]
    return res


def _counts(res):
    return int(res[13]), int(res[14]), int(res[15])


def _used(res):
    """the defined part of a result row: header + inlier confidences"""
    return res[:H + int(res[14])]


def _same(a, b):
    """bit equality (a row without inliers carries NaN, which equals nothing)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check(res, r, what, bT=2e-5, bA=1e-5, br=2e-5):
    """the assertions of the direct-mode test (test_kabsch_loop_vs_reference), against the restatement r"""
    n, n_in, it = _counts(res)
    assert n == r["w"].numel() == r["n"], (what, n)
    assert it == r["iterations"], (what, it, r["iterations"])
    if r["check"] == "n_corr":
        return
    assert n_in == int(r["inl"].sum()), (what, n_in, int(r["inl"].sum()))
    assert torch.equal(res[H:H + n_in], r["w"][r["inl"]]), what
    assert (float(res[16]) == 0.0) if n_in == 0 else (abs(float(res[16]) - float(r["w"][r["inl"]][:30].mean())) < 1e-6), what
    assert float(res[17:20].abs().max()) == 0.0
    if r["check"] != "pose":
        return
    dA = rot_angle(res[:9].view(3, 3), r["R"])
    dT = float((res[9:12].view(3, 1) - r["T"]).norm())
    dr = abs(float(res[12]) - r["rmse"])
    R64, T64, rmse64, _ = RT.solve_svd64(r["w"], r["src"], r["dst"], r["masks"])     # e: the oracle's own fp32 error
    eT, eA, er = float((r["T"].double() - T64).norm()), rot_angle(r["R"], R64), abs(r["rmse"] - rmse64)
    _log(f"corr_kabsch {what} | T: e {eT:.3e} m, bound {bT:.3e}, observed {dT:.3e} | rot: e {eA:.3e} rad, bound {bA:.3e}, "
         f"observed {dA:.3e} | rmse: e {er:.3e}, bound {br:.3e}, observed {dr:.3e}")
    assert dA < bA and dT < bT and dr < br, (what, dA, dT, dr)
    return dA, dT, dr


# ---------------------------------------------------------------------------------------------------------------------
# corr_kabsch from offsets
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", POSE + ["k1", "one_survivor"])
def test_kabsch_from_offsets_vs_restatement(name, ops):
    """the full loop, and the loop stopped after its first round -- whose R, T are those of the SEEDING (w > 0.5 plus the 64
    largest through the merge ranking and the tie replay); three rounds mostly forget which 64 they started from"""
    c = RT.kabsch_case(name)
    for num_iter in (3, 1):
        r = _ref(name, num_iter)
        res = _run(ops, c, num_iter)
        _check(res, r, f"{name} rounds<={num_iter}")
    # 131-float rows with xyz at column 128 (decoder.py:453) are the same correspondences: same bytes; and the kernel
    # repeats itself
    assert _same(_used(_run(ops, c, 1, wide=True)), _used(res)) and _same(_used(_run(ops, c, 1)), _used(res))


def test_kabsch_1000_m_from_the_origin(ops):
    """coordinates near 1000 m: fp32 centroids and residuals carry 6e-5 m steps, so the unit-scale bounds do not apply; the
    bound is three times the oracle's own fp32 distance e from the fp64 evaluation of the same rounds (the factor
    tests/test_gpu_margin.py uses), and never below the unit-scale bound."""
    name = "shift1000"
    r = _ref(name)
    R64, T64, rmse64, _ = RT.solve_svd64(r["w"], r["src"], r["dst"], r["masks"])
    eT, eA, er = float((r["T"].double() - T64).norm()), rot_angle(r["R"], R64), abs(r["rmse"] - rmse64)
    bT, bA, br = max(3 * eT, 2e-5), max(3 * eA, 1e-5), max(3 * er, 2e-5)
    res = _run(ops, RT.kabsch_case(name))
    _check(res, r, name, bT, bA, br)
    # against fp64 itself the kernel is no farther than the bound either
    assert float((res[9:12].view(3, 1).double() - T64).norm()) < bT + eT


@pytest.mark.parametrize("name", UNTIED)
def test_kabsch_offsets_mode_equals_direct_mode(name, ops):
    """the restatement's (src, dst, w) handed over ready-made give the bytes the kernel makes of the offsets itself: the two
    copies, the cut, the compaction and the merge ranking are the restatement's.  nothing_cut is the case the whole 2k
    survive in; with distinct confidences the two modes rank equal weights (the two copies of a pair) the same way."""
    c, r = RT.kabsch_case(name), _ref(name)
    a = _run(ops, c)
    b = ops.corr_kabsch(None, r["src"].t().contiguous().to(DEV), r["dst"].t().contiguous().to(DEV), None, None,
                        r["w"].to(DEV), c["eps"]).cpu()
    assert _same(_used(a), _used(b)), name


def _batch(ops, names, header_cols=(5, 25)):
    cs = [RT.kabsch_case(n) for n in names]
    k, B = cs[0]["k"], len(cs)
    buf_s = torch.cat([RT.wide_rows(c["xyz_s"]) for c in cs]).to(DEV)
    buf_d = torch.cat([RT.wide_rows(c["xyz_d"]) for c in cs]).to(DEV)
    wide = torch.full((B, 32), -3.0, device=DEV)
    res = ops.corr_kabsch(torch.stack([c["off"] for c in cs]).to(DEV), buf_s[:, RT.XYZ_COL:RT.XYZ_COL + 3],
                          buf_d[:, RT.XYZ_COL:RT.XYZ_COL + 3], torch.stack([c["si"] for c in cs]).to(DEV),
                          torch.stack([c["di"] for c in cs]).to(DEV), torch.stack([c["conf"] for c in cs]).to(DEV), RT.EPS,
                          header_out=wide[:, header_cols[0]:header_cols[1]], batch=B)
    torch.cuda.synchronize()
    assert tuple(res.shape) == (B, H + 2 * k)
    return cs, res.cpu(), wide.cpu()


def test_kabsch_batch_of_three(ops):
    cs, res, wide = _batch(ops, RT.BATCH)
    assert len({_counts(res[b])[0] for b in range(3)}) == 3            # a different survivor count per element
    for b, c in enumerate(cs):
        _check(res[b], _ref(c["name"]), f"batch element {b}")
        assert _same(_used(res[b]), _used(_run(ops, c))), b      # = its own batch-of-one call, packed coordinates
        assert _same(_used(res[b]), _used(_run(ops, c, wide=True))), b
    # header_out: a column range of a wider tensor receives the 20 header floats, its neighbours nothing
    assert _same(wide[:, 5:25], res[:, :H])
    assert bool((wide[:, :5] == -3.0).all()) and bool((wide[:, 25:] == -3.0).all())


def test_kabsch_empty_set(ops):
    """every offset of one batch element is cut: n = 0.  The kernel's loops are all bounded by n, so nothing is read or
    written out of range; the row it leaves says "no correspondences" and cannot be mistaken for a pose; its neighbours in
    the batch are untouched by it."""
    cs, res, wide = _batch(ops, RT.BATCH_WITH_EMPTY)
    n, n_in, it = _counts(res[1])
    print("header of the empty element:", res[1, :H].tolist())
    assert (n, n_in, it) == (0, 0, 1)
    assert not (bool(torch.isfinite(res[1, 9:12]).all()) and bool(torch.isfinite(res[1, 12])))
    assert _same(wide[:, 5:25], res[:, :H])
    for b in (0, 2):
        _check(res[b], _ref(cs[b]["name"]), f"element {b} next to the empty one")
        assert _same(_used(res[b]), _used(_run(ops, cs[b]))), b
    solo = _run(ops, cs[1])
    assert _counts(solo) == (0, 0, 1) and not bool(torch.isfinite(solo[9:13]).all())


def test_kabsch_refuses_what_its_lds_cannot_hold(ops):
    """k = 8192: 24 B of LDS per pair exceed the CU's 160 KB -- an error from the launcher, nothing queued; k = 4096, the
    decoder's stated maximum, runs (test_kabsch_from_offsets_vs_restatement[k4096])."""
    k = 8192
    z = torch.zeros(k, 3, device=DEV)
    idx = torch.zeros(k, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.corr_kabsch(torch.zeros(2 * k, 3, device=DEV), z, z, idx, idx, torch.zeros(k, device=DEV), RT.EPS)
    torch.cuda.synchronize()
    assert "k4096" in POSE


# ---------------------------------------------------------------------------------------------------------------------
# gather_pairs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RT.GATHER_PAIRS, ids=lambda s: "x".join(map(str, s)))
def test_gather_pairs(shape, ops):
    B, M, N, E, k = shape
    x, y, flat = RT.gather_pairs_case(*shape)
    wX, wsi, wdi = RT.gather_pairs(x, y, flat)
    X, si, di = ops.gather_pairs(x.to(DEV), y.to(DEV), flat.to(DEV))
    assert torch.equal(si.cpu(), wsi) and torch.equal(di.cpu(), wdi)
    X = X.cpu()
    assert torch.equal(X[:, :k], wX[:, :k]) and torch.equal(X[:, k:], wX[:, k:])
    if B == 1:      # the single-pair call form: 2-D in, 2-D out
        X2, si2, di2 = ops.gather_pairs(x[0].to(DEV), y[0].to(DEV), flat[0].to(DEV))
        assert X2.dim() == 2 and si2.dim() == 1
        assert torch.equal(X2.cpu(), wX[0]) and torch.equal(si2.cpu(), wsi[0]) and torch.equal(di2.cpu(), wdi[0])


# ---------------------------------------------------------------------------------------------------------------------
# assemble_map_tile / MapTileStore
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RT.MAP_TILE))
def test_map_tile_at_kitti_scale(name):
    from deeppointmap_amd.maptile import MapTileStore, assemble_map_tile
    kp, poses, centre, sel = RT.map_tile_case(name)
    n, C, S, _ = RT.MAP_TILE[name]
    t64, t32 = RT.map_tile64(kp, poses, centre, sel), RT.map_tile32(kp, poses, centre, sel)
    e = float((t32[-3:].double() - t64[-3:]).abs().max())
    bound = max(3 * e, 2e-5)
    tile = assemble_map_tile(kp.to(DEV), poses, centre, None if sel is None else torch.tensor(sel, dtype=torch.int32)).cpu()
    assert tuple(tile.shape) == tuple(t64.shape)
    assert torch.equal(tile[:-3], kp[list(range(n)) if sel is None else sel, :-3].transpose(0, 1).reshape(C - 3, -1))
    got = float((tile[-3:].double() - t64[-3:]).abs().max())
    _log(f"map_tile {name} (C {C}, S {S}, K {t64.shape[1] // S}) | xyz: e {e:.3e} m, bound {bound:.3e}, observed {got:.3e}")
    assert got <= bound
    # the store addresses the same scans by token
    order = list(range(n)) if sel is None else sel
    store = MapTileStore(DEV, channels=C, points=S, capacity=2)
    for i in range(n):
        store.put(50 + i, kp[i])
    t2, tok = store.tile([50 + i for i in order], [poses[i] for i in order], centre)
    assert torch.equal(t2.cpu(), tile) and tok.tolist() == [50 + i for i in order for _ in range(S)]


# ---------------------------------------------------------------------------------------------------------------------
# the copy and reduce kernels
# ---------------------------------------------------------------------------------------------------------------------
def test_gather_frames(ops):
    g = torch.Generator().manual_seed(2)
    F = 5
    index = torch.tensor([4, 0, 4, 2, 2, 1, 4], dtype=torch.int32)           # repeats, the last frame

    def packed(rows, cols, shift):
        buf = torch.randn(F * rows * cols + 4, generator=g).to(DEV)
        src = buf[shift:shift + F * rows * cols].view(F, rows, cols)
        assert src.data_ptr() % 16 == (4 * shift) % 16
        out = ops.gather_frames(src, index.to(DEV), rows, cols)
        assert torch.equal(out, src[index.long().to(DEV)])

    for rows, cols in [(3, 8), (300, 256), (7, 3), (30000, 3), (1, 4), (65, 1020)]:
        # less than one block; more than 64 blocks' worth (the grid-stride tail); 16-byte rows and 3-float rows
        packed(rows, cols, 0)
        packed(rows, cols, 1)        # a base one float in: 4-byte but not 16-byte aligned, the scalar path whatever cols is
    # the decoder's xyz read: rows of 131 floats, columns 128..130 (decoder.py:453)
    for M in (1, 256, 1000):
        tu = torch.randn(F * M, RT.LD, generator=g).to(DEV)
        out = ops.gather_frames(tu, index.to(DEV), M, 3, ld=tu.stride(0), offset=RT.XYZ_COL)
        assert torch.equal(out, tu.view(F, M, RT.LD)[index.long().to(DEV)][:, :, RT.XYZ_COL:])
    tu = torch.randn(F * 64, 24, generator=g).to(DEV)                        # ld > cols with cols % 4 == 0
    out = ops.gather_frames(tu, index.to(DEV), 64, 8, ld=24, offset=12)
    assert torch.equal(out, tu.view(F, 64, 24)[index.long().to(DEV)][:, :, 12:20])


@pytest.mark.parametrize("C", [1, 29, 128])
@pytest.mark.parametrize("S", [1, 31, 32, 33, 256])
def test_emit_descriptors(S, C, ops):
    g = torch.Generator().manual_seed(S * 1000 + C)
    lengths = torch.tensor([0, S, S // 2, max(S - 1, 0)], dtype=torch.int32)  # ragged, 0 and S among them
    B = lengths.numel()
    xyz, fea = torch.randn(B, S, 3, generator=g) * 30, torch.randn(B, S, C, generator=g)
    for scale, spare in ((0.0, 0), (1.0 / 60.0, 0), (0.37, 2)):
        wc, wf, wp, wd = RT.emit_descriptors(xyz, fea, lengths, scale)
        coor, feat, pad, desc = ops.emit_descriptors(xyz.to(DEV), fea.to(DEV), lengths.to(DEV), scale, spare_frames=spare)
        assert pad.dtype == torch.bool and torch.equal(pad.cpu(), wp)
        assert torch.equal(coor.cpu(), wc) and torch.equal(feat.cpu(), wf)
        if scale == 0.0:
            assert desc is None
        else:       # the wrapper allocates the descriptor: the spare frames are there, their contents are the caller's
            assert tuple(desc.shape) == (B + spare, C + 3, S)
            assert torch.equal(desc[:B].cpu(), wd)


def test_nested_levels(ops):
    g = torch.Generator().manual_seed(3)
    xyz0 = torch.randn(4, 300, 3, generator=g)
    len0 = torch.tensor([0, 1, 256, 300], dtype=torch.int32)
    npoints = [300, 257, 256, 1]
    got = ops.nested_levels(xyz0.to(DEV), len0.to(DEV), npoints)
    want = RT.nested_levels(xyz0, len0, npoints)
    assert len(got) == len(want)
    for K, (gi, gx, gl), (wi, wx, wl) in zip(npoints, got, want):
        assert tuple(gi.shape) == (4, K) and gi.dtype == torch.int32 and gl.dtype == torch.int32
        assert torch.equal(gi.cpu(), wi) and torch.equal(gx.cpu(), wx) and torch.equal(gl.cpu(), wl)


@pytest.mark.parametrize("row_multiple", [1, 4, 64])
@pytest.mark.parametrize("R", [1, 77])
def test_to_channel_first(R, row_multiple, ops):
    g = torch.Generator().manual_seed(R + row_multiple)
    for B, C in ((1, 1), (3, 33), (2, 131)):
        x = torch.randn(B, R, C, generator=g)
        out = ops.to_channel_first(x.to(DEV), row_multiple)
        ld = -(-R // row_multiple) * row_multiple
        assert tuple(out.shape) == (B, C, R) and out.stride(2) == 1
        if C > 1:
            assert out.stride(1) == ld
        if B > 1:
            assert out.stride(0) == C * ld
        assert torch.equal(out.cpu(), x.transpose(1, 2))


@pytest.mark.parametrize("C", [1, 3, 32, 255, 256])
@pytest.mark.parametrize("R", [1, 5])
def test_l2_normalize(R, C, ops):
    g = torch.Generator().manual_seed(R * 1000 + C)
    x = torch.randn(R + 2, C, generator=g)
    x[R] = 0.0                                       # a zero row and a row of norm 1e-20: both leave as x / 1e-12
    x[R + 1] = x[R + 1] / x[R + 1].norm() * 1e-20
    want = RT.l2_normalize64(x)
    assert float(want[R].abs().max()) == 0.0 and torch.equal(want[R + 1], x[R + 1].double() / 1e-12)
    out = ops.l2_normalize(x.to(DEV)).cpu()
    err = (out.double() - want).abs()
    rel = float((err / want.abs().clamp(min=1e-300)).max())
    _log(f"l2_normalize R {R} C {C} | bound {RT.l2_bound(C):.3e} relative, observed {rel:.3e}")
    assert bool((err <= RT.l2_bound(C) * want.abs()).all()), rel
    assert float(out[R].abs().max()) == 0.0
    # a view one float in (no 16-byte rows): the scalar path, the same bits
    buf = torch.empty((R + 2) * C + 1, device=DEV)
    buf[1:].copy_(x.flatten())
    shifted = buf[1:].view(R + 2, C)
    assert shifted.data_ptr() % 16 == 4
    assert torch.equal(ops.l2_normalize(shifted).cpu().view(torch.int32), out.view(torch.int32))


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 256, 256), (2, 1000, 300)], ids=lambda s: "x".join(map(str, s)))
def test_mean_rows(shape, ops):
    B, R, C = shape
    x = torch.randn(B, R, C, generator=torch.Generator().manual_seed(R)) + 0.25
    wide = torch.full((B, C + 9), -3.0, device=DEV)
    ops.mean_rows(x.to(DEV), wide[:, 4:4 + C])           # a column range of a wider tensor (decoder.py:694)
    wide = wide.cpu()
    err = (wide[:, 4:4 + C].double() - x.double().mean(dim=1)).abs()
    bound = RT.mean_rows_bound(x)
    _log(f"mean_rows {B}x{R}x{C} | bound (smallest column) {float(bound.min()):.3e}, observed (largest column) {float(err.max()):.3e}, "
         f"largest error / bound {float((err / bound.clamp(min=1e-300)).max()) if R > 1 else 0.0:.3f}")
    assert bool((err <= bound).all()), (float(err.max()), float(bound.min()))
    assert bool((wide[:, :4] == -3.0).all()) and bool((wide[:, 4 + C:] == -3.0).all())


@pytest.mark.parametrize("R", [1, 255, 257])
def test_position_embedding_rows(R, ops):
    g = torch.Generator().manual_seed(R)
    xyz = (torch.rand(R, 3, generator=g) * 2 - 1) * 80.0                     # metres, up to +-80
    xyz[0] = torch.tensor([80.0, -80.0, 0.0])
    want = O.position_embedding(xyz, 256)
    dim_t = RT.dim_t(256).to(DEV)
    nf = dim_t.numel()
    for rows in (xyz.to(DEV), RT.wide_rows(xyz).to(DEV)[:, RT.XYZ_COL:RT.XYZ_COL + 3]):     # packed, and 131-float rows
        out = ops.posemb(rows, dim_t, 256).cpu()
        assert tuple(out.shape) == (R, 256)
        err = float((out - want).abs().max())
        _log(f"posemb R {R} ld {rows.stride(0)} | bound 2.000e-06, observed {err:.3e}")
        assert err <= 2e-6
        assert bool((out[:, 3 * nf:] == 0).all()) and 3 * nf == 252
