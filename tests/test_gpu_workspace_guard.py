"""GPU: no entry point writes outside the `workspace` its dpm_*_workspace_bytes asked for.

Every case is one call (or one forward + backward pair) at a tiny shape that reaches a branch of the workspace's layout
(csrc/workspace.h).  It runs three times on the same inputs:
  * once as callers run it, with a fresh workspace of its own: the reference outputs;
  * once with `buffer + 4096` as the workspace, buffer = 4096 + bytes + 4096 bytes of 0xA5;
  * once with `buffer + 4096 + 80` (16-byte aligned, not 256), the buffer 256 bytes longer.
After the last two, every byte of the buffer outside [workspace, workspace + bytes) still holds 0xA5, and the outputs
equal the reference byte for byte (the grid neighbour search: slot 0 and the sorted row, see knn_rows).  The test only looks
at memory it owns.

The calls go through the project's thin wrappers where one exists (they marshal a dozen pointers each) and through the C
ABI by hand otherwise.  Either way the entry point receives the guarded pointer: while a case runs, `Lib` stands in for
the loaded library, forwards every call unchanged except for the `workspace` argument of the entry points in WS_FROM_END,
and records what the *_workspace_bytes entry points answered (the largest answer is `bytes`).

Every entry point below takes both offsets: those that round their base up do so themselves, and the others (pairing,
group_train, voxel_sampler, scan_context) only need the 16-byte alignment that 80 keeps."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, FILL = 4096, 0xA5

# position of `workspace` counted from the end of the C argument list (the stream is last)
WS_FROM_END = {
    "dpm_knn_hybrid": 2, "dpm_knn_hybrid_reuse": 4, "dpm_knn_build_grid": 2, "dpm_knn_hybrid_prebuilt": 2, "dpm_knn_self": 2,
    "dpm_point_normals": 2, "dpm_outlier_filter_dc": 2, "dpm_lowpass_filter_dc": 2, "dpm_reg_loss_forward": 2,
    "dpm_reg_loss_backward": 4, "dpm_match_topk": 2, "dpm_dual_softmax_topk": 2, "dpm_attention_split": 2,
    "dpm_attention_train_backward": 2, "dpm_dense_train_backward_rows": 2, "dpm_dense_train_backward_gemm": 2,
    "dpm_group_train_backward": 2, "dpm_loop_pool_forward": 2, "dpm_loop_pool_backward": 2, "dpm_fps_ex": 3,
    "dpm_voxel_sampler_select": 2, "dpm_voxel_select": 2, "dpm_ground_filter": 2, "dpm_preprocess_scan": 2,
    "dpm_scan_context_search": 2, "dpm_distance_stats": 2, "dpm_cloud_nn": 2, "dpm_icp_refine_batched": 2,
    "dpm_information_matrix_batched": 2, "dpm_local_map_register": 2,
}


class Lib:
    """the loaded library with the workspace of the entry points above replaced by `ws` (None: as the caller passed it)"""

    def __init__(self, real, ws=None):
        self.real, self.ws, self.sizes, self.guarded = real, ws, [], []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name.endswith("_workspace_bytes"):
            def size(*a):
                n = int(fn(*a))
                self.sizes.append(n)
                return n
            return size
        if name in WS_FROM_END:
            def call(*a):
                a = list(a)
                assert a[-WS_FROM_END[name]] is not None, name
                self.guarded.append(name)
                if self.ws is not None:
                    a[-WS_FROM_END[name]] = self.ws
                return fn(*a)
            return call
        return fn


@pytest.fixture(scope="module")
def api():
    from deeppointmap_amd import _lib, ops
    return _lib.load(), _lib, ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def ball(*shape, seed=0):
    """points inside the unit ball"""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(*shape, 3, generator=g)
    return (p / p.norm(dim=-1, keepdim=True) * torch.rand(*shape, 1, generator=g) ** (1 / 3)).to(DEV)


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def fresh(nbytes):
    """a workspace of the case's own (the reference run; the guarded runs never see it)"""
    return torch.full((max(int(nbytes), 1),), FILL, device=DEV, dtype=torch.uint8)


def same_bytes(a, b):
    a, b = a.contiguous().reshape(-1), b.contiguous().reshape(-1)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def run_guarded(api, monkeypatch, case, entry_points, nbytes=None):
    real, L, ops = api

    def run(lib):
        with monkeypatch.context() as m:
            m.setattr(L, "_lib", lib)
            out = [t.clone() for t in case(lib, L, ops)]
        torch.cuda.synchronize()
        return out

    ref = Lib(real)
    want = run(ref)
    assert set(entry_points) <= set(ref.guarded), (entry_points, ref.guarded)
    nbytes = max(ref.sizes) if nbytes is None else nbytes
    assert nbytes > 0
    for off in (0, 80):
        buf = torch.full((GUARD + nbytes + GUARD + (256 if off else 0),), FILL, device=DEV, dtype=torch.uint8)
        assert buf.data_ptr() % 256 == 0
        lo = GUARD + off
        got = run(Lib(real, buf.data_ptr() + lo))
        print(f"{'+'.join(entry_points)}: {nbytes} bytes at offset {off}")
        assert bool((buf[:lo] == FILL).all()), f"offset {off}: bytes in front of the workspace were written"
        assert bool((buf[lo + nbytes:] == FILL).all()), f"offset {off}: bytes behind the workspace were written"
        assert len(got) == len(want) and len(want) > 0
        for k, (g, w) in enumerate(zip(got, want)):
            assert same_bytes(g, w), f"offset {off}: output {k} differs from the run with a workspace of its own"


# ---- neighbour search ------------------------------------------------------------------------------------------------
KNN = dict(B=2, N=1024, S=64, K=16, radius=0.2)


def knn_inputs():
    pts = ball(KNN["B"], KNN["N"])
    return pts, i32([KNN["N"], KNN["N"] - 3]), pts[:, :KNN["S"]].contiguous()


def knn_rows(idx):
    """what dpm_knn_hybrid defines of a row: slot 0 (the nearest point) and the SET of the others -- their order follows the
    grid's atomically scattered point order and is free from run to run (tests/test_gpu_ops.py compares them as sets too), so
    the rows are compared sorted"""
    return [idx[..., 0].contiguous(), idx.sort(dim=-1).values]


def case_knn_hybrid(lib, L, ops):
    pts, lengths, centers = knn_inputs()
    B, N, S, K = KNN["B"], KNN["N"], KNN["S"], KNN["K"]
    idx = torch.full((B, S, K), -9, device=DEV, dtype=torch.int32)
    ws = fresh(lib.dpm_knn_workspace_bytes(B, N))
    L.check(lib.dpm_knn_hybrid(ops._ptr(pts), ops._ptr(lengths), ops._ptr(centers), B, N, S, K, KNN["radius"], ops._ptr(idx),
                               ops._ptr(ws), ops._stream(pts)), "dpm_knn_hybrid")
    return knn_rows(idx)


def case_knn_prebuilt(lib, L, ops):
    pts, lengths, centers = knn_inputs()
    grid = ops.knn_grid(pts, lengths, KNN["radius"])
    return knn_rows(ops.knn_hybrid(pts, lengths, centers, KNN["K"], KNN["radius"], grid=grid))


def case_knn_self(lib, L, ops):
    from deeppointmap_amd import preprocess
    out = preprocess.knn_self(ball(300, seed=1), 8)
    return [out["idx"], out["dist2"], out["mean_dist"]]


def case_point_normals(lib, L, ops):
    xyz = ball(300, seed=2)
    normals = torch.full((300, 3), -9.0, device=DEV)
    ws = fresh(lib.dpm_knn_self_workspace_bytes(300))
    L.check(lib.dpm_point_normals(ops._ptr(xyz), 300, 0.4, ops._ptr(normals), ops._ptr(ws), ops._stream(xyz)), "dpm_point_normals")
    return [normals]


def filter_dc(lib, L, ops, lowpass):
    from deeppointmap_amd.preprocess import KNN_CELL
    cap, n, K = 300, 257, 8
    xyz, idx, count = ball(cap, seed=3), torch.arange(cap, device=DEV, dtype=torch.int32), i32([n])
    xo, io = torch.full((cap, 3), -9.0, device=DEV), torch.full((cap,), -9, device=DEV, dtype=torch.int32)
    no = torch.full((1,), -9, device=DEV, dtype=torch.int32)
    ws = fresh(lib.dpm_filter_dc_workspace_bytes(cap, K))
    if lowpass:
        L.check(lib.dpm_lowpass_filter_dc(ops._ptr(xyz), ops._ptr(idx), ops._ptr(count), cap, 0.4, K, 2.0, 2, KNN_CELL, 1.0,
                                          ops._ptr(xo), ops._ptr(io), ops._ptr(no), ops._ptr(ws), ops._stream(xyz)), "dpm_lowpass_filter_dc")
    else:
        L.check(lib.dpm_outlier_filter_dc(ops._ptr(xyz), ops._ptr(idx), ops._ptr(count), cap, K, 1.0, KNN_CELL, 1.0, ops._ptr(xo),
                                          ops._ptr(io), ops._ptr(no), ops._ptr(ws), ops._stream(xyz)), "dpm_outlier_filter_dc")
    assert 0 < int(no.item()) <= n
    return [xo, io, no]


def case_outlier_filter_dc(lib, L, ops):
    return filter_dc(lib, L, ops, False)


def case_lowpass_filter_dc(lib, L, ops):
    return filter_dc(lib, L, ops, True)


# ---- losses and the decoder's matching --------------------------------------------------------------------------------
def case_reg_loss(lib, L, ops):
    B, M, N, C = 2, 65, 70, 64
    fa, fb = rnd(B, C, M, seed=4), rnd(B, C, N, seed=5)
    xa, xb = rnd(B, 3, M, seed=6), rnd(B, 3, N, seed=7)
    pa, pb = torch.zeros(B, M, dtype=torch.bool, device=DEV), torch.zeros(B, N, dtype=torch.bool, device=DEV)
    pa[:, -3:] = True
    nn_a, nn_b = ops.reg_loss_pairs(xa, xb, 1.0)
    loss, stats, ws = ops.reg_loss_forward(fa, fb, xa, xb, pa, pb, nn_a, nn_b, 0.1, 1.0, True)
    ga, gb = ops.reg_loss_backward(xa, xb, nn_a, nn_b, (B, C, M, N), 0.1, 1.0, True, torch.ones((), device=DEV), stats, ws)
    return [loss, stats, ga, gb]


def case_match_topk(lib, L, ops):
    f = torch.nn.functional.normalize
    return list(ops.match_topk(f(rnd(2, 65, 64, seed=8), dim=-1), f(rnd(2, 64, 64, seed=9), dim=-1), 0.1, 32))   # two strips of 64 rows


def dual_softmax(M, N):
    def case(lib, L, ops):
        S = rnd(2, M, N, seed=10)
        return list(ops.dual_softmax_topk(S, 0.1, 64)) + [S]
    return case


def case_attention_split(lib, L, ops):
    B, M, N, heads, E, nsplit = 1, 8, 1024, 1, 32, 2
    q, k, v = rnd(B * M, E, seed=11), rnd(B * N, E, seed=12), rnd(B * N, E, seed=13)
    out = torch.full((B * M, E), -9.0, device=DEV)
    ws = fresh(lib.dpm_attention_split_workspace_bytes(B, M, heads, E // heads, nsplit))
    L.check(lib.dpm_attention_split(ops._ptr(q), E, M * E, ops._ptr(k), E, N * E, ops._ptr(v), E, N * E, ops._ptr(out), E, M * E, B, M,
                                    N, heads, E // heads, 0, nsplit, ops._ptr(ws), ops._stream(q)), "dpm_attention_split")
    return [out]


# ---- training backwards -----------------------------------------------------------------------------------------------
def case_attention_train(lib, L, ops):
    B, M, N, heads, E = 2, 65, 70, 1, 32
    q, k, v, dout = rnd(B * M, E, seed=14), rnd(B * N, E, seed=15), rnd(B * N, E, seed=16), rnd(B * M, E, seed=17)
    out, lse = ops.attention_train_forward(q, k, v, B, M, N, heads)
    return list(ops.attention_train_backward(q, k, v, out, lse, dout, B, M, N, heads))


def dense_train(Cout, normed):
    def case(lib, L, ops):
        R, Cin = 130, 8
        x, W, bias, dy = rnd(R, Cin, seed=18), rnd(Cout, Cin, seed=19), rnd(Cout, seed=20), rnd(R, Cout, seed=21)
        if not normed:
            return list(ops._dense_backward_gemm(dy, x, W, True, True, True))
        gamma, beta = rnd(Cout, seed=22), rnd(Cout, seed=23)
        out, h, stats = ops.dense_train_forward(x, W, bias, gamma, beta, act=ops.ACT_RELU)
        dh, dgamma, dbeta = torch.full((R, Cout), -9.0, device=DEV), torch.full((Cout,), -9.0, device=DEV), torch.full((Cout,), -9.0, device=DEV)
        ws = fresh(lib.dpm_dense_train_workspace_bytes(R, Cin, Cout))
        L.check(lib.dpm_dense_train_backward_rows(ops._ptr(dy), ops._ptr(out), ops._ptr(h), ops._ptr(stats), ops._ptr(gamma), R, Cout,
                                                  ops.ACT_RELU, None, ops._ptr(dh), ops._ptr(dgamma), ops._ptr(dbeta), ops._ptr(ws),
                                                  ops._stream(dy)), "dpm_dense_train_backward_rows")
        return [dh, dgamma, dbeta] + list(ops._dense_backward_gemm(dh, x, W, True, True, True))
    return case


def case_group_train(lib, L, ops):
    B, N, S, K, Cout = 1, 64, 16, 16, 32
    P, xyz = rnd(B, N, Cout, seed=24), ball(B, N, seed=25)
    centers = xyz[:, :S].contiguous()
    idx = torch.randint(0, N, (B, S, K), generator=torch.Generator().manual_seed(26), dtype=torch.int32).to(DEV)
    W_rel, gamma, beta = rnd(Cout, 3, seed=27), rnd(Cout, seed=28), rnd(Cout, seed=29)
    out, slots = ops.group_train_forward(P, xyz, centers, idx, W_rel, gamma, beta, 2.0)
    return list(ops.group_train_backward(P, xyz, centers, idx, W_rel, gamma, 2.0, rnd(B, S, Cout, seed=30), slots))


def case_loop_pool(lib, L, ops):
    B, Lt, E = 2, 3, 256
    x, W1, b1, g = rnd(B * Lt, E, seed=31), rnd(E, E, seed=32, scale=0.1), rnd(E, seed=33), rnd(B, E, seed=34)
    return [ops.loop_pool_forward(x, B, Lt, W1, b1)] + list(ops.loop_pool_backward(x, B, Lt, W1, b1, g))


# ---- sampling and the scan filters --------------------------------------------------------------------------------------
def fps(N):
    def case(lib, L, ops):
        return list(ops.fps(ball(2, N, seed=35), i32([N, N - 5]), 8))
    return case


def case_voxel_sampler(lib, L, ops):
    return list(ops.voxel_sample(ball(2, 200, seed=36), torch.zeros(2, 200, dtype=torch.bool, device=DEV), 16))


def frames():
    """two frames of 200 points, a few metres across"""
    return [ball(200, seed=37) * 8.0, ball(200, seed=38) * 8.0]


def case_voxel_select(lib, L, ops):
    outs, cap, cells = [], 200, 4096   # 4096: the least max_cells the call takes
    for xyz in frames():
        idx, count = torch.arange(cap, device=DEV, dtype=torch.int32), i32([cap - 7])
        xo, io = torch.full((cap, 3), -9.0, device=DEV), torch.full((cap,), -9, device=DEV, dtype=torch.int32)
        status = torch.full((2,), -9, device=DEV, dtype=torch.int32)
        ws = fresh(lib.dpm_augment_workspace_bytes(cap, cells))
        L.check(lib.dpm_voxel_select(ops._ptr(xyz), ops._ptr(idx), ops._ptr(count), cap, 2.0, 1, cells, ops._ptr(xo), ops._ptr(io),
                                     ops._ptr(status), ops._ptr(ws), ops._stream(xyz)), "dpm_voxel_select")
        assert status.tolist()[1] == 0 and 0 < status.tolist()[0] <= cap
        outs += [xo, io, status]
    return outs


def case_ground_filter(lib, L, ops):
    outs, cap, img = [], 200, 16
    for xyz in frames():
        idx, count = torch.arange(cap, device=DEV, dtype=torch.int32), i32([cap - 7])
        xo, io = torch.full((cap, 3), -9.0, device=DEV), torch.full((cap,), -9, device=DEV, dtype=torch.int32)
        no = torch.full((1,), -9, device=DEV, dtype=torch.int32)
        ws = fresh(lib.dpm_augment_workspace_bytes(cap, img * img))
        L.check(lib.dpm_ground_filter(ops._ptr(xyz), ops._ptr(idx), ops._ptr(count), cap, img, img, 1.0, 0.5, 1, ops._ptr(xo),
                                      ops._ptr(io), ops._ptr(no), ops._ptr(ws), ops._stream(xyz)), "dpm_ground_filter")
        assert 0 <= int(no.item()) <= cap
        outs += [xo, io, no]
    return outs


def case_preprocess_scan(lib, L, ops):
    from deeppointmap_amd import preprocess
    outs = []
    for xyz in frames():
        pts, pad, idx = preprocess.preprocess_scan(xyz, voxel_size=1.0, min_dis=1.0, max_dis=60.0, ratio=60.0, return_index=True,
                                                   max_cells=4096)
        assert pts.shape[2] > 0
        outs += [pts, idx]
    return outs


# ---- evaluation, loop closure, registration -----------------------------------------------------------------------------
def case_scan_context_search(lib, L, ops):
    Q, D, K, rings, sectors = 2, 70, 2, 20, 60
    pcd = (ball(Q + D, 200, seed=39) * 40.0).transpose(1, 2).contiguous()
    _, norm, mask = ops.scan_context_build_batched(pcd, i32([200] * (Q + D)), rings, sectors, 40.0, 0.5, 2.0)
    return list(ops.scan_context_search(norm[:Q].contiguous(), mask[:Q].contiguous(), norm[Q:].contiguous(), mask[Q:].contiguous(),
                                        i32([D, D // 2]), K))


def case_distance_stats(lib, L, ops):
    M, C, P = 4097, 2, 5   # two blocks of points
    g = torch.Generator().manual_seed(40)
    dist = torch.rand(M, generator=g).to(DEV)
    surf = torch.randint(-1, P, (M,), generator=g, dtype=torch.int32).to(DEV)
    return [ops.distance_stats(dist, [0.1, 0.3, 0.5], 0.8, surf, i32([0, 1, 0, 1, 1, 0]), C)]


def case_cloud_nn(lib, L, ops):
    q, t = (ball(65, seed=41) * 4.0).t().contiguous(), (ball(300, seed=42) * 4.0).t().contiguous()
    return list(ops.cloud_nn(q, t, 1.0, (0.0, 0.0, 0.0)))


def pair_clouds():
    """two frames of 257 points (the second: the first, moved a little) and the two pairs between them"""
    a = ball(257, seed=43) * 5.0
    b = a + torch.tensor([0.05, -0.02, 0.01], device=DEV)
    return torch.stack([a.t(), b.t()]).contiguous(), i32([0, 1]), i32([1, 0])


def case_icp(lib, L, ops):
    pcd, src, dst = pair_clouds()
    init = torch.eye(4, dtype=torch.float64, device=DEV).repeat(2, 1, 1)
    return list(ops.icp_refine(pcd, i32([257, 250]), src, dst, init, [(1.0, 2), (0.5, 2)], metric=ops.ICP_POINT))


def case_infomat(lib, L, ops):
    pcd, src, dst = pair_clouds()
    Rt = torch.eye(4, device=DEV)[:3].reshape(1, 12).repeat(2, 1).contiguous()
    out = torch.full((2, 36), -9.0, device=DEV)
    ops.information_matrix_batched(pcd, src, dst, Rt, out, radius=1.0)
    return [out]


def case_local_map_register(lib, L, ops):
    cap, cap_vox, subdiv, voxel, origin = 257, 1024, 3, 1.0, (0.0, 0.0, 0.0)
    xyz = ball(cap, seed=44) * 5.0
    eye = torch.eye(4, dtype=torch.float64, device=DEV)
    table = ops.local_map_new(cap_vox, subdiv, DEV)
    ops.local_map_insert(table, cap_vox, subdiv, 0, voxel, origin, xyz, torch.arange(cap, device=DEV, dtype=torch.int32), i32([cap]), eye, 1,
                         0.0, 100.0)
    moved = (xyz + torch.tensor([0.05, -0.02, 0.01], device=DEV)).contiguous()
    return list(ops.local_map_register(table, cap_vox, subdiv, 0, voxel, origin, moved, i32([cap]), eye, [(1.0, 2), (0.5, 2)]))


# name -> (case, the entry points that must have received the workspace, bytes where Python sizes the workspace itself)
CASES = {
    "knn_hybrid": (case_knn_hybrid, ["dpm_knn_hybrid"], None),
    "knn_build_grid+prebuilt": (case_knn_prebuilt, ["dpm_knn_build_grid", "dpm_knn_hybrid_prebuilt"], None),
    "knn_self": (case_knn_self, ["dpm_knn_self"], None),
    "point_normals": (case_point_normals, ["dpm_point_normals"], None),
    "outlier_filter_dc": (case_outlier_filter_dc, ["dpm_outlier_filter_dc"], None),
    "lowpass_filter_dc": (case_lowpass_filter_dc, ["dpm_lowpass_filter_dc"], None),
    "reg_loss": (case_reg_loss, ["dpm_reg_loss_forward", "dpm_reg_loss_backward"], None),
    "match_topk": (case_match_topk, ["dpm_match_topk"], None),
    "dual_softmax_topk-64x64": (dual_softmax(64, 64), ["dpm_dual_softmax_topk"], None),
    "dual_softmax_topk-640x64-slabs": (dual_softmax(640, 64), ["dpm_dual_softmax_topk"], None),
    "dual_softmax_topk-1024x256-slabs+grid-topk": (dual_softmax(1024, 256), ["dpm_dual_softmax_topk"], None),
    "attention_split": (case_attention_split, ["dpm_attention_split"], None),
    "attention_train_backward": (case_attention_train, ["dpm_attention_train_backward"], None),
    "dense_train-normed-32": (dense_train(32, True), ["dpm_dense_train_backward_rows", "dpm_dense_train_backward_gemm"], None),
    "dense_train-plain-12": (dense_train(12, False), ["dpm_dense_train_backward_gemm"], None),
    "group_train_backward": (case_group_train, ["dpm_group_train_backward"], None),
    "loop_pool": (case_loop_pool, ["dpm_loop_pool_forward", "dpm_loop_pool_backward"], None),
    "fps_ex-16385-packing": (fps(16385), ["dpm_fps_ex"], None),
    "fps_ex-300-plain": (fps(300), ["dpm_fps_ex"], None),
    "voxel_sampler_select": (case_voxel_sampler, ["dpm_voxel_sampler_select"], None),
    "voxel_select": (case_voxel_select, ["dpm_voxel_select"], None),
    "ground_filter": (case_ground_filter, ["dpm_ground_filter"], None),
    "preprocess_scan": (case_preprocess_scan, ["dpm_preprocess_scan"], None),
    "scan_context_search": (case_scan_context_search, ["dpm_scan_context_search"], None),
    "distance_stats": (case_distance_stats, ["dpm_distance_stats"], None),
    "cloud_nn": (case_cloud_nn, ["dpm_cloud_nn"], None),
    "icp_refine_batched": (case_icp, ["dpm_icp_refine_batched"], None),
    "information_matrix_batched": (case_infomat, ["dpm_information_matrix_batched"], None),
    "local_map_register": (case_local_map_register, ["dpm_local_map_register"], 512 + 256 * ((257 + 255) // 256)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_workspace_stays_inside_its_bytes(api, monkeypatch, name):
    case, entry_points, nbytes = CASES[name]
    run_guarded(api, monkeypatch, case, entry_points, nbytes)
