"""GPU: the batched frame ingest (csrc/ingest.hip through ops.ingest_stage / ops.ingest_frames) against
PointCloud(reader's filtered array, capacity=cap), byte for byte in xyz (the whole buffer), idx and count."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def mods():
    from deeppointmap_amd import augment, dataset, ops
    return augment, dataset, ops


def records(n, stride, seed):
    """n records of `stride` floats with distinct, exactly representable values"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-(1 << 20), 1 << 20, size=(n, stride)).astype(np.float32) / 64).astype(np.float32)


def want_frame(augment, dataset, rows, drop_nan, cap):
    pcd = augment.PointCloud(dataset.filter_rows(rows, drop_nan)[:, :3], capacity=cap)
    return pcd.xyz.cpu().numpy(), pcd.idx.cpu().numpy(), pcd.count.cpu().numpy()


def ingest(ops, frames, cap):
    block = ops.ingest_stage(frames)
    xyz, idx, count = ops.ingest_frames(block, len(frames), cap, device=DEV)
    torch.cuda.synchronize()
    assert xyz.shape == (len(frames), cap, 3) and idx.shape == (len(frames), cap) and count.shape == (len(frames),)
    assert xyz.dtype == torch.float32 and idx.dtype == torch.int32 and count.dtype == torch.int32
    return xyz.cpu().numpy(), idx.cpu().numpy(), count.cpu().numpy()


def check(mods, frames, cap):
    augment, dataset, ops = mods
    xyz, idx, count = ingest(ops, frames, cap)
    for f, (rows, drop_nan) in enumerate(frames):
        wx, wi, wc = want_frame(augment, dataset, rows, drop_nan, cap)
        assert count[f] == wc[0], (f, count[f], wc)
        assert xyz[f].tobytes() == wx.tobytes(), f         # the whole buffer, bit for bit (NaN payloads included)
        assert np.array_equal(idx[f], wi), f
    return xyz, idx, count


def sizes(ops):
    C = ops.INGEST_CHUNK
    return C, [0, 1, 2, C - 1, C, C + 1, 2 * C + 1], 2 * C + 64      # the capacity is no multiple of the chunk


@pytest.mark.parametrize("stride,chunks", [(3, 3), (4, 3), (4, 65)], ids=["3", "4", "4-65chunks"])
def test_every_length_alone_and_in_one_batch(mods, stride, chunks):
    C, lengths, cap = sizes(mods[2])
    if chunks == 65:   # more than 64 chunks: the scan's one wave takes the chunk counts in two rounds and carries the sum over
        rows = records(64 * C + 1, stride, 9)
        rows[::1000, 1] = np.nan
        _, _, count = check(mods, [(rows, True)], 64 * C + 64)
        assert count[0] == rows.shape[0] - len(rows[::1000])
        return
    frames = [(records(n, stride, 10 + k), stride == 4) for k, n in enumerate(lengths)]
    for fr in frames:                                  # a batch of one frame
        check(mods, [fr], cap)
    _, _, count = check(mods, frames, cap)             # seven frames of different lengths in one batch
    assert count.tolist() == lengths


@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("col", [0, 1, 2])
def test_nan_rows_are_dropped_in_order(mods, stride, col):
    augment, dataset, ops = mods
    C, _, cap = sizes(ops)
    n = 2 * C + 1
    rows = records(n, stride, 20 + col)
    bad = [0, C - 1, C, n - 1]
    rows[bad, col] = np.nan
    xyz, idx, count = check(mods, [(rows, True)], cap)
    assert count[0] == n - 4
    assert np.array_equal(xyz[0, :n - 4], np.delete(rows, bad, axis=0)[:, :3])     # stable: the kept rows in input order
    assert not xyz[0, n - 4:].any() and np.array_equal(idx[0], np.arange(cap))
    # drop_nan = False keeps them
    xyz, _, count = check(mods, [(rows, False)], cap)
    assert count[0] == n and np.isnan(xyz[0, bad, col]).all()


def test_nan_intensity_keeps_the_row_and_all_nan_frame_is_empty(mods):
    augment, dataset, ops = mods
    C, _, cap = sizes(ops)
    rows = records(C + 5, 4, 31)
    rows[[0, 7, C, C + 4], 3] = np.nan
    _, _, count = check(mods, [(rows, True)], cap)
    assert count[0] == C + 5
    empty = np.full((C + 3, 4), np.nan, np.float32)
    empty[:, 3] = 1.0
    xyz, idx, count = check(mods, [(empty, True), (rows, True), (empty[:, :3].copy(), True)], cap)
    assert count.tolist() == [0, C + 5, 0] and not xyz[0].view(np.uint32).any() and not xyz[2].view(np.uint32).any()
    assert np.array_equal(idx[0], np.arange(cap))


def test_bits_survive(mods):
    """Inf, -0.0, a denormal and NaN payloads (in a kept row's other columns with drop_nan off) arrive bit for bit"""
    augment, dataset, ops = mods
    C, _, cap = sizes(ops)
    rows = records(C + 2, 4, 41)
    u = rows.view(np.uint32)
    u[1, 0], u[1, 1], u[1, 2] = 0x7F800000, 0xFF800000, 0x80000000        # +Inf, -Inf, -0.0
    u[C, 0], u[C, 1], u[C, 2] = 0x00000001, 0x807FFFFF, 0x00400000          # denormals
    xyz, _, count = check(mods, [(rows, True)], cap)
    assert count[0] == C + 2
    assert xyz[0].view(np.uint32)[1].tolist() == [0x7F800000, 0xFF800000, 0x80000000]
    assert xyz[0].view(np.uint32)[C].tolist() == [0x00000001, 0x807FFFFF, 0x00400000]
    u[2, 0], u[2, 1] = 0x7FC12345, 0xFFA00001                                # NaN payloads, quiet and signalling
    xyz, _, count = ingest(ops, [(rows, False)], cap)
    assert count[0] == C + 2 and xyz[0].view(np.uint32)[2, :2].tolist() == [0x7FC12345, 0xFFA00001]
    xyz, _, count = ingest(ops, [(rows, True)], cap)
    assert count[0] == C + 1 and xyz[0].view(np.uint32)[2].tolist() == u[3, :3].tolist()


def test_two_runs_give_identical_bytes(mods):
    augment, dataset, ops = mods
    C, lengths, cap = sizes(ops)
    frames = []
    for k, n in enumerate(lengths):
        rows = records(n, 4, 50 + k)
        rows[::7, k % 3] = np.nan
        frames.append((rows, True))
    a, b = ingest(ops, frames, cap), ingest(ops, frames, cap)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    check(mods, frames, cap)


def test_too_many_rows_raise_before_anything_is_queued(mods, monkeypatch):
    augment, dataset, ops = mods
    from deeppointmap_amd import _lib
    C, _, cap = sizes(ops)
    block = ops.ingest_stage([(records(5, 3, 1), False), (records(cap + 1, 4, 2), True)])
    called = []
    real = _lib.load().dpm_ingest_frames
    monkeypatch.setattr(ops._lib, "load", lambda: type("L", (), {"dpm_ingest_frames": staticmethod(lambda *a: called.append(a) or 0)})())
    with pytest.raises(ValueError, match="capacity"):
        ops.ingest_frames(block, 2, cap, device=DEV)
    assert not called                                   # the wrapper refused before the entry point was reached
    monkeypatch.undo()
    # the entry point itself refuses too (DPM_EINVAL), before its copy and its launches: the outputs stay untouched
    xyz = torch.full((2, cap, 3), 7.0, device=DEV)
    idx = torch.full((2, cap), 7, device=DEV, dtype=torch.int32)
    count = torch.full((2,), 7, device=DEV, dtype=torch.int32)
    ws = torch.zeros(2 * 3, device=DEV, dtype=torch.int32)
    dev_block = torch.zeros(block.numel(), device=DEV, dtype=torch.uint8)
    status = real(block.data_ptr(), dev_block.data_ptr(), block.numel(), 2, cap, C, xyz.data_ptr(), idx.data_ptr(),
                  count.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert status == -1
    assert bool((xyz == 7).all()) and bool((idx == 7).all()) and bool((count == 7).all()) and not bool(dev_block.any())
    assert real(block.data_ptr(), dev_block.data_ptr(), block.numel(), 2, cap + 1, C + 1, xyz.data_ptr(), idx.data_ptr(),
                count.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream) == -1     # another chunk size


def test_from_buffers_wraps_views_of_the_arena(mods):
    augment, dataset, ops = mods
    C, _, cap = sizes(ops)
    rows = [records(100, 3, 61), records(C + 9, 4, 62)]
    rows[1][5, 1] = np.nan
    block = ops.ingest_stage([(rows[0], False), (rows[1], True)])
    xyz, idx, count = ops.ingest_frames(block, 2, cap, device=DEV)
    R = np.eye(3, dtype=np.float64)[[1, 0, 2]]
    a = augment.PointCloud.from_buffers(xyz[0], idx[0], count[0:1], R, np.ones((3, 1), np.float32), host_n=100)
    b = augment.PointCloud.from_buffers(xyz[1], idx[1], count[1:2])
    assert a.xyz.data_ptr() == xyz.data_ptr() and a.cap == cap and a._host_n == 100 and b._host_n is None
    assert a.R.dtype == torch.float32 and torch.equal(a.R, torch.from_numpy(R).float()) and torch.equal(b.T, torch.zeros(3, 1))
    assert b.nbr_point == C + 8 and a.nbr_point == 100
    pts, _, _, pad, _ = augment.collate_frames([a, b], cap)
    assert np.array_equal(pts[0, :, :100].cpu().numpy().T, rows[0]) and int((~pad[1]).sum()) == C + 8
