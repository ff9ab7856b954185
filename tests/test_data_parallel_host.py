"""CPU: the flat gradient layout of deeppointmap_amd/data_parallel.py and the chunk table of its launches, the `DataParallel`
wrapper's state-dict keys, an inert `GradSync`, and the argument checks of the new C entry points (before any HIP call)."""
import numpy as np
import pytest
import torch

NUMELS = (1, 3, 4, 5, 4095, 4096, 4097)


def test_layout_offsets_are_aligned_disjoint_and_ordered():
    from deeppointmap_amd.data_parallel import flat_layout
    for numels in (NUMELS, NUMELS[::-1], (8193, 1, 1, 2, 7), (4,), ()):
        offsets, L = flat_layout(numels)
        assert len(offsets) == len(numels) and L % 4 == 0
        assert all(o % 4 == 0 for o in offsets)
        end = 0
        for o, n in zip(offsets, numels):   # in order, no overlap, at most 3 elements of padding behind a tensor
            assert end <= o <= end + 3
            end = o + n
        assert end <= L <= end + 3
        assert L == sum((n + 3) // 4 * 4 for n in numels)


def test_chunk_table_covers_each_element_exactly_once():
    from deeppointmap_amd import _lib
    from deeppointmap_amd.data_parallel import flat_layout
    from deeppointmap_amd.optim import chunk_table
    chunk = _lib.load().dpm_optim_chunk()
    assert chunk == 4096
    offsets, L = flat_layout(NUMELS)
    table = chunk_table(NUMELS, chunk)
    assert table.dtype == np.int32 and table.shape == (sum((n + chunk - 1) // chunk for n in NUMELS), 2)
    hits = np.zeros(L, np.int64)
    per_tensor = [np.zeros(n, np.int64) for n in NUMELS]
    for t, c in table:
        lo, hi = c * chunk, min(NUMELS[t], (c + 1) * chunk)
        assert 0 <= lo < hi
        per_tensor[t][lo:hi] += 1
        hits[offsets[t] + lo:offsets[t] + hi] += 1
    assert all((h == 1).all() for h in per_tensor)
    covered = np.zeros(L, bool)
    for o, n in zip(offsets, NUMELS):
        covered[o:o + n] = True
    assert np.array_equal(hits, covered.astype(np.int64))   # the padding belongs to no chunk


def test_data_parallel_wrapper_keys_and_module_round_trip():
    from deeppointmap_amd.data_parallel import DataParallel
    inner = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.LayerNorm(5))
    model = DataParallel(inner)
    assert model.module is inner
    assert list(model.state_dict()) == ["module." + k for k in inner.state_dict()]
    assert [id(p) for p in model.parameters()] == [id(p) for p in inner.parameters()]
    x = torch.randn(4, 3)
    assert torch.equal(model(x), inner(x))
    # the reference's add_module / remove_module key handling: a prefixed state dict loads into the wrapper, a stripped one into the module
    other = DataParallel(torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.LayerNorm(5)))
    other.load_state_dict(model.state_dict(), strict=True)
    stripped = {k[len("module."):]: v for k, v in model.state_dict().items()}
    other.module.load_state_dict(stripped, strict=True)
    assert all(torch.equal(a, b) for a, b in zip(other.module.state_dict().values(), inner.state_dict().values()))
    model.eval()
    assert not inner.training
    model.train()
    assert inner.training
    with pytest.raises(ValueError):
        DataParallel(inner, mode="ring")


def test_grad_sync_without_a_process_group_is_inert():
    from deeppointmap_amd import optim
    from deeppointmap_amd.data_parallel import GradSync
    lin = torch.nn.Linear(3, 5)
    frozen = torch.nn.Parameter(torch.zeros(7), requires_grad=False)
    sync = GradSync([lin.weight, frozen, lin.bias])
    assert not sync.active and sync.world == 1 and sync.rank == 0 and sync.plan_builds == 0
    assert [id(p) for p in sync.params] == [id(lin.weight), id(lin.bias)]       # the trainable ones, in iteration order
    assert sync.offsets == [0, 16] and sync.length == 24
    assert sync.offset_of(lin.bias) == 16 and sync.offset_of(frozen) is None
    sync.pack(), sync.exchange(), sync.broadcast_parameters()                      # CPU tensors, no library call: nothing happens
    assert sync.flat is None and sync.gathered is None and sync.plan_builds == 0
    assert GradSync([lin.weight, frozen], trainable_only=False).length == 16 + 8
    with pytest.raises(ValueError):
        GradSync(lin.parameters(), mode="ring")
    with pytest.raises(ValueError):
        GradSync([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))])
    # attached but inert: the optimiser keeps its plain step (here: it refuses CPU tensors as ever)
    opt = optim.AdamW(lin.parameters())
    opt.attach_grad_sync(sync)
    assert not opt._synced()
    opt.detach_grad_sync()
    with pytest.raises(ValueError):
        optim.SGD([lin.weight]).attach_grad_sync(sync)                             # the layout holds a tensor the optimiser does not


def test_invalid_arguments_return_einval_without_a_device():
    """every check of the new C entry points comes before the first HIP call"""
    from deeppointmap_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(64)
    p = buf.data_ptr()
    step = lambda algo=0, n_chunks=1, t=p, c=p, s=p, n_slices=1, stride=8, divisor=1.0, count=1.0: lib.dpm_optim_step_synced(   # noqa: E731
        algo, t, c, n_chunks, 1e-3, 0.9, 0.999, 1e-8, 0.0, count, 0.0, 0.0, 0, 0, s, n_slices, stride, divisor, None)
    assert step(n_slices=0) == -1
    assert step(n_slices=-2) == -1
    assert step(stride=6) == -1                  # not a multiple of 4
    assert step(stride=-4) == -1
    assert step(divisor=0.5) == -1
    assert step(divisor=0.0) == -1
    assert step(divisor=float("nan")) == -1
    assert step(algo=3) == -1
    assert step(n_chunks=-1) == -1
    assert step(t=None) == -1 and step(c=None) == -1 and step(s=None) == -1
    assert step(count=0.0) == -1                 # Adam's step count starts at 1
    assert step(n_chunks=0) == 0                 # nothing to launch
    assert step(n_chunks=0, n_slices=0) == -1    # ... but the arguments are still checked
    for fn in (lib.dpm_flat_pack, lib.dpm_flat_unpack):
        assert fn(p, p, -1, p, 8, None) == -1
        assert fn(p, p, 1, p, 6, None) == -1     # flat_len not a multiple of 4
        assert fn(p, p, 1, p, -4, None) == -1
        assert fn(None, p, 1, p, 8, None) == -1 and fn(p, None, 1, p, 8, None) == -1 and fn(p, p, 1, None, 8, None) == -1
        assert fn(p, p, 0, p, 8, None) == 0
