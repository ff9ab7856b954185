"""GPU: the data-parallel kernels of csrc/optim.hip -- dpm_flat_pack / dpm_flat_unpack and dpm_optim_step_synced.

Pack and unpack move bytes: the packed buffer equals the one torch builds, byte for byte.  The synced step is checked against
the project's own one-launch optimisers as the yardstick: the gradient the kernel has to form -- slice_0 + slice_1 + ... in
rank order, then a true division by W -- is computed on the CPU in numpy (fp32, sequential adds, IEEE division; torch's GPU
division by a Python scalar multiplies by a reciprocal and is no reference for W = 3), handed to an unattached optim.AdamW /
Adam / SGD on cloned parameters, and parameters and every state tensor must come out byte-equal, after one and after two steps.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NUMELS = (1, 3, 4, 5, 4095, 4096, 4097, 8193)
VIEW = 4       # NUMELS[VIEW] is a view one element into a larger buffer: 4-byte aligned only, the scalar path
NONE = 5       # NUMELS[NONE] has no gradient in the pack test


def _tensors(seed, fill=True):
    """the eight tensors on the GPU; tensor VIEW is a view at an odd element offset"""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for i, n in enumerate(NUMELS):
        t = (torch.randn(n, generator=gen) if fill else torch.zeros(n)).to(DEV)
        if i == VIEW:
            buf = torch.zeros(n + 8, device=DEV)
            buf[1:1 + n] = t
            t = buf[1:1 + n]
            assert t.data_ptr() % 16 == 4
        out.append(t)
    return out


def _plan(rows):
    from deeppointmap_amd import _lib
    from deeppointmap_amd.optim import _Plan
    return _Plan(rows, _lib.load().dpm_optim_chunk(), torch.device(DEV, torch.cuda.current_device()))


def _call(name, plan, flat):
    from deeppointmap_amd import _lib
    fn = getattr(_lib.load(), name)
    _lib.check(fn(plan.tensors_ptr, plan.chunks_ptr, plan.n_chunks, flat.data_ptr(), flat.numel(),
                  torch.cuda.current_stream().cuda_stream), name)


def test_pack_equals_the_torch_built_buffer_and_unpack_restores():
    from deeppointmap_amd.data_parallel import flat_layout
    offsets, L = flat_layout(NUMELS)
    src = _tensors(3)
    want = torch.zeros(L)
    for i, (t, o, n) in enumerate(zip(src, offsets, NUMELS)):
        if i != NONE:
            want[o:o + n] = t.cpu()
    plan = _plan([[0 if i == NONE else t.data_ptr(), o, n] for i, (t, o, n) in enumerate(zip(src, offsets, NUMELS))])
    flat = torch.zeros(L, device=DEV)
    _call("dpm_flat_pack", plan, flat)
    assert flat.cpu().numpy().tobytes() == want.numpy().tobytes()   # zeros in the padding and in the None region
    # a second pack over a buffer that held something else: every region is rewritten (the None one with zeros), the padding stays
    pad = torch.ones(L, dtype=torch.bool)
    for o, n in zip(offsets, NUMELS):
        pad[o:o + n] = False
    assert int(pad.sum()) == L - sum(NUMELS) > 0
    flat.fill_(7.0)
    _call("dpm_flat_pack", plan, flat)
    got = flat.cpu()
    assert torch.equal(got[~pad], want[~pad]) and bool((got[pad] == 7.0).all())
    # unpack into fresh tensors of the same shapes and alignments; the row with address 0 is skipped
    flat.copy_(want)
    dst = _tensors(0, fill=False)
    _call("dpm_flat_unpack", _plan([[0 if i == NONE else t.data_ptr(), o, n] for i, (t, o, n) in enumerate(zip(dst, offsets, NUMELS))]), flat)
    for i, (a, b) in enumerate(zip(dst, src)):
        assert torch.equal(a, torch.zeros_like(b) if i == NONE else b), i
    assert torch.equal(flat.cpu(), want)                           # unpack reads only
    # a row that does not fit the buffer moves nothing (the kernel checks it: no write beyond flat)
    small = torch.full((8,), 5.0, device=DEV)
    _call("dpm_flat_pack", _plan([[src[3].data_ptr(), 4, 5]]), small)
    assert bool((small == 5.0).all())


class _FixedSlices:
    """what an optimiser asks of an attached GradSync, over a buffer the test filled: the exchange already happened"""

    def __init__(self, params, offsets, buffer, n_slices, divisor):
        self.active, self.params = True, list(params)
        self._offset = {id(p): o for p, o in zip(params, offsets)}
        self._slices = (buffer, n_slices, buffer.shape[-1], float(divisor))
        self.packs = self.exchanges = 0

    def offset_of(self, p):
        return self._offset.get(id(p))

    def pack(self):
        self.packs += 1

    def exchange(self):
        self.exchanges += 1

    def slices(self):
        return self._slices


def _gathered(W, L, seed):
    """(W, L) fp32 on the CPU: magnitudes 1e-8 .. 1e4 (log-uniform), mixed signs"""
    gen = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(W, L, generator=gen, dtype=torch.float64) * 12.0 - 8.0)
    sign = torch.where(torch.rand(W, L, generator=gen) < 0.5, -1.0, 1.0)
    return (mag * sign).float()


def _ordered_mean(slices: np.ndarray, W: int) -> np.ndarray:
    g = slices[0].copy()
    for r in range(1, slices.shape[0]):
        g = g + slices[r]
    assert g.dtype == np.float32
    return g / np.float32(W)


OPTIMISERS = {
    "adamw": ("AdamW", dict(lr=1e-2, weight_decay=1e-2)),
    "adam_wd": ("Adam", dict(lr=1e-2, weight_decay=0.1, betas=(0.8, 0.99))),
    "sgd_nesterov": ("SGD", dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=0.05)),
    "sgd_plain": ("SGD", dict(lr=1e-2)),
}


def _params(seed):
    return [torch.nn.Parameter(t) for t in _tensors(seed)]


def _same(a_params, a_opt, b_params, b_opt, what):
    for i, (a, b) in enumerate(zip(a_params, b_params)):
        assert a.detach().cpu().numpy().tobytes() == b.detach().cpu().numpy().tobytes(), (what, "param", i)
        sa, sb = a_opt.state.get(a, {}), b_opt.state.get(b, {})
        assert sorted(sa) == sorted(sb), (what, i)
        for k in sa:
            va, vb = sa[k], sb[k]
            assert (va.detach().cpu().numpy().tobytes() == vb.detach().cpu().numpy().tobytes()) if torch.is_tensor(va) else va == vb, (what, k, i)


@pytest.mark.parametrize("W", [1, 2, 3, 8, 11])   # 11 = a full batch of eight slices and a remainder: the kernel's other path
@pytest.mark.parametrize("name", list(OPTIMISERS))
def test_synced_step_equals_the_plain_step_on_the_ordered_mean(name, W):
    """Two steps (the second exercises the bias correction and SGD's `first` flag), fresh slices each.  For W >= 3 the inputs
    are first shown to be order-sensitive: the same slices summed in reverse rank order differ somewhere, so a kernel that adds
    in another order fails.  (For W <= 2 no such input exists: a + b = b + a in IEEE arithmetic.)"""
    from deeppointmap_amd import optim
    from deeppointmap_amd.data_parallel import flat_layout
    cls, kw = getattr(optim, OPTIMISERS[name][0]), OPTIMISERS[name][1]
    offsets, L = flat_layout(NUMELS)
    want_p, got_p = _params(11), _params(11)
    want_opt, got_opt = cls(want_p, **kw), cls(got_p, **kw)
    buffer = torch.zeros(W, L, device=DEV)
    sync = _FixedSlices(got_p, offsets, buffer, W, W)
    got_opt.attach_grad_sync(sync)
    for step in (1, 2):
        slices = _gathered(W, L, seed=100 * W + step)
        s = slices.numpy()
        g = _ordered_mean(s, W)
        if W >= 3:
            assert np.any(_ordered_mean(s[::-1], W) != g), "the inputs must make the order of the sum visible"
        buffer.copy_(slices)
        for p, o, n in zip(want_p, offsets, NUMELS):
            p.grad = torch.from_numpy(g[o:o + n].copy()).to(DEV)
        want_opt.step()
        got_opt.step()
        assert sync.packs == sync.exchanges == step
        _same(want_p, want_opt, got_p, got_opt, f"{name} W{W} step {step}")
        assert all(p.grad is None for p in got_p)   # the synced step neither needs nor writes p.grad
    assert got_opt.plan_builds <= 2                   # SGD with momentum: the `first` launch and the later ones


@pytest.mark.parametrize("W", [2, 3, 8])
def test_one_presummed_slice_with_divisor_w(W):
    """all-reduce mode: n_slices = 1, divisor = W on the pre-summed buffer is the same recipe"""
    from deeppointmap_amd import optim
    from deeppointmap_amd.data_parallel import flat_layout
    offsets, L = flat_layout(NUMELS)
    want_p, got_p = _params(12), _params(12)
    want_opt, got_opt = optim.AdamW(want_p, lr=1e-2), optim.AdamW(got_p, lr=1e-2)
    buffer = torch.zeros(1, L, device=DEV)
    got_opt.attach_grad_sync(_FixedSlices(got_p, offsets, buffer, 1, W))
    for step in (1, 2):
        total = _gathered(1, L, seed=7 * W + step)
        g = total.numpy()[0] / np.float32(W)
        buffer.copy_(total)
        for p, o, n in zip(want_p, offsets, NUMELS):
            p.grad = torch.from_numpy(g[o:o + n].copy()).to(DEV)
        want_opt.step(), got_opt.step()
        _same(want_p, want_opt, got_p, got_opt, f"allreduce W{W} step {step}")


def test_detached_optimiser_is_the_plain_one_again():
    from deeppointmap_amd import optim
    from deeppointmap_amd.data_parallel import flat_layout
    offsets, L = flat_layout(NUMELS)
    a_p, b_p = _params(13), _params(13)
    a, b = optim.SGD(a_p, lr=0.1, momentum=0.5), optim.SGD(b_p, lr=0.1, momentum=0.5)
    b.attach_grad_sync(_FixedSlices(b_p, offsets, torch.zeros(1, L, device=DEV), 1, 1))
    b.detach_grad_sync()
    for p, q in zip(a_p, b_p):
        p.grad = torch.ones_like(p)
        q.grad = torch.ones_like(q)
    a.step(), b.step()
    _same(a_p, a, b_p, b, "detached")
