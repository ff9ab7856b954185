"""The fused tail of a decoder block (csrc/gemm_b3.hip, decoder_tail_b3_kernel; ops.decoder_tail, Decoder._block_tail) against the
three launches it replaces -- ops.linear_layernorm, ops.linear (ReLU), ops.linear_layernorm with the knob off -- bit for bit,
and the entry point's argument checks on the host."""
import threading

import pytest
import torch

DEV = "cuda:0"
C = 256


@pytest.fixture(scope="module")
def ops():
    from deeppointmap_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def layers():
    """random weights of one block tail from a fixed seed: (Wo, bo, g2, be2, W0, b0, W2, b2, g3, be3)"""
    gen = torch.Generator(device=DEV).manual_seed(2024)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=gen)   # noqa: E731
    Wo, W0, W2 = (rnd(C, C) / C ** 0.5 for _ in range(3))
    bo, b0, b2, be2, be3 = (rnd(C) for _ in range(5))
    g2, g3 = 1 + 0.5 * rnd(C), 1 + 0.5 * rnd(C)
    return Wo, bo, g2, be2, W0, b0, W2, b2, g3, be3


def _three_calls(ops, a, z1, L, post):
    Wo, bo, g2, be2, W0, b0, W2, b2, g3, be3 = L
    z2 = ops.linear_layernorm(a, Wo, bo, g2, be2, pre=z1)
    h = ops.linear(z2, W0, b0, act=ops.ACT_RELU)
    return ops.linear_layernorm(h, W2, b2, g3, be3, pre=z2, post=post)


def _lift_row_window(monkeypatch, ops):
    """small inputs reach the fused kernels (ops.linear_layernorm and ops.decoder_tail share the window)"""
    monkeypatch.setattr(ops, "FUSED_LN_MIN_ROWS", 0)


@pytest.fixture(scope="module")
def rows():
    """a, z1, post for the largest row count, shared by the cases below (smaller cases take its leading rows)"""
    gen = torch.Generator(device=DEV).manual_seed(7)
    return tuple(torch.randn(640, C, device=DEV, generator=gen) for _ in range(3))


@pytest.mark.gpu
@pytest.mark.parametrize("R", [8, 64, 72, 640])       # less than a tile, one tile, a ragged last tile, several tiles
@pytest.mark.parametrize("use_post", [False, True])
@pytest.mark.parametrize("use_bias", [False, True])
def test_tail_equals_the_three_launches(ops, layers, rows, monkeypatch, R, use_post, use_bias):
    from deeppointmap_amd import knobs
    _lift_row_window(monkeypatch, ops)
    a, z1, post = (t[:R].contiguous() for t in rows)
    post = post if use_post else None
    L = list(layers)
    if not use_bias:
        L[1] = L[5] = L[7] = None
    monkeypatch.setattr(knobs, "DECODER_TAIL_FUSED", False)
    assert ops.decoder_tail(a, z1, *L, post) is None
    want = _three_calls(ops, a, z1, L, post)
    monkeypatch.setattr(knobs, "DECODER_TAIL_FUSED", True)
    z1_before = z1.clone()
    got = ops.decoder_tail(a, z1, *L, post)
    assert got is not None and got.shape == want.shape
    assert torch.equal(got, want)
    assert torch.equal(z1, z1_before)      # the decoder's form: `out` is a tensor of its own, the inputs stay as they are


@pytest.mark.gpu
def test_tail_row_scales_and_the_eps_path(ops, layers, rows, monkeypatch):
    """rows scaled by 1e3 and by 1e-6 and an all-zero row (a = z1 = 0: LayerNorm's variance is the bias row's alone; with no
    biases the row is constant and only eps keeps rsqrt finite)"""
    from deeppointmap_amd import knobs
    _lift_row_window(monkeypatch, ops)
    a, z1, post = (t[:72].clone() for t in rows)
    a[3] *= 1e3
    z1[3] *= 1e3
    a[10] *= 1e-6
    z1[10] *= 1e-6
    a[64:70] *= 1e3
    a[70] *= 1e-6
    z1[70] *= 1e-6
    a[17] = 0
    z1[17] = 0
    a[71] = 0
    z1[71] = 0
    for use_bias in (True, False):
        L = list(layers)
        if not use_bias:
            L[1] = L[5] = L[7] = None
        monkeypatch.setattr(knobs, "DECODER_TAIL_FUSED", False)
        want = _three_calls(ops, a, z1, L, post)
        monkeypatch.setattr(knobs, "DECODER_TAIL_FUSED", True)
        got = ops.decoder_tail(a, z1, *L, post)
        assert got is not None and torch.isfinite(got).all()
        assert torch.equal(got, want), use_bias


@pytest.mark.gpu
def test_tail_unsupported_shapes_fall_back(ops, layers, rows, monkeypatch, cfg_full):
    """C = 128 and an `a` whose rows start 4 bytes off a 16-byte boundary are not the kernel's: the wrapper says None (the entry
    point DPM_EUNSUPPORTED) and Decoder._block_tail gives the three launches' rows"""
    from deeppointmap_amd import _lib
    _lift_row_window(monkeypatch, ops)
    gen = torch.Generator(device=DEV).manual_seed(5)
    a, z1, post = (t[:72].contiguous() for t in rows)
    # another width
    L128 = [torch.randn(128, 128, device=DEV, generator=gen) / 128 ** 0.5 if i in (0, 4, 6) else torch.randn(128, device=DEV, generator=gen)
            for i in range(10)]
    a128, z128 = a[:, :128].contiguous(), z1[:, :128].contiguous()
    assert ops.decoder_tail(a128, z128, *L128, None) is None
    # the entry point itself: an X pointer 4 bytes off, and C = 128
    Wo, bo, g2, be2, W0, b0, W2, b2, g3, be3 = layers
    planes = [ops._weight_planes(W) for W in (Wo, W0, W2)]
    out = torch.empty_like(a)
    buf = torch.zeros(72 * C + 4, device=DEV)
    a_off = buf[1:1 + 72 * C].view(72, C)
    a_off.copy_(a)

    def call(ap, Cc):
        (po, oo, no), (p0, o0, n0), (p2, o2, n2) = planes
        return _lib.load().dpm_decoder_tail_bf16x3(ap, z1.data_ptr(), post.data_ptr(), out.data_ptr(), 72, Cc, po.data_ptr() + 2 * oo, no,
                                                   bo.data_ptr(), g2.data_ptr(), be2.data_ptr(), p0.data_ptr() + 2 * o0, n0, b0.data_ptr(),
                                                   p2.data_ptr() + 2 * o2, n2, b2.data_ptr(), g3.data_ptr(), be3.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream)
    assert call(a_off.data_ptr(), C) == -2
    assert call(a.data_ptr(), 128) == -2
    assert call(a.data_ptr(), C) == 0 and torch.equal(out, _three_calls(ops, a, z1, layers, post))
    # the helper, on a decoder's own block 0: the kernel refused (rows of `a` 260 floats apart) -> the fallback's rows
    from deeppointmap_amd.decoder import Decoder
    from deeppointmap_amd.weights import init_procedural
    dec = init_procedural(Decoder(cfg_full)).to(DEV)
    pre = "descriptor_attention.0"
    wide = torch.zeros(72, C + 4, device=DEV)
    a_str = wide[:, :C]
    a_str.copy_(a)
    calls = []
    real = ops.decoder_tail
    monkeypatch.setattr(ops, "decoder_tail", lambda *args: calls.append(real(*args)) or calls[-1])
    got = dec._block_tail(pre, a_str, z1, post)
    assert calls == [None]
    z2 = dec._lin_ln(pre + ".cross_attn.out_proj", pre + ".norm2", a_str, z1)
    want = dec._lin_ln(pre + ".mlp.2", pre + ".norm3", dec._lin(pre + ".mlp.0", z2, ops.ACT_RELU), z2, post)
    assert torch.equal(got, want)
    fused = dec._block_tail(pre, a, z1, post)
    assert calls[-1] is not None and torch.equal(fused, want)


@pytest.mark.gpu
def test_registration_forward_knob_on_off_and_graph_replay(ops, cfg_full, monkeypatch):
    """registration_forward on two pairs of 256-token descriptors (the joint forward), one 256 x 128 pair (the stacked forward) and
    the two-sided loop: R, T, rmse, the inlier confidences and their count are the same bits with the fused tail and with the three
    launches; a pair replayed through its captured graph equals the eager call."""
    from deeppointmap_amd import knobs
    from deeppointmap_amd.decoder import Decoder
    from deeppointmap_amd.weights import init_procedural
    _lift_row_window(monkeypatch, ops)
    dec = init_procedural(Decoder(cfg_full)).to(DEV)
    dec.graph_min_hits = 0
    gen = torch.Generator().manual_seed(23)

    def desc(M):
        return torch.cat([torch.rand(128, M, generator=gen), 60 * torch.randn(3, M, generator=gen)]).to(DEV)
    used = []
    real = ops.decoder_tail
    monkeypatch.setattr(ops, "decoder_tail", lambda *args: used.append(real(*args)) or used[-1])

    def same(x, y):
        return torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[2], y[2]) and x[3] == y[3] and x[2].numel() == y[2].numel()
    pairs = [(desc(256), desc(256)), (desc(256), desc(256)), (desc(256), desc(128))]
    for i, (s, d) in enumerate(pairs):
        for stack in ((True, False) if i == 2 else (True,)):
            dec.stack_sides = stack
            monkeypatch.setattr(knobs, "DECODER_TAIL_FUSED", False)
            off = dec.registration_forward(s, d, num_sample=0.5)
            assert all(u is None for u in used)
            monkeypatch.setattr(knobs, "DECODER_TAIL_FUSED", True)
            del used[:]
            on = dec.registration_forward(s, d, num_sample=0.5)
            assert len(used) == dec.attention_layers * (1 if stack else 2) and all(u is not None for u in used)
            del used[:]
            assert same(on, off), (i, stack)
    dec.stack_sides = True
    # the captured graph of the 256 x 256 shape
    s, d = pairs[0]
    eager = dec.registration_forward(s, d, num_sample=0.5)
    dec.graph_min_hits = 2
    replays = [dec.registration_forward(s, d, num_sample=0.5) for _ in range(4)]
    if threading.active_count() == 1:      # (graphs are only captured in single-threaded processes, decoder.py)
        assert dec.captured(256, 256)
    assert all(same(r, eager) for r in replays)
    dec.graph_min_hits = 0


# ---- host: argument checks of the entry point (nothing is launched: every call below returns before the launch) and its binding row
def test_entry_point_argument_checks_need_no_gpu():
    import ctypes
    from deeppointmap_amd import _lib
    lib = _lib.load()
    keep = [(ctypes.c_char * 64)() for _ in range(16)]
    al = [ctypes.addressof(k) + (-ctypes.addressof(k)) % 16 for k in keep]     # 16-byte aligned, never dereferenced
    n = 256 * 256

    def call(a=al[0], pre=al[1], post=al[2], out=al[3], R=64, Cc=256, wo=al[4], po=n, bo=al[5], g2=al[6], be2=al[7], w0=al[8], p0=n,
             b0=al[9], w2=al[10], p2=n, b2=al[11], g3=al[12], be3=al[13]):
        return lib.dpm_decoder_tail_bf16x3(a, pre, post, out, R, Cc, wo, po, bo, g2, be2, w0, p0, b0, w2, p2, b2, g3, be3, None)
    for bad in (dict(a=None), dict(pre=None), dict(out=None), dict(wo=None), dict(w0=None), dict(w2=None), dict(g2=None), dict(be2=None),
                dict(g3=None), dict(be3=None), dict(R=0), dict(Cc=0), dict(po=n - 1), dict(p0=n - 1), dict(p2=n - 1), dict(out=al[0])):
        assert call(**bad) == -1, bad
    for unsupported in (dict(Cc=128, po=n, p0=n, p2=n), dict(Cc=512, po=4 * n, p0=4 * n, p2=4 * n), dict(a=al[0] + 4), dict(pre=al[1] + 8),
                        dict(post=al[2] + 4), dict(out=al[3] + 4), dict(wo=al[4] + 2), dict(bo=al[5] + 4), dict(g3=al[12] + 4),
                        dict(po=n + 4), dict(p2=n + 2)):
        assert call(**unsupported) == -2, unsupported


def test_signature_row_and_knob():
    from deeppointmap_amd import _lib, knobs
    I, P, LL = _lib.I, _lib.P, _lib.LL
    assert _lib.SIGNATURES["dpm_decoder_tail_bf16x3"] == (I, [P, P, P, P, I, I, P, LL, P, P, P, P, LL, P, P, LL, P, P, P, P])
    assert knobs.DECODER_TAIL_FUSED is True and knobs._ENV["DPM_DECODER_TAIL"][0] == "DECODER_TAIL_FUSED"
    assert knobs._ENV["DPM_DECODER_TAIL"][1]("0") is False and knobs._ENV["DPM_DECODER_TAIL"][1]("1") is True
