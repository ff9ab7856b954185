"""Seeded INPUTS of the decoder training fixture (decoder_train_<case>.*.npz): every case is regenerated from its numpy seed
here; the fixture stores only what the reference answered.  Imported by tests/golden/make_golden_decoder_train.py (runs the
reference in fp32 and fp64), by the tests and by scripts/decoder_train_bench.py.  No reference code here.

Geometry: target tokens in a cube, a ground-truth pose (R, T) source -> target, source tokens that are jittered copies of
target tokens (taken back through the pose) or uniform.  Coordinates and poses are rounded to fp32 first, so the fp64 run sees
the same points.  `gap(case)` is the smallest relative distance of any candidate squared distance from eps_offset^2: the
generator asserts it is above 1e-4 in every case, so the pair list is the same in fp32 and fp64, on any device."""
from types import SimpleNamespace

import numpy as np

IN_CHANNEL, MODEL_CHANNEL = 128, 256
EPS_OFFSET = 2.0
SAMPLE_STRIDE = 16   # parameter gradients are stored as max, 2-norm and every 16th element from a seeded offset


def cfg(layers=1, eps_positive=1.0, offset_value="manhattan"):
    """the reference's `args`: Decoder reads args.decoder.* and args.loss.{tau, eps_offset}, RegistrationLoss args.loss.*"""
    return SimpleNamespace(
        decoder=SimpleNamespace(in_channel=IN_CHANNEL, model_channel=MODEL_CHANNEL, attention_layers=layers),
        loss=SimpleNamespace(tau=0.1, offset_value=offset_value, eps_positive=eps_positive, eps_offset=EPS_OFFSET,
                             lambda_p=1.0, lambda_c=1.0, lambda_o=1.0))


def _pose(rng, B, angle=0.4, shift=3.0):
    Rs, Ts = [], []
    for _ in range(B):
        ax = rng.standard_normal(3)
        ax /= np.linalg.norm(ax)
        a = rng.uniform(-angle, angle)
        Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        Rs.append(np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx)
        Ts.append(rng.uniform(-shift, shift, (3, 1)))
    return np.stack(Rs), np.stack(Ts)


def _make(seed, B, M, N, side=30.0, jitter=0.8, copies=0.6, len_s=None, len_d=None, masks=True):
    rng = np.random.default_rng(seed)
    R, T = _pose(rng, B)
    R, T = R.astype(np.float32).astype(np.float64), T.astype(np.float32).astype(np.float64)
    xd = rng.uniform(0, side, (B, 3, N))
    gs = rng.uniform(0, side, (B, 3, M))                  # source tokens in the target frame
    n = int(copies * M)
    for b in range(B):
        pick = rng.integers(0, N, n)
        gs[b, :, :n] = xd[b][:, pick] + rng.uniform(-jitter, jitter, (3, n))
    return _finish(rng, R, T, gs, xd, len_s, len_d, masks)


def _finish(rng, R, T, gs, xd, len_s=None, len_d=None, masks=True):
    B, _, M = gs.shape
    N = xd.shape[2]
    xs = np.einsum("bji,bjm->bim", R, gs - T)             # R^T (g - T)
    xs, xd = xs.astype(np.float32).astype(np.float64), xd.astype(np.float32).astype(np.float64)
    fs = rng.standard_normal((B, IN_CHANNEL, M)).astype(np.float32).astype(np.float64)
    fd = rng.standard_normal((B, IN_CHANNEL, N)).astype(np.float32).astype(np.float64)
    ps, pd = np.zeros((B, M), bool), np.zeros((B, N), bool)
    for b in range(B):
        if len_s is not None:
            ps[b, len_s[b]:] = True
        if len_d is not None:
            pd[b, len_d[b]:] = True
    return dict(src=np.concatenate([fs, xs], 1), dst=np.concatenate([fd, xd], 1), ps=ps if masks else None,
                pd=pd if masks else None, R=R, T=T)


def _no_pairs(seed, B=2, M=80, N=64):
    """target tokens on a 6 m lattice, every source token 2.3 to 2.8 m from one of them: nothing within eps_offset = 2, while the
    loss (eps_positive = 3) still finds its positives"""
    rng = np.random.default_rng(seed)
    R, T = _pose(rng, B)
    R, T = R.astype(np.float32).astype(np.float64), T.astype(np.float32).astype(np.float64)
    g = np.stack(np.meshgrid(*[np.arange(4) * 6.0] * 3, indexing="ij")).reshape(3, 64)[:, :N]
    xd = np.stack([g[:, rng.permutation(N)] for _ in range(B)])
    gs = np.empty((B, 3, M))
    for b in range(B):
        d = rng.standard_normal((3, M))
        gs[b] = xd[b][:, rng.integers(0, N, M)] + rng.uniform(2.3, 2.8, M) * d / np.linalg.norm(d, axis=0)
    return _finish(rng, R, T, gs, xd, len_s=[M - 7, M], len_d=[N, N - 5])


def _hubs(seed, B=1, M=160, N=144):
    """one source token within eps_offset of 40 target tokens and one target token within eps_offset of 48 source tokens,
    the rest as in _make"""
    c = _make(seed, B, M, N, side=40.0, masks=True)
    rng = np.random.default_rng(seed + 1000)
    C = IN_CHANNEL
    R, T = c["R"], c["T"]
    gs = np.einsum("bij,bjm->bim", R, c["src"][:, C:]) + T
    xd = c["dst"][:, C:].copy()
    hub_s, hub_d = gs[0, :, 5].copy(), xd[0, :, 9].copy()
    d = rng.standard_normal((3, 40))
    xd[0, :, 20:60] = hub_s[:, None] + rng.uniform(0.2, 1.7, 40) * d / np.linalg.norm(d, axis=0)
    d = rng.standard_normal((3, 48))
    gs[0, :, 30:78] = hub_d[:, None] + rng.uniform(0.2, 1.7, 48) * d / np.linalg.norm(d, axis=0)
    xs = np.einsum("bji,bjm->bim", R, gs - T).astype(np.float32).astype(np.float64)
    c["src"] = np.concatenate([c["src"][:, :C], xs], 1)
    c["dst"] = np.concatenate([c["dst"][:, :C], xd.astype(np.float32).astype(np.float64)], 1)
    return c


def cases():
    """name -> (inputs: src (B,131,M), dst (B,131,N) float64 holding fp32 values, ps / pd bool or None, R (B,3,3), T (B,3,1); cfg)"""
    return {
        "plain_256": (_make(11, 1, 256, 256, masks=False), cfg()),
        "masks_ragged": (_make(52, 2, 512, 256, side=20.0, len_s=[475, 362], len_d=[247, 156]), cfg()),   # K >= 1000
        "no_pairs": (_no_pairs(13), cfg(eps_positive=3.0)),
        "hubs": (_hubs(14), cfg(offset_value="euclidean")),
        "three_layers": (_make(15, 1, 96, 80, side=12.0, len_s=[90], len_d=[71]), cfg(layers=3)),
    }


def masks(inputs):
    """(ps, pd) with None replaced by all-False"""
    B, _, M = inputs["src"].shape
    N = inputs["dst"].shape[2]
    ps = inputs["ps"] if inputs["ps"] is not None else np.zeros((B, M), bool)
    pd = inputs["pd"] if inputs["pd"] is not None else np.zeros((B, N), bool)
    return ps, pd


def candidates(inputs, dtype=np.float32):
    """(dist2 (B,M,N) of the unpadded candidates in `dtype`, valid (B,M,N))"""
    C = IN_CHANNEL
    R, T = inputs["R"].astype(dtype), inputs["T"].astype(dtype)
    g = np.einsum("bij,bjm->bim", R, inputs["src"][:, C:].astype(dtype)) + T
    d = g[:, :, :, None] - inputs["dst"][:, C:].astype(dtype)[:, :, None, :]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    ps, pd = masks(inputs)
    return d2, ~ps[:, :, None] & ~pd[:, None, :]


def gap(inputs):
    """smallest |dist2 - eps_offset^2| / eps_offset^2 over the unpadded candidates (fp64)"""
    d2, valid = candidates(inputs, np.float64)
    e2 = EPS_OFFSET * EPS_OFFSET
    return float((np.abs(d2[valid] - e2) / e2).min())


def sample_offset(key):
    """the seeded start of a parameter tensor's strided gradient sample"""
    import zlib
    return zlib.crc32(key.encode()) % SAMPLE_STRIDE


def state_dict(c, dtype=None):
    """procedural decoder weights of a case's cfg (deeppointmap_amd.weights), as torch tensors"""
    from deeppointmap_amd.params import decoder_shapes
    from deeppointmap_amd.weights import procedural_state_dict
    sd = procedural_state_dict(decoder_shapes(c))
    return sd if dtype is None else {k: v.to(dtype) for k, v in sd.items()}


# ---- the fixture files: decoder_train_<case>.partNN.npz, each below 1 MiB -------------------------------------------------
PART_BYTES = 900 * 1024


def fixture_parts(name, here):
    import os
    return sorted(os.path.join(here, f) for f in os.listdir(here) if f.startswith(f"decoder_train_{name}.part") and f.endswith(".npz"))


def save_fixture(name, arrays, here):
    """arrays {key: ndarray} -> numbered part files; arrays larger than a part are cut along their flat index ("key#i")"""
    import json
    import os
    for f in fixture_parts(name, here):
        os.remove(f)
    manifest, pieces = {}, []
    for k, a in arrays.items():
        a = np.ascontiguousarray(a)
        per = max(1, PART_BYTES // max(a.itemsize, 1))
        flat = a.reshape(-1)
        n = max(1, -(-flat.size // per))
        manifest[k] = [list(a.shape), n]
        for i in range(n):
            pieces.append((f"{k}#{i}", flat[i * per:(i + 1) * per]))
    parts, cur, size = [], {}, 0
    for k, a in pieces:
        if cur and size + a.nbytes > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = a
        size += a.nbytes
    parts.append(cur)
    parts[0]["manifest"] = np.frombuffer(json.dumps(manifest).encode(), dtype=np.uint8)
    total = 0
    for i, p in enumerate(parts):
        path = os.path.join(here, f"decoder_train_{name}.part{i:02d}.npz")
        np.savez_compressed(path, **p)
        assert os.path.getsize(path) < (1 << 20), path
        total += os.path.getsize(path)
    return len(parts), total


def load_fixture(name, here):
    """-> {key: ndarray}; "<key>/64" is rebuilt from the stored fp32 run and the stored difference (fp64 run - fp32 run)"""
    import json
    raw = {}
    for f in fixture_parts(name, here):
        with np.load(f) as z:
            raw.update({k: z[k] for k in z.files})
    manifest = json.loads(bytes(raw.pop("manifest")).decode())
    out = {}
    for k, (shape, n) in manifest.items():
        out[k] = np.concatenate([raw[f"{k}#{i}"] for i in range(n)]).reshape(shape)
    for k in [k for k in out if k.endswith("/d64")]:
        base = k[:-4]
        out[base + "/64"] = out[base + "/32"].astype(np.float64) + out.pop(k).astype(np.float64)
    return out


OUT_KEYS = ("src_pairing", "dst_pairing", "src_coarse", "dst_coarse", "src_res", "dst_res")
