"""Seeded INPUTS of the encoder training fixture (encoder_train_<case>.partNN.npz): every case is regenerated from its seed here;
the fixture stores only what the reference answered.  Imported by tests/golden/make_golden_encoder_train.py (runs the reference
Encoder in .train() mode in fp32 and fp64), by the tests and by scripts/encoder_train_bench.py.  No reference code here.

A case is a batch of synthetic LiDAR-like frames (deeppointmap_amd/synthetic.py, normalised coordinates) with per-frame valid
lengths (valid points lead, the rest is padding filled with zeros), the cotangent G of `fea` and a config.  The scalar that is
back-propagated is sum(fea * G * ~padding)."""
import json
import os
import zlib

import numpy as np

SAMPLE_STRIDE = 16   # large parameter gradients are stored as max, 2-norm and every 16th element from a seeded offset
WHOLE_BELOW = 4096   # ... smaller ones whole
PART_BYTES = 900 * 1024

# name -> (config, B, N, valid lengths, seed)
CASES = {
    "reduced_padded": ("reduced", 2, 4096, (4096, 3796), 21),      # 300 padded points on the second frame
    "default_8192": ("default", 1, 8192, (8192,), 22),
    "reduced_short": ("reduced", 2, 2048, (2048, 300), 23),        # a frame shorter than npoint[0] = 512: whole centre rows are padding
}


def cfg(name):
    from deeppointmap_amd.config import default_args, reduced_args
    return reduced_args() if CASES[name][0] == "reduced" else default_args()


def inputs(name):
    """-> points (B,3,N) float32, padding (B,N) bool, G (B,out_channel,S) float32 with S = the returned level's point count"""
    import torch
    from deeppointmap_amd import synthetic
    kind, B, N, lens, seed = CASES[name]
    c = cfg(name)
    base = synthetic.base_cloud(N, seed=seed)
    pts = torch.stack([synthetic.frame(3 * b, N, base) for b in range(B)]).numpy().astype(np.float32)
    pad = np.zeros((B, N), bool)
    for b, n in enumerate(lens):
        pad[b, n:] = True
        pts[b][:, n:] = 0.0
    enc = c.encoder
    S = enc.npoint[len(enc.npoint) - enc.upsample_layers - 1]
    G = np.random.default_rng(seed + 1000).standard_normal((B, enc.out_channel, S)).astype(np.float32)
    return pts, pad, G


def state_dict(c, dtype=None):
    """procedural encoder weights of a config (deeppointmap_amd.weights), as torch tensors"""
    from deeppointmap_amd.params import encoder_shapes
    from deeppointmap_amd.weights import procedural_state_dict
    sd = procedural_state_dict(encoder_shapes(c))
    return sd if dtype is None else {k: v.to(dtype) for k, v in sd.items()}


def sample_offset(key):
    return zlib.crc32(key.encode()) % SAMPLE_STRIDE


def grad_sample(key, g):
    """what the fixture keeps of a parameter gradient: the whole tensor when small, else the strided sample"""
    flat = np.asarray(g).reshape(-1)
    return flat if flat.size < WHOLE_BELOW else flat[sample_offset(key)::SAMPLE_STRIDE]


def fixture_parts(name, here):
    return sorted(os.path.join(here, f) for f in os.listdir(here) if f.startswith(f"encoder_train_{name}.part") and f.endswith(".npz"))


def save_fixture(name, arrays, here):
    """arrays {key: ndarray} -> numbered part files below 1 MiB; arrays larger than a part are cut along their flat index"""
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
        path = os.path.join(here, f"encoder_train_{name}.part{i:02d}.npz")
        np.savez_compressed(path, **p)
        assert os.path.getsize(path) < (1 << 20), path
        total += os.path.getsize(path)
    return len(parts), total


def load_fixture(name, here):
    """-> {key: ndarray}; "<key>/64" is rebuilt from the stored fp32 run and the stored difference (fp64 run - fp32 run)"""
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
        if base.startswith("win/"):
            out[base + "/64"] = out[base + "/32"] + out.pop(k)
        else:
            out[base + "/64"] = out[base + "/32"].astype(np.float64) + out.pop(k).astype(np.float64)
    return out
