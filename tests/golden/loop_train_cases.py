"""Seeded INPUTS of the loop-detection training fixture (loop_train_<case>.partNN.npz): every case is regenerated from its numpy
seed here; the fixture stores only what the reference answered.  Imported by tests/golden/make_golden_loop_train.py (runs the
reference in fp32 and fp64), by the tests and by scripts/loop_train_bench.py.  No reference code here.

Descriptors, padding masks, cfg and weights are those of decoder_train_cases; a case adds the two frame positions src_T, dst_T
(B,3,1) whose distance decides the label (a pair is a loop when it is at most DISTANCE).  Positions are rounded to fp32 first,
so the fp64 run sees the same points; `gap(case)` is the smallest | ||src_T - dst_T|| - DISTANCE | / DISTANCE, which the
generator asserts to be above 1e-4: the labels are the same in fp32 and fp64, on any device."""
import json
import os
from types import SimpleNamespace

import numpy as np

import decoder_train_cases as D

DISTANCE = 10.0
SAMPLE_STRIDE = D.SAMPLE_STRIDE
HEAD = tuple(f"loop_head.{k}.{w}" for k in ("mlp.0", "mlp.2", "projection.0", "projection.2") for w in ("weight", "bias"))
SAMPLED = ("loop_head.mlp.0.weight", "loop_head.mlp.2.weight", "loop_head.projection.0.weight")   # stored as samples
WHOLE = tuple(k for k in HEAD if k not in SAMPLED)                                                  # stored whole


def cfg(layers=1):
    c = D.cfg(layers)
    c.train = SimpleNamespace(loop_detection=SimpleNamespace(distance=DISTANCE))
    return c


def _positions(seed, labels):
    """labels: 1 = within DISTANCE (1 to 8 m apart), 0 = beyond (12 to 40 m)"""
    rng = np.random.default_rng(seed)
    B = len(labels)
    src_T = rng.uniform(-100.0, 100.0, (B, 3, 1))
    d = rng.standard_normal((B, 3, 1))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.array([rng.uniform(1.0, 8.0) if l else rng.uniform(12.0, 40.0) for l in labels]).reshape(B, 1, 1)
    dst_T = src_T + r * d
    f = lambda a: a.astype(np.float32).astype(np.float64)   # noqa: E731
    return f(src_T), f(dst_T)


def _case(seed, labels, M, N, layers=1, **kw):
    inputs = D._make(seed, len(labels), M, N, **kw)
    inputs["src_T"], inputs["dst_T"] = _positions(seed + 500, labels)
    inputs["labels"] = np.array(labels, bool)
    return inputs, cfg(layers)


def cases():
    """name -> (inputs: decoder_train_cases' src, dst, ps, pd plus src_T, dst_T (B,3,1) and the intended labels (B,); cfg)"""
    return {
        "pairs_256": _case(21, [1, 0, 0, 1], 256, 256, masks=False),
        "ragged": _case(22, [0, 1, 1], 250, 77, layers=3, side=20.0, len_s=[250, 201, 133], len_d=[60, 77, 41]),
        "all_negative": _case(23, [0, 0], 96, 80, side=12.0, len_s=[90, 96], len_d=[80, 71]),
        "all_positive": _case(24, [1, 1], 96, 80, side=12.0, len_s=[96, 85], len_d=[75, 80]),
    }


masks = D.masks
state_dict = D.state_dict
sample_offset = D.sample_offset


def distances(inputs, dtype=np.float64):
    return np.linalg.norm((inputs["src_T"].astype(dtype) - inputs["dst_T"].astype(dtype))[:, :, 0], axis=1)


def gap(inputs):
    return float((np.abs(distances(inputs) - DISTANCE) / DISTANCE).min())


# ---- the fixture files: loop_train_<case>.partNN.npz, each below 1 MiB -------------------------------------------------------
PART_BYTES = 900 * 1024


def fixture_parts(name, here):
    return sorted(os.path.join(here, f) for f in os.listdir(here) if f.startswith(f"loop_train_{name}.part") and f.endswith(".npz"))


def save_fixture(name, arrays, here):
    """arrays {key: ndarray} -> numbered part files (no array of this fixture is larger than a part)"""
    for f in fixture_parts(name, here):
        os.remove(f)
    parts, cur, size = [], {}, 0
    for k, a in arrays.items():
        a = np.ascontiguousarray(a)
        assert a.nbytes <= PART_BYTES, k
        if cur and size + a.nbytes > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k.replace("/", "|")] = a
        size += a.nbytes
    parts.append(cur)
    parts[0]["manifest"] = np.frombuffer(json.dumps(sorted(arrays)).encode(), dtype=np.uint8)
    total = 0
    for i, p in enumerate(parts):
        path = os.path.join(here, f"loop_train_{name}.part{i:02d}.npz")
        np.savez_compressed(path, **p)
        assert os.path.getsize(path) < (1 << 20), path
        total += os.path.getsize(path)
    return len(parts), total


def load_fixture(name, here):
    """-> {key: ndarray}; "<key>/64" is rebuilt from the stored fp32 run and the stored difference (fp64 run - fp32 run)"""
    raw = {}
    for f in fixture_parts(name, here):
        with np.load(f) as z:
            raw.update({k.replace("|", "/"): z[k] for k in z.files})
    keys = json.loads(bytes(raw.pop("manifest")).decode())
    assert sorted(raw) == keys, "fixture parts are missing"
    for k in [k for k in raw if k.endswith("/d64")]:
        base = k[:-4]
        raw[base + "/64"] = raw[base + "/32"].astype(np.float64) + raw.pop(k).astype(np.float64)
    return raw


METRIC_KEYS = ("loss_loop", "loop_precision", "loop_recall", "loop_false_positive")
