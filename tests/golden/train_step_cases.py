"""Seeded INPUTS of the training-step fixture (train_step_<case>.npz): every case is regenerated from its numpy seed here; the
fixture stores only what the reference answered (and the refined-SE3 dictionary as arrays, so that a test can write the pickle
the pipeline reads).  Imported by tests/golden/make_golden_train_step.py (runs the reference's _train_registration in fp32 and
fp64 on stand-in modules) and by the tests.  No reference code here.

A case is what the stand-in encoder returns for F = B * S frames -- coor (F,3,N) unscaled, fea (F,C,N), mask (F,N) -- plus the
batch's global poses R (F,3,3), T (F,3,1), calib (F,4,4), the frame numbers pcd_index (B,S), one refined-SE3 dictionary and
per map whether it reads that dictionary (file name '' = no dictionary: the whole map takes the global poses).  All floats are
rounded to fp32 first, so the fp64 run sees the same numbers."""
import os

import numpy as np

COOR_SCALE = 60          # configs: slam_system.coor_scale
MAP_SIZE_MAX = 8         # train.registration.map_size_max unless the case says otherwise
KEYS = ("src_desc", "dst_desc", "gt", "src_global", "dst_global")    # recorded in fp32 and fp64
METRIC_KEYS = ("loss_regis", "loss_p", "loss_c", "loss_o", "top1_acc", "offset_err")


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _rot(rng, max_angle):
    """a rotation by up to max_angle (rad) about a random axis (Rodrigues), float64"""
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(-max_angle, max_angle)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def _se3(rng, max_angle, max_t):
    M = np.eye(4)
    M[:3, :3] = _rot(rng, max_angle)
    M[:3, 3] = rng.uniform(-max_t, max_t, 3)
    return M


def _make(seed, B, S, N, C, pcd_index, keys, files, calib_identity, map_size_max=MAP_SIZE_MAX, seeds=(0,)):
    rng = np.random.default_rng(seed)
    F = B * S
    coor = rng.uniform(-1.0, 1.0, (F, 3, N))
    fea = rng.standard_normal((F, C, N))
    mask = rng.random((F, N)) < 0.2
    mask[:, 0] = False
    R = np.stack([_rot(rng, np.pi) for _ in range(F)])
    T = rng.uniform(-30.0, 30.0, (F, 3, 1))
    calib = np.stack([np.eye(4) if calib_identity else _se3(rng, 0.5, 1.5) for _ in range(F)])
    values = np.stack([_se3(rng, 0.3, 4.0) for _ in keys]) if len(keys) else np.zeros((0, 4, 4))
    pcd_index = np.asarray(pcd_index, np.int64).reshape(B, S)
    return dict(B=B, S=S, N=N, C=C, map_size_max=map_size_max, seeds=tuple(seeds),
                coor=_f32(coor), fea=_f32(fea), mask=mask, R=_f32(R), T=_f32(T), calib=_f32(calib), pcd_index=pcd_index,
                dict_keys=np.asarray(keys, np.int64).reshape(-1, 2), dict_values=values, uses_dict=tuple(bool(f) for f in files))


def cases():
    """name -> inputs.  `seeds`: the values random.seed() takes, one recorded run each (fixture keys "<seed>/...")."""
    # case (b), frame numbers per map and what the dictionary holds for them:
    #   map 0: [20, 23, 21, 20, 26]  (23,20) direct as (20,23); 21 < 23 reversed as (21,23); 20 == 20 repeated; 26 -> 21 only
    #          or 23 over the bridge 20 ((20,26) with (20,21) / (20,23)): the dictionary has no (23,26)
    #   map 1: [40, 37, 44, 41, 39]  every pair direct or reversed except those of frame 39, which no key names: missing outright,
    #          with and without the bridge 40 -> the global poses
    #   map 2: no dictionary
    b_keys = [(20, 23), (21, 23), (20, 26), (20, 21), (20, 20), (21, 26),
              (37, 40), (40, 44), (40, 41), (37, 44), (37, 41), (41, 44)]
    return {
        "a": _make(31, 1, 2, 256, 128, [7, 9], [], [""], True),
        "b": _make(32, 3, 5, 37, 5, [20, 23, 21, 20, 26, 40, 37, 44, 41, 39, 3, 4, 5, 6, 7], b_keys, ["d", "d", ""], False,
                   seeds=(0, 1, 5)),   # S1 = 4 (second draw), 1 (first draw), 3
        "c": _make(33, 2, 7, 16, 8, [5, 6, 7, 8, 9, 10, 11, 50, 49, 48, 47, 46, 45, 44],
                   [(5, 6), (5, 7), (8, 9), (8, 10), (5, 8), (49, 50), (46, 47), (45, 47), (47, 50)], ["d", "d"], False,
                   map_size_max=4, seeds=(0, 1)),
    }


def se3_dict(inputs):
    return {(int(k[0]), int(k[1])): v.copy() for k, v in zip(inputs["dict_keys"], inputs["dict_values"])}


def info(inputs, dict_file):
    """the `info` of a batch as the reference's collate makes it (the fields _train_registration reads)"""
    return {"num_map": inputs["B"], "dsf_index": [(0, 0, int(i)) for i in inputs["pcd_index"].reshape(-1)],
            "refined_SE3_file": [dict_file if u else "" for u in inputs["uses_dict"]]}


def fixture_path(name, here):
    return os.path.join(here, f"train_step_{name}.npz")


def load_fixture(name, here):
    """-> {key: ndarray}; "<key>/64" is rebuilt from the stored fp32 run and the stored difference (fp64 run - fp32 run)"""
    with np.load(fixture_path(name, here)) as z:
        raw = {k.replace("|", "/"): z[k] for k in z.files}
    for k in [k for k in raw if k.endswith("/d64")]:
        base = k[:-4]
        raw[base + "/64"] = raw[base + "/32"].astype(np.float64) + raw.pop(k).astype(np.float64)
    return raw
