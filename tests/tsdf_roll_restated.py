"""Rolling the TSDF map restated in numpy (dpm_tsdf_evict, dpm_tsdf_absorb; include/dpm_hip.h is the rule, DESIGN §7l "Rolling
the map"): the tile test in float32 with every operation rounded once, the evict partition and the absorb merge on exported
records (keys int64, sums int64, counts uint32).  Written from the rule, not from deeppointmap_amd/tsdf.py, whose own numpy
form (tile_of, tile_near, merge_records) tests/test_tsdf_roll_host.py compares with this one.

Three mutants of the tile test, each a plausible slip, which tests/tsdf_roll_cases.py must tell from the true form:
  voxel_centre   the voxel's own centre in place of its tile's;
  strict         `<` in place of `<=`;
  unbiased       the tile taken from the UNBIASED coordinate with C's division (towards zero): the tiles left of the bias shift
                 by one tile side.  (With a flooring shift the unbiased form is the true one: 2^20 is a multiple of 2^b.)
"""
import numpy as np

BIAS = 1 << 20
AXIS = (1 << 21) - 1
MUTANTS = ("voxel_centre", "strict", "unbiased")
f32 = np.float32


def axes(keys):
    k = np.asarray(keys, np.int64)
    return [(k >> (21 * a)) & AXIS for a in range(3)]


def pack(x, y, z):
    return np.asarray(x, np.int64) | (np.asarray(y, np.int64) << 21) | (np.asarray(z, np.int64) << 42)


def tile_keys(keys, b):
    x, y, z = axes(keys)
    return pack(x >> b, y >> b, z >> b)


def centres(keys, b, voxel, mutant=None):
    """per axis, float32: the centre of the tile of every voxel key"""
    v, out = f32(voxel), []
    for idx in axes(keys):
        if mutant == "voxel_centre":
            out.append(((idx - BIAS).astype(f32) + f32(0.5)) * v)
            continue
        if mutant == "unbiased":
            u = idx - BIAS
            first = np.sign(u) * ((np.abs(u) >> b) << b)
        else:
            first = ((idx >> b) << b) - BIAS
        out.append((first.astype(f32) + f32(0.5) * f32(1 << b)) * v)
    return out


def near(keys, b, voxel, origin, pose, radius, mutant=None):
    """per voxel key: its tile is NEAR the pose"""
    P, o = np.asarray(pose, np.float64).reshape(4, 4), np.asarray(origin, np.float64).reshape(3)
    t = (P[:3, 3] - o).astype(f32)                       # (float)(pose[3 | 7 | 11] - origin)
    r2 = f32(float(radius) * float(radius))
    c = centres(keys, b, voxel, mutant)
    d = [c[a] - t[a] for a in range(3)]
    dist = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    return dist < r2 if mutant == "strict" else dist <= r2


def sort_records(keys, sums, counts):
    k = np.asarray(keys, np.int64).reshape(-1)
    order = np.argsort(k, kind="stable")
    return k[order], np.asarray(sums, np.int64).reshape(-1)[order], np.asarray(counts, np.uint32).reshape(-1)[order]


def evict(records, b, voxel, origin, pose, radius, mutant=None):
    """records with unique keys -> (kept, out), each sorted by key: out holds the voxels of the tiles that are not near"""
    k, s, c = sort_records(*records)
    assert len(np.unique(k)) == len(k)
    keep = near(k, b, voxel, origin, pose, radius, mutant)
    return (k[keep], s[keep], c[keep]), (k[~keep], s[~keep], c[~keep])


def absorb(table, records):
    """table: records with unique keys; records: any -> (the table after, sorted by key; records whose key has bit 63 set).  A
    record with count 0 is skipped; equal keys add, sums modulo 2^64 and counts modulo 2^32 as the device's integers do."""
    held = {int(k): [int(s), int(c)] for k, s, c in zip(*table)}
    outside = 0
    for k, s, c in zip(np.asarray(records[0]).astype(np.int64).tolist(), np.asarray(records[1], np.int64).tolist(),
                       np.asarray(records[2]).astype(np.uint32).tolist()):
        if k < 0:
            outside += 1
            continue
        if c == 0:
            continue
        e = held.setdefault(k, [0, 0])
        e[0], e[1] = e[0] + s, e[1] + c
    ks = sorted(held)
    sums = np.array([((held[k][0] + (1 << 63)) % (1 << 64)) - (1 << 63) for k in ks], np.int64)
    counts = np.array([held[k][1] % (1 << 32) for k in ks], np.uint32)
    return (np.array(ks, np.int64), sums, counts), outside


def same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))
