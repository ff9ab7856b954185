"""Meshing beyond the table restated in numpy, written from the contract (include/dpm_hip.h: dpm_tsdf_mesh_indexed,
dpm_tsdf_surface_tiles; DESIGN §7l "Meshing beyond the table"): the yardstick of tests/test_gpu_tsdf_mesh.py, shown on the CPU
by tests/test_tsdf_mesh_host.py.  Everything is built on tests/tsdf_restated.py as it is (Grid, mesh, surface, _grad).

  tile_of          a voxel key's tile, by coordinates
  needed_keys      brute force: per owned base voxel its 64 offsets k0 + {lo .. hi}^3 (the contract: lo, hi = -1, 2); a thinner
                   halo (lo = 0, or hi = 1) is the MUTANT a test has to tell from the true form
  base_keys        the cell a triangle of tsdf_restated.mesh came from
  vertex_normals   the normal of a vertex (key of p, direction): surface()'s rule on the edge p - q, float32 or float64
  indexed          tsdf_restated.mesh -> (vertices, faces, normals, keys, dirs) in weld's order, optionally of owned cells only
  batch_mesh       one batch of the out-of-core mesh: the field of the needed records only, its owned triangles and normals
  merge            batches merged by vertex name; soup: an indexed mesh back as triangles
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lidar_odometry_restated as L  # noqa: E402
import tsdf_restated as R  # noqa: E402

F32 = np.float32
BITS = (1, 2, 4, 3, 5, 6, 7)      # q ^ p of direction 0 .. 6
AXIS = (1 << 21) - 1


def coords(keys):
    """biased coordinates (n,3) of voxel (or tile) keys"""
    k = np.asarray(keys, np.int64).reshape(-1)
    return np.stack([(k >> (21 * a)) & AXIS for a in range(3)], axis=1)


def pack(xyz):
    x = np.asarray(xyz, np.int64).reshape(-1, 3)
    return x[:, 0] | (x[:, 1] << 21) | (x[:, 2] << 42)


def tile_of(keys, b):
    return pack(coords(keys) >> int(b))


def needed_keys(all_keys, owner_tiles, b, lo=-1, hi=2):
    """the keys among `all_keys` that the cells and crossings anchored in the owner tiles read -> sorted.  Brute force: every
    one of the 2^(3b) lattice positions of an owner tile is a base voxel k0 (the halo is defined by tiles, not by what they
    hold), and k0 + d for the (hi - lo + 1)^3 offsets d is listed (64 for the contract's -1 .. 2) when it lies inside the 21
    bits."""
    all_keys = np.asarray(all_keys, np.int64)
    side = np.arange(1 << int(b))
    cell = np.stack(np.meshgrid(side, side, side, indexing="ij"), -1).reshape(-1, 3)
    base = ((coords(np.unique(np.asarray(owner_tiles, np.int64))) << int(b))[:, None, :] + cell[None, :, :]).reshape(-1, 3)
    want = []
    span = range(lo, hi + 1)
    for dx in span:
        for dy in span:
            for dz in span:
                x = base + np.array([dx, dy, dz])
                ok = np.all((x >= 0) & (x <= AXIS), axis=1)
                want.append(np.intersect1d(pack(x[ok]), all_keys))
    return np.unique(np.concatenate(want))


def base_keys(vertex_keys):
    """triangles' vertex keys (n,3) -> the key k0 of the cell each came from.  The three edges of a triangle end in all four
    corners of its tetrahedron (one corner against three: its three edges; two against two: A-P, A-Q, B-Q or A-P, B-Q, B-P),
    corner 0 of the cell is one of them and, holding no bit, is the p end of its edge: k0 is the smallest of the three keys."""
    return np.asarray(vertex_keys, np.int64).reshape(-1, 3).min(axis=1)


def vertex_normals(fld, vertex_keys, vertex_dirs, dtype=F32):
    """fld = (keys, D) in `dtype` -> (V,3): for the edge between p and q = p + bits(direction), g = grad(p) + grad(q) per axis,
    divided by sqrt((gx*gx + gy*gy) + gz*gz) where that is > 0, else zeros: tsdf_restated.surface's lines"""
    dt = dtype
    G = R.Grid(*fld)
    out = np.zeros((len(vertex_keys), 3), dt)
    with np.errstate(all="ignore"):
        for i, (key, d) in enumerate(zip(np.asarray(vertex_keys).tolist(), np.asarray(vertex_dirs).tolist())):
            x0 = L.unpack_key(key)
            x1 = x0 + np.array([BITS[d] & 1, (BITS[d] >> 1) & 1, BITS[d] >> 2])
            g0, g1 = R._grad(G, x0, G.value(x0), dt), R._grad(G, x1, G.value(x1), dt)
            g = [dt(g0[b] + g1[b]) for b in range(3)]
            ln = np.sqrt(dt(dt(g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]))
            out[i] = [dt(gb / ln) if ln > 0 else dt(0) for gb in g]
    return out


def weld_named(tk, td, tp):
    """triangles by vertex names -> (vertices, faces, keys, dirs) in weld's order: vertices sorted by (key, direction), a face
    rotated so that its smallest index leads, faces sorted by row.  Written apart from deeppointmap_amd.tsdf.weld."""
    names = sorted(set(zip(np.asarray(tk).reshape(-1).tolist(), np.asarray(td).reshape(-1).tolist())))
    index = {n: i for i, n in enumerate(names)}
    where = {}
    for k, d, p in zip(np.asarray(tk).reshape(-1).tolist(), np.asarray(td).reshape(-1).tolist(), np.asarray(tp).reshape(-1, 3)):
        where.setdefault((k, d), p)
    faces = []
    for ks, ds in zip(np.asarray(tk).reshape(-1, 3).tolist(), np.asarray(td).reshape(-1, 3).tolist()):
        f = [index[(k, d)] for k, d in zip(ks, ds)]
        j = f.index(min(f))
        faces.append(f[j:] + f[:j])
    faces.sort()
    return (np.array([where[n] for n in names], F32).reshape(-1, 3), np.array(faces, np.int32).reshape(-1, 3),
            np.array([n[0] for n in names], np.int64), np.array([n[1] for n in names], np.int32))


def indexed(fld, voxel, owner_tiles=None, b=None, normals_from=None, dtype=F32):
    """-> (vertices, faces, normals, keys, dirs) of the field's mesh, of the cells anchored in the owner tiles only when given.
    normals_from: the field the normals read (default: fld)"""
    tk, td, tp = R.mesh(fld, voxel)
    if owner_tiles is not None:
        own = np.isin(tile_of(base_keys(tk), b), np.asarray(owner_tiles, np.int64)) if len(tk) else np.zeros(0, bool)
        tk, td, tp = tk[own], td[own], tp[own]
    v, f, k, d = weld_named(tk, td, tp)
    return v, f, vertex_normals(fld if normals_from is None else normals_from, k, d, dtype), k, d


def cut(exported, keys):
    """the records of `exported` (sorted by key) whose key is in `keys`"""
    keep = np.isin(exported[0], keys)
    return tuple(a[keep] for a in exported)


def batch_mesh(exported, voxel, owners, b, min_count=1, lo=-1, hi=2):
    """one batch of the out-of-core mesh: the field of `needed_keys` ALONE, the triangles of its owned cells and their normals read
    from that field alone -> (vertices, faces, normals, keys, dirs)"""
    return indexed(R.field(cut(exported, needed_keys(exported[0], owners, b, lo, hi)), min_count), voxel, owners, b)


def merge(parts):
    """batches merged by vertex name, the first of equal names kept -> (vertices, faces, normals), and the number of names that
    came with different bytes from two batches (the contract: none)"""
    clash, seen = 0, {}
    for v, f, n, k, d in parts:
        for name, pv, pn in zip(zip(k.tolist(), d.tolist()), v, n):
            held = seen.setdefault(name, (pv.tobytes(), pn.tobytes()))
            clash += held != (pv.tobytes(), pn.tobytes())
    names = sorted(seen)
    index = {n: i for i, n in enumerate(names)}
    faces = []
    for v, f, n, k, d in parts:
        local = [index[name] for name in zip(k.tolist(), d.tolist())]
        for row in f.tolist():
            g = [local[i] for i in row]
            j = g.index(min(g))
            faces.append(g[j:] + g[:j])
    faces.sort()
    vertices = np.frombuffer(b"".join(seen[n][0] for n in names), F32).reshape(-1, 3)
    normals = np.frombuffer(b"".join(seen[n][1] for n in names), F32).reshape(-1, 3)
    return vertices, np.array(faces, np.int32).reshape(-1, 3), normals, clash


def soup(part):
    """an indexed mesh (vertices, faces, normals, keys, dirs) back as triangles: (vertex keys, directions, positions)"""
    v, f, n, k, d = part
    return k[f], d[f], v[f]


# ------------------------------------------------------------------------------------------------------ a block of constructed voxels
def block_records(seed, side=6, corner=(5, -3, 6), missing=0.1, thin=0.1, zeros=4):
    """a side^3 block of voxels at (unbiased) `corner` with random values of either sign: `missing` of them left out, `thin` of
    them with count 1 (unqualified at min_count 2), a few with sum 0 (D == 0 counts as positive) -> (keys, sums, counts) in a
    random order, unique keys"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3) + np.asarray(corner) + L.BIAS
    n = len(g)
    sums = rng.integers(1 << 18, 1 << 24, n) * rng.choice([-1, 1], n)
    counts = rng.integers(2, 6, n).astype(np.uint32)
    role = rng.permutation(n)
    gone, weak = role[:int(missing * n)], role[int(missing * n):int((missing + thin) * n)]
    counts[weak] = 1
    sums[role[-zeros:]] = 0
    keep = np.setdiff1d(np.arange(n), gone)
    keep = keep[rng.permutation(len(keep))]
    return pack(g[keep]), sums[keep].astype(np.int64), counts[keep]


def block_coverage(fld):
    """what the cells of a field exercise -> (the set of (sign pattern of a tetrahedron's 4 corners, parity of its permutation)
    over the cells with 8 qualified corners, the set of corners m = 1 .. 7 that were the FIRST one missing of a cell)"""
    G = R.Grid(*fld)
    cases, exits = set(), set()
    for key in G.keys.tolist():
        x0 = L.unpack_key(key)
        D = [G.value(x0 + np.array([m & 1, (m >> 1) & 1, m >> 2])) for m in range(8)]
        gone = [m for m in range(8) if D[m] is None]
        if gone:
            exits.add(gone[0])
            continue
        for perm in R.PERMUTATIONS:
            m = [0, 1 << perm[0], (1 << perm[0]) | (1 << perm[1]), 7]
            cases.add((sum(int(D[m[i]] < 0) << i for i in range(4)), R._parity(perm)))
    return cases, exits
