"""Numpy restatement of csrc/scan_context.hip, in float32 and float64.

`build(..., dtype=np.float32)` mirrors the kernel's arithmetic operation by operation and must equal it BIT FOR BIT: every
product and sum below is one rounded float32 operation, as the device's are (the library is built with -ffp-contract=off).
The float64 build uses the same fp32 tables, so it differs only by the rounding of the arithmetic.  `search` is the plain
triple loop over (query, row, shift); its float32 form rounds every operation but does not claim the device's bits (there the
dot product is an fma chain), so the GPU search is compared with the float64 form within a bound.
"""
import numpy as np


def tables(rings, sectors, max_range):
    """the host tables, formed in float64 and rounded once (ops.scan_context_tables restated)"""
    m = np.arange(1, rings + 1, dtype=np.float64)
    ring_e2 = ((m * float(max_range) / rings) ** 2).astype(np.float32)
    a = 2.0 * np.pi * np.arange(1, sectors // 2, dtype=np.float64) / sectors
    return ring_e2, np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32)


def build(xyz, count, rings, sectors, max_range, min_range, z_offset, dtype=np.float32, tabs=None):
    """xyz (cap,3) float32 -> raw (rings,sectors), normalised (rings,sectors) of `dtype`, mask (python int)"""
    ring_e2, cs = tables(rings, sectors, max_range) if tabs is None else tabs
    f = dtype
    ring_e2, cs = ring_e2.astype(f), cs.astype(f)
    min_r2 = f(np.float32(float(min_range) * float(min_range)))
    zoff = f(np.float32(z_offset))
    raw = np.zeros((rings, sectors), f)
    xyz = np.asarray(xyz, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(max(0, min(int(count), len(xyz)))):
            x, y, z = (f(v) for v in xyz[i])
            if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
                continue
            r2 = f(f(x * x) + f(y * y))
            if r2 == 0 or not (r2 >= min_r2 and r2 < ring_e2[rings - 1]):
                continue
            ring = int(np.count_nonzero(r2 >= ring_e2[:rings - 1]))
            half = 0 if (y > 0 or (y == 0 and x > 0)) else 1
            if half:
                x, y = f(-x), f(-y)
            k = 0
            for m in range(sectors // 2 - 1):
                k += 1 if f(f(cs[m, 0] * y) - f(cs[m, 1] * x)) >= 0 else 0
            h = f(z + zoff)
            if not h > 0:
                continue
            c = half * (sectors // 2) + k
            raw[ring, c] = max(raw[ring, c], h)
    return (raw,) + finish(raw, dtype)


def finish(raw, dtype=np.float32):
    f = dtype
    rings, sectors = raw.shape
    norm = np.zeros((rings, sectors), f)
    mask = 0
    for j in range(sectors):
        n2 = f(0)
        for r in range(rings):
            n2 = f(n2 + f(raw[r, j] * raw[r, j]))
        n = f(np.sqrt(n2))
        if n > 0:
            for r in range(rings):
                norm[r, j] = f(raw[r, j] / n)
            mask |= 1 << j
    return norm, mask


def mask_to_int64(mask):
    """the python-int mask as the signed 64-bit value the tensors hold"""
    return mask - (1 << 64) if mask >> 63 else mask


def pair_distances(Aq, mq, Ac, mc, dtype=np.float64):
    """d(s) for s = 0 .. sectors-1 of one pair, by the definition: the plain loops"""
    f = dtype
    rings, sectors = Aq.shape
    out = np.zeros(sectors, f)
    for s in range(sectors):
        used, S = 0, f(0)
        for j in range(sectors):
            jj = (j + s) % sectors
            if (mq >> j) & 1 and (mc >> jj) & 1:
                used += 1
            dot = f(0)
            for r in range(rings):
                dot = f(dot + f(f(Aq[r, j]) * f(Ac[r, jj])))
            S = f(S + dot)
        out[s] = max(f(f(1) - f(S / f(used))), f(0)) if used else f(1)
    return out


def pair_distances_fast(Aq, mq, Ac, mc, dtype=np.float64):
    """the same numbers as pair_distances in float64 up to summation order (used where the triple loop is too slow to run
    for every case; tests pin it to pair_distances)"""
    rings, sectors = Aq.shape
    G = Aq.astype(dtype).T @ Ac.astype(dtype)                     # (j, j')
    j = np.arange(sectors)
    bq = np.array([(mq >> t) & 1 for t in range(sectors)], bool)
    bc = np.array([(mc >> t) & 1 for t in range(sectors)], bool)
    out = np.zeros(sectors, dtype)
    for s in range(sectors):
        jj = (j + s) % sectors
        used = int(np.count_nonzero(bq & bc[jj]))
        S = G[j, jj].sum(dtype=dtype)
        out[s] = max(dtype(1) - S / dtype(used), dtype(0)) if used else dtype(1)
    return out


def search(q_norm, q_mask, db_norm, db_mask, limits, K, dtype=np.float64, distances=pair_distances):
    """-> dist (Q,K) of dtype, row (Q,K), shift (Q,K): the K smallest (d, row) per query, ties to the smaller shift inside a
    pair and to the smaller row between pairs, padded with (inf, -1, -1)"""
    Q, D = len(q_norm), len(db_norm)
    dist = np.full((Q, K), np.inf, dtype)
    row = np.full((Q, K), -1, np.int64)
    shift = np.full((Q, K), -1, np.int64)
    for q in range(Q):
        lim = max(0, min(int(limits[q]), D))
        per_row = [distances(q_norm[q], int(q_mask[q]), db_norm[c], int(db_mask[c]), dtype) for c in range(lim)]
        best = []
        for c, d in enumerate(per_row):
            s = int(np.argmin(d))            # the first among equal: the smaller shift
            best.append((d[s], c, s))
        best.sort(key=lambda t: (t[0], t[1]))
        for k, (d, c, s) in enumerate(best[:K]):
            dist[q, k], row[q, k], shift[q, k] = d, c, s
    return dist, row, shift


def roll_columns(A, mask, m):
    """the descriptor turned by m columns: new column j = old column (j - m) % sectors, so that query `A` matches the turned
    copy at shift m (query column j <-> candidate column j + m)"""
    sectors = A.shape[1]
    B = np.roll(A, m, axis=1)
    bits = [(mask >> t) & 1 for t in range(sectors)]
    nm = 0
    for j in range(sectors):
        nm |= bits[(j - m) % sectors] << j
    return B, nm


def random_descriptors(rng, n, rings, sectors, occupancy=0.6, height=20.0, empty_columns=5):
    """n random raw descriptors (float32) with `empty_columns` empty columns each -> raw (n,rings,sectors)"""
    raw = (rng.random((n, rings, sectors)) * height).astype(np.float32)
    raw *= rng.random((n, rings, sectors)) < occupancy
    for i in range(n):
        raw[i][:, rng.choice(sectors, size=min(empty_columns, sectors), replace=False)] = 0
    return raw
