"""The information matrix (csrc/infomat.hip) restated in plain numpy for inputs on a dyadic lattice, where it is EXACT.

The kernel sums the matched target coordinates as 64-bit integers rint(v * 2^qexp), converts the ten sums to fp64 and rounds
once to fp32.  With every coordinate a multiple of 2^-s (s <= qexp), a power-of-two radius and a pose that is a signed
permutation plus a lattice translation, nothing before that final rounding rounds at all: the fp32 distance
(dx^2 + dy^2) + dz^2 is an exact integer multiple of 4^-s, equal distances are bit-equal and "on the radius" means
d^2 == r^2.  The expected matrix is then float32(exact value) and a test compares raw bits -- one wrong neighbour moves a first
moment by at least one lattice step, which the sizing rule below keeps visible in fp32.

Search: brute force in fp64 over integer lattice units (every intermediate is an integer below 2^53, so fp64 is exact); the
match is the smallest d^2, then the smallest original target index -- the kernel's (distance bits, index) key, and what
np.argmin returns; kept when d^2 <= r^2.  Nothing of the code under test is used."""
import numpy as np

CHUNK = 512  # queries per brute-force block


def to_lattice(a, s, what="input"):
    """float array of multiples of 2^-s -> int64 lattice units (asserts that it is on the lattice)"""
    v = np.asarray(a, dtype=np.float64) * float(1 << s)
    q = np.rint(v)
    assert np.array_equal(v, q), f"{what} is not on the 2^-{s} lattice"
    return q.astype(np.int64)


def radius_units(radius, s):
    """the radius in lattice units; it must be a power of two (so that (float)(r * r) is exact) of at least one step"""
    m, _ = np.frexp(float(radius))
    assert m == 0.5, f"radius {radius} is not a power of two"
    r = float(radius) * (1 << s)
    assert r == int(r) and r >= 1, f"radius {radius} is below the lattice step 2^-{s}"
    return int(r)


def pose_units(Rt, s):
    """Rt (>=12,) [R row-major, T] -> (R int64 (3,3), T int64 (3,)); R must be a signed permutation, T on the lattice"""
    Rt = np.asarray(Rt, dtype=np.float64)
    R = Rt[:9].reshape(3, 3)
    assert np.isin(R, (-1.0, 0.0, 1.0)).all() and (np.abs(R).sum(0) == 1).all() and (np.abs(R).sum(1) == 1).all(), \
        "the pose is not a signed permutation"
    return R.astype(np.int64), to_lattice(Rt[9:12], s, "translation")


def moments_of(t):
    """(..., 3) int64 points -> (..., 10) int64: 1, x, y, z, xx, yy, zz, xy, xz, yz"""
    x, y, z = t[..., 0], t[..., 1], t[..., 2]
    return np.stack([np.ones_like(x), x, y, z, x * x, y * y, z * z, x * y, x * z, y * z], -1)


def matrix_from_moments(m, s, exact=True):
    """(..., 10) integer moments in lattice units -> (..., 6, 6) float32: the 36 entries in fp64, rounded once.
    exact=False lifts the bound that makes the fp64 image of the moments exact (comparisons at a tolerance only)"""
    m = np.asarray(m)
    assert not exact or (np.abs(m.astype(object)) < (1 << 53)).all(), "a moment reaches 2^53 lattice units: its fp64 value is not exact"
    m = m.astype(np.float64)
    u, u2 = 2.0 ** -s, 4.0 ** -s
    n, x, y, z = m[..., 0], m[..., 1] * u, m[..., 2] * u, m[..., 3] * u
    xx, yy, zz, xy, xz, yz = (m[..., k] * u2 for k in range(4, 10))
    o = np.zeros_like(n)
    G = np.stack([zz + yy, -xy, -xz, o, -z, y,
                  -xy, zz + xx, -yz, z, o, -x,
                  -xz, -yz, yy + xx, -y, x, o,
                  o, z, -y, n, o, o,
                  -z, o, x, o, n, o,
                  y, -x, o, o, o, n], -1)
    return G.reshape(m.shape[:-1] + (6, 6)).astype(np.float32)


def restate(pcd1, pcd2, Rt, radius, s, exact=True):
    """pcd1 (3, N1) queries, pcd2 (3, N2) targets, Rt (>=12,), all on the 2^-s lattice -> dict
      G        (6, 6) float32, exactly what the kernel must return
      moments  (10,) Python ints in lattice units
      match    (N1,) original target index of the kept match, -1 where there is none
      d2       (N1,) squared distance to the nearest target, lattice units
      second   (N1,) nearest target at ANOTHER POSITION than the match, smallest index among equals; -1 where it is not
               within the radius (or the query has no match).  A target that coincides with the match is the same answer:
               it has the same moments
      tied     (N1,) bool: two or more targets at distinct positions share the smallest distance, within the radius
      q, t     the transformed queries / the targets in lattice units, (N, 3) int64
    exact=False: see matrix_from_moments; the search is exact either way."""
    q0 = to_lattice(np.asarray(pcd1).T, s, "pcd1")
    t = to_lattice(np.asarray(pcd2).T, s, "pcd2")
    R, T = pose_units(Rt, s)
    q = q0 @ R.T + T
    r2 = radius_units(radius, s) ** 2
    N1, N2 = len(q), len(t)
    _, pos = np.unique(t, axis=0, return_inverse=True)  # position id: coincident targets share one
    pos = pos.reshape(-1)
    tf = t.astype(np.float64)
    tt = (tf * tf).sum(1)
    match, d2 = np.empty(N1, np.int64), np.empty(N1, np.int64)
    second, tied = np.full(N1, -1, np.int64), np.zeros(N1, bool)
    for c in range(0, N1, CHUNK):
        qf = q[c:c + CHUNK].astype(np.float64)
        d = (qf * qf).sum(1)[:, None] + tt[None, :] - 2.0 * (qf @ tf.T)  # integers below 2^53: exact
        assert d.max() < 2.0 ** 53
        ar = np.arange(len(qf))
        best = d.argmin(1)                                               # smallest d^2, then smallest index
        bd = d[ar, best]
        other = pos[None, :] != pos[best][:, None]
        tied[c:c + CHUNK] = ((d == bd[:, None]) & other).any(1) & (bd <= r2)
        d[~other] = np.inf
        sec = d.argmin(1)
        ok = (bd <= r2) & (d[ar, sec] <= r2)
        match[c:c + CHUNK] = np.where(bd <= r2, best, -1)
        d2[c:c + CHUNK] = bd.astype(np.int64)
        second[c:c + CHUNK] = np.where(ok, sec, -1)
    mom = [int(v) for v in moments_of(t[match[match >= 0]]).sum(0, dtype=np.int64)] if (match >= 0).any() else [0] * 10
    return dict(G=matrix_from_moments(np.array(mom, dtype=object), s, exact), moments=mom, match=match, d2=d2, second=second,
                tied=tied, q=q, t=t, r2=r2, s=s)


def swapped_matrices(ref):
    """every query whose `second` exists, given that second target instead of its match -> (K, 6, 6) float32, (K,) query ids"""
    who = np.flatnonzero(ref["second"] >= 0)
    t = ref["t"]
    m = np.array(ref["moments"], dtype=np.int64)[None, :] - moments_of(t[ref["match"][who]]) + moments_of(t[ref["second"][who]])
    return matrix_from_moments(m, ref["s"]), who
