"""Seeded inputs of the exact information-matrix tests (tests/test_infomat_host.py, tests/test_gpu_infomat_exact.py): clouds on a
dyadic lattice, built from seeds -- no arrays are stored.  Every case is a dict
  name, s (lattice step 2^-s), radius (a power of two), pcd1 (3, N1) / pcd2 (3, N2) float32, Rt (12,) float32, branch (what
  part of csrc/infomat.hip the case exists for)
sized by the rule  N1 * max|target coordinate| * 4 < 2^23 * 2^-s : the first moments then stay below 2^21 lattice steps, fp32
holds them exactly, and one lattice step of change in any of them survives the final rounding (tests/infomat_restated.py).
`grid_shape` restates the grid header of grid_setup_kernel in fp32 so that a case can assert which branch it reaches."""
import functools

import numpy as np

IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=np.float32)
GMAX, GB_CHUNK = 512, 4096  # csrc/infomat.hip


def _cloud(units, s):
    """(N, 3) integer lattice units -> (3, N) float32 metres, read-only"""
    a = np.ascontiguousarray((np.asarray(units, dtype=np.float64) / (1 << s)).T.astype(np.float32))
    a.setflags(write=False)
    return a


def _case(name, s, radius, q, t, branch, Rt=IDENTITY, **extra):
    c = dict(name=name, s=s, radius=float(radius), pcd1=_cloud(q, s), pcd2=_cloud(t, s), Rt=np.array(Rt, dtype=np.float32),
             branch=branch, **extra)
    n1, amax = c["pcd1"].shape[1], float(np.abs(c["pcd2"]).max())
    assert n1 * amax * 4 < 2 ** 23 * 2.0 ** -s, (name, "sizing rule", n1, amax)
    return c


def grid_shape(pcd2, radius):
    """the header grid_setup_kernel computes for a target cloud (fp32 arithmetic, fine grid on) and the grid row / column of
    every target -> dict(H, cs, inv_cs, gx, gy, lox, loy, row, col, chunks)"""
    f = np.float32
    x, y = pcd2[0].astype(f), pcd2[1].astype(f)
    lox, hix, loy, hiy = x.min(), x.max(), y.min(), y.max()
    ext = max(max(hix - lox, hiy - loy), f(1e-6))
    cs, H = max(f(radius) * f(0.5005), ext / f(GMAX - 1)), 2
    if cs >= f(radius):
        cs, H = max(f(radius), ext / f(GMAX - 1)), 1
    inv = f(1.0) / cs
    gx, gy = min(GMAX, int((hix - lox) / cs) + 1), min(GMAX, int((hiy - loy) / cs) + 1)
    col = np.clip(np.floor((x - lox) * inv), 0, gx - 1).astype(np.int64)
    row = np.clip(np.floor((y - loy) * inv), 0, gy - 1).astype(np.int64)
    return dict(H=H, cs=float(cs), inv_cs=inv, gx=gx, gy=gy, lox=lox, loy=loy, row=row, col=col,
                chunks=-(-pcd2.shape[1] // GB_CHUNK))


def query_cells(g, q_metres):
    """(N1, 3) transformed queries in metres -> their (unclamped) grid row and column under header g"""
    f = np.float32
    q = np.asarray(q_metres, dtype=f)
    return (np.floor((q[:, 1] - g["loy"]) * g["inv_cs"]).astype(np.int64),
            np.floor((q[:, 0] - g["lox"]) * g["inv_cs"]).astype(np.int64))


# ---------------------------------------------------------------------------------------------- single-pair cases, s = 5
L = 32  # lattice steps per metre at s = 5


def fine_partial_chunks():
    """N1 = 3000 (no multiple of 256), N2 = 4097 (a full chunk plus one point), r = 1 in a 24 x 24 x 2 m box: half-radius cells,
    H = 2.  300 queries lie outside the target's bounding box: 200 by 1/32 .. 1/2 m next to a target (they match through
    cells below 0 and beyond gx / gy), 100 by up to 6 m (they do not)."""
    rng = np.random.default_rng(5101)
    hx, hz = 12 * L, L
    t = np.stack([rng.integers(-hx, hx + 1, 4097), rng.integers(-hx, hx + 1, 4097), rng.integers(-hz, hz + 1, 4097)], 1)
    lo, hi = t.min(0), t.max(0)
    q = t[rng.integers(0, len(t), 2700)] + rng.integers(-19, 20, (2700, 3))      # moved by up to 0.6 m per axis
    near = []
    for axis in (0, 1):
        for side in (0, 1):
            edge = lo[axis] if side == 0 else hi[axis]
            cand = np.flatnonzero(np.abs(t[:, axis] - edge) <= 12)
            p = t[rng.choice(cand, 50)] + rng.integers(-8, 9, (50, 3))
            k = rng.integers(1, 17, 50)
            p[:, axis] = edge - k if side == 0 else edge + k                       # 1/32 .. 1/2 m outside, <= 28 steps from its target
            near.append(p)
    far = np.stack([rng.integers(-hx, hx + 1, 100), rng.integers(-hx, hx + 1, 100), rng.integers(-hz, hz + 1, 100)], 1)
    k = rng.integers(33, 193, 100)
    axis, side = rng.integers(0, 2, 100), rng.integers(0, 2, 100)
    far[np.arange(100), axis] = np.where(side == 0, lo[axis] - k, hi[axis] + k)
    far[:25, 1] = hi[1] + rng.integers(40, 120, 25)                               # some beyond a corner: both cells out of range
    far[:25, 0] = lo[0] - rng.integers(40, 120, 25)
    q = np.concatenate([q] + near + [far])
    q = q[rng.permutation(len(q))]
    return _case("fine_partial_chunks", 5, 1.0, q, t, "H = 2, partly filled chunk, N1 % 256 != 0, cells outside the grid")


def second_ring():
    """A sparse, nearly planar cloud (mean spacing about 1.6 m) and r = 1: the nearest target is routinely 0.5 .. 1 m away in x
    or y -- two cells, where the rows are pruned by the lower bound -- and a good share of the queries has none."""
    rng = np.random.default_rng(5102)
    h = 18 * L
    n2 = int((36 / 1.6) ** 2)
    t = np.stack([rng.integers(-h, h + 1, n2), rng.integers(-h, h + 1, n2), rng.integers(-3, 4, n2)], 1)
    q = np.stack([rng.integers(-h - 16, h + 17, 2500), rng.integers(-h - 16, h + 17, 2500), rng.integers(-3, 4, 2500)], 1)
    return _case("second_ring", 5, 1.0, q, t, "H = 2, winners two cells away: the row prune in both directions")


def _sites():
    """243 isolated sites, 4 m apart (three layers in z) and moved by up to 1/4 m: targets stay within 1 m and queries within
    1.1 m of their site, so no query sees another site's targets"""
    rng = np.random.default_rng(5103)
    g = np.arange(-4, 5) * 4 * L
    c = np.stack(np.meshgrid(g, g, np.array([-4, 0, 4]) * L, indexing="ij"), -1).reshape(-1, 3)
    return rng, c + rng.integers(-8, 9, c.shape)


def on_radius_and_ties():
    """Shuffled targets.  A third of the sites: one target, queries at exactly d^2 = r^2 (every lattice vector of squared length
    1024 steps).  A third: one target, queries one lattice step beyond (d^2 = 1025 steps^2 and d = 33 steps).  A third: two or
    four targets at equal distance from the query, within and on the radius -- the smallest index must win."""
    rng, c = _sites()
    kind = rng.permutation(len(c)) % 3
    R = L  # radius in steps
    span = np.arange(-R - 1, R + 2)
    v = np.stack(np.meshgrid(span, span, span, indexing="ij"), -1).reshape(-1, 3)
    n = (v * v).sum(1)
    on, beyond = v[n == R * R], v[(n == R * R + 1) | ((n == (R + 1) ** 2) & ((v != 0).sum(1) == 1))]
    t, q = [], []
    for site, k in zip(c, kind):
        if k == 0:
            t.append(site[None])
            q.append(site + on[rng.choice(len(on), 3, replace=False)])
        elif k == 1:
            t.append(site[None])
            q.append(site + beyond[rng.choice(len(beyond), 3, replace=False)])
        else:
            # targets at +-a on one axis (and on a second one: four), queries on the remaining axis at +-b with
            # a^2 + b^2 <= r^2 (a = R, b = 0: a tie on the radius itself); with two targets the query may leave the axis
            a, i = int(rng.integers(1, R + 1)), int(rng.integers(0, 3))
            e = np.eye(3, dtype=np.int64)
            u, w, third = a * e[i], a * e[(i + 1) % 3], e[(i + 2) % 3]
            four = rng.random() < 0.5
            t.append(site + (np.stack([u, -u, w, -w]) if four else np.stack([u, -u])))
            b = int(rng.integers(0, int(np.sqrt(R * R - a * a)) + 1))
            m = 0 if four else int(rng.integers(0, int(np.sqrt(R * R - a * a - b * b)) + 1))
            q.append(site + np.stack([third * b, -third * b]) + m * e[(i + 1) % 3])
    t, q = np.concatenate(t), np.concatenate(q)
    return _case("on_radius_and_ties", 5, 1.0, q, t[rng.permutation(len(t))], "d^2 == r^2 kept, one step beyond dropped, ties")


def _clustered(seed, reach):
    """corner points that fix a 40 m extent on both axes, 2000 clusters of four targets within `reach` steps, and 3000 queries
    within `reach` steps of a target"""
    rng = np.random.default_rng(seed)
    h = 20 * L
    centre = np.stack([rng.integers(-h + reach, h - reach + 1, 2000), rng.integers(-h + reach, h - reach + 1, 2000),
                       rng.integers(-L, L + 1, 2000)], 1)
    t = (centre[:, None, :] + rng.integers(-reach, reach + 1, (2000, 4, 3))).reshape(-1, 3)
    t = np.concatenate([np.array([[-h, -h, 0], [h, h, 0]]), t])
    q = t[rng.integers(0, len(t), 3000)] + rng.integers(-reach, reach + 1, (3000, 3))
    return q, t[rng.permutation(len(t))]


def coarse_grid():
    """r = 2^-4 over 40 m: extent / r = 640 >= 511, the cell edge is extent / 511 >= r -- 3 x 3 blocks, H = 1"""
    q, t = _clustered(5104, 2)
    return _case("coarse_grid", 5, 2.0 ** -4, q, t, "H = 1 (cell edge >= radius, 3 x 3 cells)")


def full_grid_fine():
    """r = 2^-3 over 40 m on both axes: 256 < extent / r = 320 < 511, H = 2 with about 512 rows and columns -- every thread of
    grid_offsets_kernel owns rows and its cross-wave prefix runs over all four waves"""
    q, t = _clustered(5105, 4)
    return _case("full_grid_fine", 5, 2.0 ** -3, q, t, "H = 2 with gx, gy > 256: all of grid_offsets_kernel")


BAND_Y0, BAND_N = 3 * L + 5, 4000   # the band of long_rows: y in [BAND_Y0, BAND_Y0 + 8) steps (1/4 m), x over 4 m


def long_rows():
    """N2 = 9001 (three chunks, the last partly filled), 4000 of them in a band 1/4 m wide in y and 4 m long in x: more than 512
    points in one grid row (the overflow loop of grid_cells_kernel) and hundreds of candidates per row range"""
    rng = np.random.default_rng(5106)
    h = 18 * L
    cell = rng.choice(128 * 8 * 64, BAND_N, replace=False)
    band = np.stack([cell % 128 - 64, cell // 128 % 8 + BAND_Y0, cell // 1024 - 32], 1)
    n = 9001 - BAND_N
    rest = np.stack([rng.integers(-h, h + 1, n), rng.integers(-h, h + 1, n), rng.integers(-L, L + 1, n)], 1)
    t = np.concatenate([band, rest])
    t = t[rng.permutation(len(t))]
    qb = np.stack([rng.integers(-80, 81, 1500), rng.integers(BAND_Y0 - 40, BAND_Y0 + 48, 1500), rng.integers(-40, 41, 1500)], 1)
    qr = rest[rng.integers(0, n, 1500)] + rng.integers(-19, 20, (1500, 3))
    q = np.concatenate([qb, qr])
    return _case("long_rows", 5, 1.0, q[rng.permutation(len(q))], t, "grid rows of more than 512 points, long row ranges")


def far_from_origin():
    """step 1/4 m, cloud moved by (1000, -2000, 50) m: qexp drops to 10 and the cell arithmetic runs on large coordinates.
    N1 = 257 is what the sizing rule leaves at |y| <= 2015 m (two blocks of queries)."""
    rng = np.random.default_rng(5107)
    s, shift = 2, np.array([1000, -2000, 50]) * 4
    t = np.stack([rng.integers(-60, 61, 1500), rng.integers(-60, 61, 1500), rng.integers(-8, 9, 1500)], 1)
    q = t[rng.integers(0, len(t), 257)] + rng.integers(-4, 5, (257, 3))
    return _case("far_from_origin", s, 1.0, q + shift, t + shift, "qexp = 10, large coordinates")


def _posed(base, name, R, T_steps):
    """`base` with its queries moved by the inverse of the pose (R, T): the kernel's R q + T lands on the base case's queries"""
    s = base["s"]
    q = np.rint(base["pcd1"].T.astype(np.float64) * (1 << s)).astype(np.int64)
    R = np.array(R, dtype=np.int64)
    p1 = (q - np.array(T_steps)) @ R                     # R^T (q - T), row vectors
    Rt = np.concatenate([R.reshape(-1), np.array(T_steps) / (1 << s)]).astype(np.float32)
    c = dict(base, name=name, pcd1=_cloud(p1, s), Rt=Rt, branch=base["branch"] + "; pose = signed permutation + lattice shift")
    return c


def permuted_rot_z():
    return _posed(case("fine_partial_chunks"), "permuted_rot_z", [[0, -1, 0], [1, 0, 0], [0, 0, 1]], [112, -232, 24])


def permuted_cyclic():
    return _posed(case("fine_partial_chunks"), "permuted_cyclic", [[0, 0, 1], [1, 0, 0], [0, 1, 0]], [-75, 41, 130])


# ---------------------------------------------------------------------------------------------- degenerate cases
def one_target():
    rng = np.random.default_rng(5108)
    t = np.array([[37, -101, 12]])
    return _case("one_target", 5, 1.0, t + rng.integers(-40, 41, (300, 3)), t, "N2 = 1: a 1 x 1 grid")


def one_query():
    rng = np.random.default_rng(5109)
    t = np.stack([rng.integers(-200, 201, 500), rng.integers(-200, 201, 500), rng.integers(-20, 21, 500)], 1)
    return _case("one_query", 5, 1.0, t[123:124] + np.array([[3, -2, 1]]), t, "N1 = 1: one quad with three idle turns")


def coincident_targets():
    rng = np.random.default_rng(5110)
    t = np.repeat(np.array([[-77, 300, 5]]), 50, 0)
    return _case("coincident_targets", 5, 1.0, t[0] + rng.integers(-40, 41, (300, 3)), t, "all targets at one point: zero extent")


def vertical_line():
    """2000 targets on a vertical line 62.5 m tall: one cell holds them all (a row of more than 512 points at gx = gy = 1)"""
    rng = np.random.default_rng(5111)
    t = np.stack([np.full(2000, 40), np.full(2000, -25), np.arange(2000)], 1)
    q = t[rng.integers(0, 2000, 700)] + rng.integers(-30, 31, (700, 3))
    return _case("vertical_line", 5, 1.0, q, t[rng.permutation(2000)], "one cell with 2000 points")


def stacks():
    """121 isolated vertical stacks of 1 .. 24 targets one lattice step apart (one grid cell each, so a query's row range IS the
    stack) and one query per target at the target's height, up to 1 m away in the plane: EVERY candidate of a range is some
    query's winner, wherever the scheduling-dependent order inside the cell puts it -- first eight, loop, clamped second slot,
    last position -- in the query's own row, the rows next to it and the pruned rows two cells away."""
    rng = np.random.default_rng(5113)
    g = np.arange(-5, 6) * 3 * L
    c = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2) + rng.integers(-8, 9, (121, 2))
    span = np.arange(-L, L + 1)
    v = np.stack(np.meshgrid(span, span, indexing="ij"), -1).reshape(-1, 2)
    v = v[(v * v).sum(1) <= L * L]
    t, q = [], []
    for k, site in enumerate(c):
        n = k % 24 + 1
        z = int(rng.integers(-16, 17)) + np.arange(n)
        t.append(np.concatenate([np.tile(site, (n, 1)), z[:, None]], 1))
        q.append(np.concatenate([site + v[rng.integers(0, len(v), n)], z[:, None]], 1))
    t, q = np.concatenate(t), np.concatenate(q)
    return _case("stacks", 5, 1.0, q[rng.permutation(len(q))], t[rng.permutation(len(t))],
                 "every candidate of a row range wins once: no position of a range may be dropped")


def no_match():
    rng = np.random.default_rng(5112)
    t = np.stack([rng.integers(-300, 301, 600), rng.integers(-300, 301, 600), rng.integers(-20, 21, 600)], 1)
    q = np.stack([rng.integers(-340, 341, 400), rng.integers(-340, 341, 400), 20 + rng.integers(33, 80, 400)], 1)
    q[:200, :2] = t[:200, :2]                                          # straight above a target: 33 steps and more over the highest
    return _case("no_match", 5, 1.0, q, t, "nothing within the radius: the zero matrix")


SINGLE = {f.__name__: f for f in (fine_partial_chunks, second_ring, on_radius_and_ties, coarse_grid, full_grid_fine, long_rows,
                                  far_from_origin, permuted_rot_z, permuted_cyclic, one_target, one_query, coincident_targets,
                                  vertical_line, stacks, no_match)}


@functools.lru_cache(maxsize=None)
def case(name):
    return SINGLE[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """tests/infomat_restated.py on a single-pair case: computed once per process, shared by every test that needs it"""
    import infomat_restated as IR
    c = case(name)
    return IR.restate(c["pcd1"], c["pcd2"], c["Rt"], c["radius"], c["s"])


# ---------------------------------------------------------------------------------------------- batched cases
F_FRAMES, N_BATCH = 5, 3001
PAIR_LISTS = {   # (source frame, target frame); frame 4 is nobody's target, every list has a self pair
    3: [(0, 1), (1, 1), (4, 0)],
    8: [(0, 1), (1, 2), (2, 0), (4, 2), (3, 3), (4, 1), (0, 2), (3, 0)],
    16: [(0, 1), (1, 2), (2, 3), (3, 0), (4, 0), (4, 1), (4, 2), (4, 3), (2, 2), (0, 3), (1, 0), (3, 1), (0, 0), (2, 1),
         (3, 2), (1, 3)],
}


@functools.lru_cache(maxsize=None)
def frames():
    """(5, 3, 3001) float32: five views of one world of 5000 lattice points in a 34 x 34 x 2 m box -- 3001 of them each, half of
    those moved by up to 10 steps per axis"""
    rng = np.random.default_rng(5120)
    h = 17 * L
    world = np.stack([rng.integers(-h, h + 1, 5000), rng.integers(-h, h + 1, 5000), rng.integers(-L, L + 1, 5000)], 1)
    out = []
    for _ in range(F_FRAMES):
        p = world[rng.choice(5000, N_BATCH, replace=False)]
        p = p + rng.integers(-10, 11, p.shape) * (rng.random((N_BATCH, 1)) < 0.5)
        out.append(_cloud(p, 5))
    a = np.stack(out)
    assert N_BATCH * float(np.abs(a).max()) * 4 < 2 ** 23 * 2.0 ** -5
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def pair_poses(n_pairs):
    """(P, 12) float32: the identity for a self pair, otherwise a lattice shift of up to half a metre, every fifth pair turned by
    90 degrees about z as well"""
    rng = np.random.default_rng(5130 + n_pairs)
    Rt = np.tile(IDENTITY, (n_pairs, 1))
    for p, (a, b) in enumerate(PAIR_LISTS[n_pairs]):
        if a == b:
            continue
        Rt[p, 9:12] = rng.integers(-16, 17, 3) / L
        if p % 5 == 3:
            Rt[p, :9] = [0, -1, 0, 1, 0, 0, 0, 0, 1]
    Rt.setflags(write=False)
    return Rt


@functools.lru_cache(maxsize=None)
def pair_reference(n_pairs, p):
    import infomat_restated as IR
    a, b = PAIR_LISTS[n_pairs][p]
    return IR.restate(frames()[a], frames()[b], pair_poses(n_pairs)[p], 1.0, 5)
