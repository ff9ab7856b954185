"""The inputs of tests/test_gpu_tsdf_roll.py, shared with tests/test_tsdf_roll_host.py, which shows on the CPU that they tell
the three mutants of tests/tsdf_roll_restated.py from the true form.

A case is a SimpleNamespace: voxel, b (tile_bits), origin (3,), pose (4,4) float64, radius, cap_vox and records = (keys int64,
sums int64, counts uint32) with unique keys in no order: the map before the evict.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_roll_restated as R  # noqa: E402

BIAS = R.BIAS
# (cap_vox, occupied slots, evicted): the wave (64) and block (256) edges of one lane per slot, tables filled to every slot (the
# rebuild's probing wraps), nothing / one / a wave / a wave and one / everything evicted
SHAPES = [(2, 0, 0), (2, 1, 0), (2, 1, 1), (2, 2, 2), (64, 63, 1), (64, 64, 0), (64, 64, 64), (256, 65, 64), (256, 255, 65),
          (256, 256, 256), (512, 256, 1), (512, 257, 65), (512, 257, 257), (512, 512, 64)]


def at(t):
    P = np.eye(4)
    P[:3, 3] = t
    return P


def values(n, rng):
    """sums within 2^40 of zero, either sign; counts over the whole uint32 range, never 0 (a held voxel has a sample)"""
    sums = rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64)
    counts = rng.integers(1, 1 << 32, n, dtype=np.int64).astype(np.uint32)
    if n > 2:
        counts[0], counts[1] = np.uint32(0xFFFFFFFF), np.uint32(1)
    return sums, counts


def voxels_of_tile(tile, b):
    """the 2^(3b) biased voxel coordinates (n,3) of the tile with unbiased tile coordinates `tile`"""
    side = 1 << b
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return g + (np.asarray(tile, np.int64) * side + BIAS)


def _case(coords, seed, **kw):
    rng = np.random.default_rng(seed)
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    keys = R.pack(coords[:, 0], coords[:, 1], coords[:, 2])
    assert len(np.unique(keys)) == len(keys)
    order = rng.permutation(len(keys))
    sums, counts = values(len(keys), rng)
    base = dict(voxel=0.25, b=3, origin=np.zeros(3), cap_vox=1 << 12)
    base.update(kw)
    return SimpleNamespace(records=(keys[order], sums, counts), **base)


def exact():
    """voxel 0.25, b = 3: tiles of 2 m.  The pose sits on the centre of tile (0,0,0), (1,1,1) m; the tiles at offsets (3,4,0),
    (0,-3,4), (-4,0,3) tile sides lie at (6,8,0) m and so on: squared distance 100 = (float)(10 * 10) EXACTLY in fp32 (all
    terms are small integers), NEAR by `<=`.  (5,0,0) likewise; (3,4,1) is far, (3,3,0) near.  Every tile is full, so the
    voxel-centre mutant finds voxels of one tile on both sides."""
    tiles = [(0, 0, 0), (3, 4, 0), (0, -3, 4), (-4, 0, 3), (5, 0, 0), (3, 4, 1), (3, 3, 0), (-5, -1, 0)]
    coords = np.concatenate([voxels_of_tile(t, 3) for t in tiles])
    return _case(coords, 1, pose=at([1.0, 1.0, 1.0]), radius=10.0, cap_vox=1 << 13)


def straddle(b=3, voxel=0.25):
    """tiles on both sides of the bias on every axis (voxel indices 2^20 - 2^b .. 2^20 + 2^b - 1), the pose 1.5 tile sides below
    zero on x with a radius of 1.25 sides: the tile just left of the bias on x (centre -0.5 sides) is near, and the form that
    divides the unbiased coordinate towards zero puts it at +0.5 sides, far"""
    side = (1 << b) * voxel
    tiles = [(x, y, z) for x in (-2, -1, 0, 1) for y in (-1, 0) for z in (-1, 0)]
    rng = np.random.default_rng(7 + b)
    corners = np.array([[0, 0, 0], [(1 << b) - 1] * 3])           # the first and the last voxel of every tile, and 38 between
    coords = np.concatenate([np.asarray(t) * (1 << b) + BIAS + np.concatenate([corners, rng.integers(0, 1 << b, (38, 3))])
                             for t in tiles])
    coords = np.unique(coords, axis=0)
    return _case(coords, 2 + b, b=b, voxel=voxel, pose=at([-1.5 * side, -0.5 * side, -0.5 * side]), radius=1.25 * side, cap_vox=1 << 11)


def big_tiles():
    """b = 10 (tiles of 256 m at voxel 0.25): a few voxels from each of 27 tiles round the bias, a general pose and radius"""
    rng = np.random.default_rng(11)
    tiles = [(x, y, z) for x in (-2, -1, 0) for y in (-1, 0, 1) for z in (-1, 0, 1)]
    coords = np.concatenate([np.asarray(t) * 1024 + BIAS + rng.integers(0, 1024, (30, 3)) for t in tiles])
    coords = np.unique(coords, axis=0)
    return _case(coords, 12, b=10, pose=at([-140.3, 17.9, 60.2]), radius=301.7, cap_vox=1 << 11)


def far_origin():
    """the map's origin 1 km out on every axis and the pose beside it: (float)(pose - origin) is formed in double first"""
    rng = np.random.default_rng(13)
    coords = np.unique(BIAS + rng.integers(-40, 40, (700, 3)), axis=0)
    o = np.array([1000.0, -1000.0, 1000.0])
    return _case(coords, 14, origin=o, pose=at(o + [1.3, -2.1, 0.7]), radius=6.0, cap_vox=1 << 11)


def general(b=5, voxel=0.2, seed=20):
    rng = np.random.default_rng(seed)
    coords = np.unique(BIAS + rng.integers(-3 << b, 3 << b, (900, 3)), axis=0)
    side = (1 << b) * voxel
    return _case(coords, seed + 1, b=b, voxel=voxel, pose=at(rng.uniform(-side, side, 3)), radius=1.8 * side, cap_vox=1 << 11)


def cases():
    return {"exact": exact(), "straddle_b3": straddle(3), "straddle_b10": straddle(10, 0.25), "big_tiles": big_tiles(),
            "far_origin": far_origin(), "general_b5": general()}


def shaped(cap_vox, occupied, evicted, seed=0):
    """`occupied` voxels of which exactly `evicted` lie in far tiles: near ones from the tile at the pose (b = 3: 512 voxels),
    far ones from tiles 9 and more tile sides away, radius 3 sides"""
    rng = np.random.default_rng(1000 * cap_vox + 10 * occupied + evicted + seed)
    near = voxels_of_tile((0, 0, 0), 3)[rng.permutation(512)[:occupied - evicted]]
    far = np.concatenate([voxels_of_tile(t, 3) for t in [(9, 0, 0), (-9, 2, 1), (0, 0, -11)]])
    far = far[rng.permutation(len(far))[:evicted]]
    c = _case(np.concatenate([near, far]), 99 + occupied, pose=at([1.0, 1.0, 1.0]), radius=6.0, cap_vox=cap_vox)
    c.occupied, c.evicted = occupied, evicted
    return c


# ------------------------------------------------------------------------------------------------- frames for rolled-map runs
LINE = dict(voxel=0.4, max_range=8.0, b=3, slack=1.0)      # tiles of 3.2 m; reach 8 + 1.6 + 2.77 + 0.4 = 12.77 m
LINE_X = (0.0, 24.0, 48.0, 60.0, 36.0, 12.0)               # six poses on a 60 m line, out and back: tiles leave and return


def line_frames(origin=(0.0, 0.0, 0.0)):
    """six frames of 196 rows on the line: three rows of ground (z = -1.5, a voxel apart, so that cells have their 8 corners)
    reaching 7 m before and behind the sensor, so neighbouring frames, 12 m apart, share voxels, and a 5 x 5 patch across the
    line 3 m ahead; all within max_range.  -> [(xyz (196,3) float32 sensor frame, pose (4,4))]; the poses turn a little so nothing is axis-exact"""
    s = np.arange(57) * 0.25 - 7.0 + 0.013
    ground = np.concatenate([np.stack([s, np.full_like(s, y), np.full_like(s, -1.5)], 1) for y in (-0.4, 0.01, 0.42)])
    u, w = [g.ravel() for g in np.meshgrid(np.arange(5) * 0.3 - 0.6, np.arange(5) * 0.3 - 0.61)]
    post = np.stack([np.full_like(u, 3.0), u, w], 1)
    local = np.concatenate([ground, post])
    out = []
    for k, x in enumerate(LINE_X):
        import icp_restated as I
        P = I.se3([0.01 * k, -0.02, 0.03 * k], np.asarray(origin) + [x, 0.1 * k, 0.05])
        world = local + [x, 0.0, 0.0] + np.asarray(origin)
        out.append((((world - P[:3, 3]) @ P[:3, :3]).astype(np.float32), P))
    return out


CORRIDOR = dict(voxel=0.25, max_range=4.0, b=3, slack=1.0, register_every=3, frames=150, advance=0.4)


def _boxes():
    """ribs on both walls of the corridor, every 2 m, staggered: they pin the motion along it"""
    out = []
    for x in np.arange(-8.0, 80.0, 2.0):
        out.append(((x, 1.2, -1.5), (x + 0.6, 2.0, 1.5)))
        out.append(((x + 1.0, -2.0, -1.5), (x + 1.6, -1.2, 1.5)))
    return np.array(out)


def corridor(frames=None, advance=None, columns=96, beams=48, reach=6.0):
    """a sensor moving along a corridor of 4 x 3 m (x from -10 to 80 m) with ribs of 0.6 x 0.8 m on both walls: `frames` poses
    `advance` metres apart -> (xyz per frame [(n,3) float32, sensor frame], analytic normals per frame, poses (frames,4,4)).
    The rays are tests/tsdf_register_restated.box_room's.  Only the ribs within `reach` metres along the corridor are cast
    against: a return within max_range = 4 m is not changed by a rib farther off, and the returns beyond are taken out
    (gated_corridor)."""
    import icp_restated as I
    frames = CORRIDOR["frames"] if frames is None else frames
    advance = CORRIDOR["advance"] if advance is None else advance
    az = (np.arange(columns) + 0.37) * (2 * np.pi / columns)
    el = np.radians(np.linspace(-38.0, 38.0, beams) + 0.21)
    e, a = [g.ravel() for g in np.meshgrid(el, az, indexing="ij")]
    rays = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], axis=1)
    lo, hi = np.array([-10.0, -2.0, -1.5]), np.array([80.0, 2.0, 1.5])
    boxes = _boxes()
    out_xyz, out_n, poses = [], [], []
    for k in range(frames):
        P = I.se3([0.001 * np.sin(k), -0.001, 0.02 * np.sin(0.1 * k)], [advance * k, 0.17 * np.sin(0.05 * k), 0.09])
        d, o = rays @ P[:3, :3].T, P[:3, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(d > 0, (hi - o) / d, np.where(d < 0, (lo - o) / d, np.inf))        # the corridor, from inside
            axis = np.argmin(t, axis=1)
            best = t[np.arange(len(t)), axis]
            close = boxes[(boxes[:, 0, 0] <= o[0] + reach) & (boxes[:, 1, 0] >= o[0] - reach)]      # the ribs, from outside
            t1, t2 = (close[:, None, 0] - o) / d, (close[:, None, 1] - o) / d                       # (ribs, rays, 3)
            near, far = np.minimum(t1, t2), np.maximum(t1, t2)
            tin, tout = near.max(2), far.min(2)
            tin = np.where((tin <= tout) & (tin > 0), tin, np.inf)
            rib = tin.argmin(0)
            first = tin[rib, np.arange(len(d))]
            hit = first < best
            axis = np.where(hit, near[rib, np.arange(len(d))].argmax(1), axis)
            best = np.where(hit, first, best)
        nw = np.zeros_like(d)
        nw[np.arange(len(d)), axis] = -np.sign(d[np.arange(len(d)), axis])
        out_xyz.append((rays * best[:, None]).astype(np.float32))
        out_n.append((nw @ P[:3, :3]).astype(np.float32))
        poses.append(P)
    return out_xyz, out_n, np.stack(poses)


def touched(xyz, pose, voxel, truncation, step, max_range):
    """the voxel coordinates (unbiased, unique rows) an integrate of the frame at `pose` touches, in float64: for COUNTING voxels
    when a test's sizes are chosen, not for bytes"""
    p = np.asarray(xyz, np.float64)
    r = np.linalg.norm(p, axis=1)
    ok = (r > 0) & (r <= max_range)
    p, r = p[ok], r[ok]
    u = (p / r[:, None]) @ pose[:3, :3].T
    n = int(np.ceil(truncation / step))
    t = r[:, None] + np.arange(-n, n + 1)[None, :] * step
    pts = pose[:3, 3] + u[:, None, :] * t[:, :, None]
    return np.unique(np.floor(pts[t > 0] / voxel).astype(np.int64), axis=0)


def gated_corridor():
    """`corridor` with the returns beyond max_range taken out of every frame: a registration reads the field at EVERY row it is
    given, and a row far beyond max_range would read where an unrolled map still holds what a rolled one has sent to the host"""
    xyz, nrm, poses = corridor()
    keep = [np.linalg.norm(x.astype(np.float64), axis=1) <= CORRIDOR["max_range"] - 1e-3 for x in xyz]
    return [x[k] for x, k in zip(xyz, keep)], [n[k] for n, k in zip(nrm, keep)], poses
