"""A fused surface on the GPU: a truncated signed distance field (TSDF) over hashed voxels (csrc/tsdf_map.hip), its zero
crossings as surface points with normals, and a triangle mesh from marching tetrahedra.  The reference has no counterpart:
its map is a cloud of points.  DESIGN §7l is the definition.

`TsdfMap.integrate` fuses one frame under its pose: every return is a ray from the pose's translation, sampled every `step`
metres within `truncation` of the return; each sample adds the signed distance to the return along the ray, as seen from
the centre of the voxel it falls into, to that voxel's integer sum.  Integer atomics only, so the map is a function of the
frames alone: the sorted export has the same bytes whatever the order of rows, frames or launches.
`integrate_frames` does the same for a list of stored frames in one launch (LoopCloser.store), which is how
`GeometricSlam.surface_map` fuses a run under its corrected poses.

`TsdfMap(distance="plane")` fuses the distance of the voxel's centre to the TANGENT PLANE at the return instead (the distance
along the ray is wrong by about d tan(incidence) for a centre d beside a slanted ray), each sample weighted by the cosine of
the incidence in 1/256ths; it needs a normal per return, in the sensor frame.  A map keeps one form from its construction:
`unit` is the count of one full-weight sample, 1 or 256, and every `min_count` and carve weight is given in full-weight samples.
`carve` / `carve_frames` tell every voxel THE MAP ALREADY HOLDS that a ray crosses well before its return "free, at the
truncation distance": lookups only, so the key set stays, and what was seen through is forgotten once the free observations
outweigh it.  Carving is meant to run after the integrations; a later integrate simply adds to what is there.

`TsdfMap.sample` reads the field at points -- the trilinear interpolant between the 8 voxel centres round each and its exact
gradient inside that cell, defined only where all 8 voxels are qualified -- and `TsdfMap.register` is Gauss-Newton of a scan
against it: the residual of a point is the field's value there, its Jacobian the gradient, so nothing is searched.  Both are
lookups only.  `TsdfTracker` is frame-to-model odometry on one map: predict, register, read back once, fuse under the registered
pose; a failed registration writes nothing.  The plane form is the one to register against: in a band fed by one plane its
field is exactly linear, while the ray form's is not a distance off the ray's axis.

`TsdfMap.raycast` looks at the map the way the sensor does: per pose and ray the range at which the field changes sign between
two samples that both have a value, the unit normal there in the SENSOR frame and a flag (MISS, HIT from free space, BACK out of
the back of a surface); one launch for any number of poses, lookups only.  An occupied-block set (the 8 x 8 x 8 blocks that hold
a qualified voxel), built on first use and dropped by every write, lets empty space cost one probe per block entered; the bytes
are those of `skip=False`.  `TsdfMap.render` compacts the HIT rays of one pose into a frame with ray indices and normals that
`integrate(..., normals=)`, `register`, ScanContext and `transform_frames` take as they are; `TsdfTracker.predicted` renders at
the predicted pose.  The step is fixed (no sphere tracing: the field is clamped at the truncation), a crossing needs two valued
samples in a row, so sparse maps miss, and BACK ends the ray.

LIMITS: carving reaches only voxels that exist and claims none; no weight cap or decay; the frame's pose is the origin of every
ray (no per-point origins for sweeps that are not deskewed); the normals of the plane form are the caller's (or dpm_point_normals
of the frame alone, `normals=<radius>`); marching tetrahedra, not marching cubes; the voxels live on the device unless
the map is rolled: `TsdfMap.roll` evicts the tiles far from the sensor to a `TsdfArchive` on the host and absorbs them when the
sensor comes back (integer addition: `merged_export` is the unrolled map's export, byte for byte; a rolling map costs twice the
table).

`TsdfMap.mesh_indexed` is `mesh` welded on the device (vertices, faces, per-vertex normals and vertex names in `weld`'s order,
one synchronisation), and with `tiles=` it meshes only the cells those tiles own.  `merged_mesh` / `merged_surface` mesh a map
larger than the table -- the map's voxels and an archive's, in batches of tiles through one scratch table, merged by vertex name
on the host -- with the bytes of the map that never rolled: no seams.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import augment, ops
from .odometry import _HashedMap, _pose_tensor
from .refine import CONVERGED, MAX_ITER, NO_MATCH, IcpResult

OVERFLOW = "the TSDF map is full (max_voxels={}): samples found no free slot and the map is undefined; raise max_voxels"
FIX_ONE = 16777216.0    # 2^24: a sum is in units of 2^-24 m


class TsdfSurface(NamedTuple):
    """zero crossings along the axes, sorted by (key, axis), on the device.  xyz is in WORLD coordinates, (float)((double)xyz_map
    + origin), so that evaluate.map_accuracy(s.xyz, scene, origin=s.origin) takes it as it is; xyz_map is what the kernel wrote,
    relative to `origin`."""
    xyz: torch.Tensor        # (3,M) float32, world
    normals: torch.Tensor    # (3,M) float32, towards free space; (0,0,0) where the field has no gradient
    keys: torch.Tensor       # (M,) int64: the voxel k0 of the crossing between k0 and k0 + e_axis
    axes: torch.Tensor       # (M,) int32
    origin: np.ndarray       # (3,) float64
    xyz_map: torch.Tensor    # (3,M) float32, map frame


class TsdfMesh(NamedTuple):
    """an indexed triangle mesh in `weld`'s order: vertices sorted by name (key, direction), every face rotated so that its
    smallest index leads, faces sorted by row.  Map frame: world = vertices + origin."""
    vertices: torch.Tensor      # (V,3) float32
    faces: torch.Tensor         # (F,3) int32; (b - a) x (c - a) points to free space
    normals: torch.Tensor       # (V,3) float32: the field's unit gradient on the vertex's edge; (0,0,0) where it has none
    vertex_keys: torch.Tensor   # (V,) int64: the voxel p of the edge p - q the vertex lies on
    vertex_dirs: torch.Tensor   # (V,) int32: 0..6, which q


def field_values(sums, counts) -> np.ndarray:
    """D = (float)((double)sum / ((double)count * 2^24)) of exported slots, as the kernels form it"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return (np.asarray(sums, np.int64).astype(np.float64)
                / (np.asarray(counts).astype(np.uint32).astype(np.float64) * FIX_ONE)).astype(np.float32)


def _first_index(k, d):
    """a vertex name (key, direction) a row -> (each row's index among the distinct names, sorted; the first row of each of them)"""
    order = np.lexsort((d, k))
    first = np.concatenate([[True], (np.diff(k[order]) != 0) | (np.diff(d[order]) != 0)])
    index = np.empty(k.size, np.int64)
    index[order] = np.cumsum(first) - 1
    return index, order[first]


def _canonical_faces(faces):
    """(F,3) indices -> int32, each face rotated so that its smallest index leads, the faces sorted by row"""
    lead = faces.argmin(axis=1)
    faces = np.stack([faces[np.arange(len(faces)), (lead + j) % 3] for j in range(3)], axis=1)
    return np.ascontiguousarray(faces[np.lexsort((faces[:, 2], faces[:, 1], faces[:, 0]))].astype(np.int32))


def _by_name(keys, minor):
    """device: the order that sorts rows by (key, then direction or axis)"""
    order = torch.sort(minor, stable=True).indices
    return order[torch.sort(keys[order], stable=True).indices]


def _surface_of(keys, axes, xyz_map, normals, origin) -> TsdfSurface:
    """surface rows in any order (xyz_map and normals (n,3), map frame) -> TsdfSurface sorted by (key, axis), world = map + origin"""
    order = _by_name(keys, axes)
    local = xyz_map[order].t().contiguous()
    world = (local.double() + torch.from_numpy(origin).to(local.device)[:, None]).float()
    return TsdfSurface(world, normals[order].t().contiguous(), keys[order], axes[order], origin, local)


def weld(vertex_keys, vertex_dirs, xyz):
    """triangles as (n,3) vertex names (key, direction) + (n,3,3) positions -> (vertices (V,3) float32 sorted by name, faces
    (F,3) int32, each rotated so that its smallest vertex comes first, sorted by row).  A name has one position."""
    k, d = np.asarray(vertex_keys, np.int64).reshape(-1), np.asarray(vertex_dirs, np.int32).reshape(-1)
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    if k.size == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    index, keep = _first_index(k, d)
    return np.ascontiguousarray(p[keep]), _canonical_faces(index.reshape(-1, 3))


def write_ply(path, vertices, faces=None, normals=None) -> None:
    """a binary little-endian PLY: vertices (V,3) float32 [with normals (V,3)], faces (F,3) int32 as uchar-counted lists"""
    v = np.ascontiguousarray(np.asarray(vertices, "<f4").reshape(-1, 3))
    cols, props = [v], ["x", "y", "z"]
    if normals is not None:
        n = np.asarray(normals, "<f4").reshape(-1, 3)
        if n.shape != v.shape:
            raise ValueError("write_ply: one normal per vertex")
        cols.append(n)
        props += ["nx", "ny", "nz"]
    f = np.zeros((0, 3), "<i4") if faces is None else np.asarray(faces, "<i4").reshape(-1, 3)
    if f.size and not (0 <= f.min() and f.max() < len(v)):
        raise ValueError("write_ply: faces index the vertices")
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"] + [f"property float {p}" for p in props]
    if faces is not None:
        head += [f"element face {len(f)}", "property list uchar int vertex_indices"]
    head.append("end_header")
    with open(path, "wb") as out:
        out.write(("\n".join(head) + "\n").encode("ascii"))
        out.write(np.ascontiguousarray(np.concatenate(cols, axis=1)).tobytes())
        if faces is not None:
            rec = np.zeros(len(f), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
            rec["n"], rec["v"] = 3, f
            out.write(rec.tobytes())


class TsdfCast(NamedTuple):
    """what `TsdfMap.raycast` saw, on the device: per pose and ray the range along the ray (metres), the unit normal in the
    SENSOR frame (towards the field's positive side) and a flag -- MISS 0: no crossing, range and normal zeros; HIT 1: from free
    space into a surface; BACK 2: out of the back of one"""
    range: torch.Tensor      # (F,R) float32
    normals: torch.Tensor    # (F,R,3) float32
    flag: torch.Tensor       # (F,R) int32


# -- rolling the map: tiles, and the host archive of the voxels that left the device -------------------------------------------
KEY_BIAS, _AXIS = 1 << 20, (1 << 21) - 1
NO_RECORDS = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.uint32))


def tile_of(keys, tile_bits: int) -> np.ndarray:
    """voxel keys -> the keys of their tiles, pack_key(x >> b, y >> b, z >> b): the cube of 2^b voxels per axis"""
    k, b = np.asarray(keys, np.int64), int(tile_bits)
    return ((k & _AXIS) >> b) | ((((k >> 21) & _AXIS) >> b) << 21) | ((((k >> 42) & _AXIS) >> b) << 42)


def tile_near(tile_keys, tile_bits: int, centre_map_xyz, radius: float, voxel_size: float) -> np.ndarray:
    """dpm_tsdf_evict's test restated in numpy float32, every operation rounded once: per axis c = ((float)((t << b) - 2^20) +
    0.5f * (float)2^b) * v, d = c - (float)centre, NEAR when (dx*dx + dy*dy) + dz*dz <= (float)(radius * radius).
    centre_map_xyz: the pose's translation minus the map's origin, float64."""
    t, b = np.asarray(tile_keys, np.int64), int(tile_bits)
    v, half = np.float32(voxel_size), np.float32(0.5) * np.float32(1 << b)
    at = np.asarray(centre_map_xyz, np.float64).reshape(3).astype(np.float32)
    d = [((((t >> (21 * a)) & _AXIS) << b) - KEY_BIAS).astype(np.float32) for a in range(3)]
    d = [(d[a] + half) * v - at[a] for a in range(3)]
    with np.errstate(invalid="ignore", over="ignore"):
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= np.float32(float(radius) * float(radius))


def merge_records(keys, sums, counts):
    """records in any order -> sorted by key with equal keys added (int64 and uint32 addition, wrapping as the device's)"""
    k = np.asarray(keys).astype(np.int64, copy=False).reshape(-1)
    s, c = np.asarray(sums, np.int64).reshape(-1), np.asarray(counts).astype(np.uint32, copy=False).reshape(-1)
    if not k.size == s.size == c.size:
        raise ValueError("records: keys, sums and counts of one length")
    if k.size == 0:
        return tuple(a.copy() for a in NO_RECORDS)
    order = np.argsort(k, kind="stable")
    k, s, c = k[order], s[order], c[order]
    first = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
    with np.errstate(over="ignore"):
        return k[first], np.add.reduceat(s, first, dtype=np.int64), np.add.reduceat(c, first, dtype=np.uint32)


class TsdfArchive:
    """The voxels of a rolled TsdfMap that are not on the device, on the host in numpy: per tile key (`tile_of`, 2^tile_bits
    voxels per axis) the records (key, sum, count) sorted by key, equal keys added.  The map it serves writes voxel_size,
    origin, distance, truncation and step into it at the first `TsdfMap.roll` (`save` / `load` carry them), and a map that
    differs in voxel_size, origin or distance is refused from then on: records of another grid or another unit cannot add."""
    META = ("voxel_size", "origin", "distance", "truncation", "step")

    def __init__(self, tile_bits: int = 5):
        if not ops.TSDF_TILE_BITS[0] <= int(tile_bits) <= ops.TSDF_TILE_BITS[1]:
            raise ValueError(f"tile_bits in [{ops.TSDF_TILE_BITS[0]}, {ops.TSDF_TILE_BITS[1]}]")
        self.tile_bits = int(tile_bits)
        self.tiles = {}                       # tile key (int) -> (keys, sums, counts)
        self.voxel_size = self.origin = self.distance = self.truncation = self.step = None

    def __len__(self) -> int:
        return sum(len(t[0]) for t in self.tiles.values())

    def bind(self, m: "TsdfMap"):
        """take the map's geometry at first use; later, refuse a map of another voxel_size, origin or distance"""
        if m.origin is None:
            raise ValueError("archive: the map has no origin yet")
        if self.voxel_size is None:
            self.voxel_size, self.origin, self.distance = m.voxel_size, m.origin.copy(), m.distance
            self.truncation, self.step = m.truncation, m.step
        elif (self.voxel_size != m.voxel_size or self.distance != m.distance
              or np.asarray(self.origin, np.float64).tobytes() != np.asarray(m.origin, np.float64).tobytes()):
            raise ValueError(f"archive: it holds voxels of voxel_size {self.voxel_size}, origin {self.origin}, distance "
                             f"'{self.distance}'; the map has {m.voxel_size}, {m.origin}, '{m.distance}'")
        return self

    def add(self, keys, sums, counts):
        k, s, c = merge_records(keys, sums, counts)
        if k.size and k.min() < 0:
            raise ValueError("archive: a key with bit 63 set is no voxel")
        tiles = tile_of(k, self.tile_bits)
        order = np.argsort(tiles, kind="stable")              # keeps the key order inside a tile
        tiles, k, s, c = tiles[order], k[order], s[order], c[order]
        edges = np.flatnonzero(np.concatenate([[True], tiles[1:] != tiles[:-1], [True]])) if k.size else []
        for lo, hi in zip(edges[:-1], edges[1:]):
            t, new = int(tiles[lo]), (k[lo:hi], s[lo:hi], c[lo:hi])
            held = self.tiles.get(t)
            self.tiles[t] = new if held is None else merge_records(*[np.concatenate(p) for p in zip(held, new)])
        return self

    def tiles_near(self, centre_map_xyz, radius: float, voxel_size: Optional[float] = None) -> np.ndarray:
        """the keys of the held tiles that are NEAR the centre (`tile_near`: the kernel's test), sorted"""
        v = self.voxel_size if voxel_size is None else voxel_size
        t = np.array(sorted(self.tiles), np.int64)
        return t[tile_near(t, self.tile_bits, centre_map_xyz, radius, v)] if t.size else t

    def take(self, tile_keys):
        """the records of these tiles, sorted by key; the tiles leave the archive (a tile it does not hold gives nothing)"""
        out = [self.tiles.pop(int(t)) for t in np.unique(np.asarray(tile_keys, np.int64)) if int(t) in self.tiles]
        return merge_records(*[np.concatenate(p) for p in zip(*out)]) if out else tuple(a.copy() for a in NO_RECORDS)

    def records(self):
        """everything held, sorted by key; nothing leaves"""
        out = list(self.tiles.values())
        return merge_records(*[np.concatenate(p) for p in zip(*out)]) if out else tuple(a.copy() for a in NO_RECORDS)

    def save(self, path):
        """one .npz: the records and voxel_size, origin, distance, truncation, step, tile_bits"""
        if self.voxel_size is None:
            raise ValueError("archive: no map has used it yet (voxel_size, origin and distance are unknown)")
        k, s, c = self.records()
        with open(path, "wb") as out:
            np.savez(out, keys=k, sums=s, counts=c, voxel_size=np.float64(self.voxel_size), origin=np.asarray(self.origin, np.float64),
                     distance=np.array(self.distance), truncation=np.float64(self.truncation), step=np.float64(self.step),
                     tile_bits=np.int64(self.tile_bits))

    @classmethod
    def load(cls, path) -> "TsdfArchive":
        with np.load(path, allow_pickle=False) as z:
            a = cls(int(z["tile_bits"]))
            a.voxel_size, a.origin, a.distance = float(z["voxel_size"]), z["origin"].astype(np.float64).reshape(3), str(z["distance"])
            a.truncation, a.step = float(z["truncation"]), float(z["step"])
            return a.add(z["keys"], z["sums"], z["counts"])


def merged_export(m: "TsdfMap", archive: TsdfArchive):
    """the sorted union of the map's export and the archive's records with equal keys added: what the map would export had it
    never been rolled"""
    return merge_records(*[np.concatenate(p) for p in zip(m.export(), archive.records())])


# -- meshing beyond the table: batches of owner tiles through one scratch table, merged on the host by vertex name -----------
def records_by_tile(keys, sums, counts, tile_bits: int) -> dict:
    """records -> {tile key: (keys, sums, counts) sorted by key, equal keys added}"""
    k, s, c = merge_records(keys, sums, counts)
    tiles = tile_of(k, tile_bits)
    order = np.argsort(tiles, kind="stable")
    tiles, k, s, c = tiles[order], k[order], s[order], c[order]
    edges = np.flatnonzero(np.concatenate([[True], tiles[1:] != tiles[:-1], [True]])) if k.size else []
    return {int(tiles[lo]): (k[lo:hi], s[lo:hi], c[lo:hi]) for lo, hi in zip(edges[:-1], edges[1:])}


def _axes(keys):
    k = np.asarray(keys, np.int64)
    return [(k >> (21 * a)) & _AXIS for a in range(3)]


def _pack(x, y, z):
    return np.asarray(x, np.int64) | (np.asarray(y, np.int64) << 21) | (np.asarray(z, np.int64) << 42)


def _halo(keys, owners, tile_bits: int) -> np.ndarray:
    """which voxels x does a cell or crossing anchored in one of the `owners` (sorted tile keys) read: tile_of(x - d) is an
    owner for some d in {-1, 0, 1, 2}^3 with x - d inside the 21 bits.  Per axis x - 2 .. x + 1 meets at most two tiles (a
    tile has at least 8 voxels), the one of the lowest and the one of the highest coordinate that exists: 8 candidates."""
    b, x = int(tile_bits), _axes(keys)
    ends = [(np.maximum(x[a] - 2, 0) >> b, np.minimum(x[a] + 1, _AXIS) >> b) for a in range(3)]
    out = np.zeros(len(x[0]), bool)
    for i in range(8):
        out |= np.isin(_pack(ends[0][i & 1], ends[1][(i >> 1) & 1], ends[2][i >> 2]), owners)
    return out


def _neighbours(owners, tile_bits: int) -> np.ndarray:
    """the tiles within one tile of an owner on every axis that are no owners themselves, sorted"""
    t, top = _axes(owners), _AXIS >> int(tile_bits)
    out = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                n = [t[0] + dx, t[1] + dy, t[2] + dz]
                ok = np.all([(c >= 0) & (c <= top) for c in n], axis=0)
                out.append(_pack(n[0][ok], n[1][ok], n[2][ok]))
    return np.setdiff1d(np.concatenate(out), owners)


def _needed_parts(by_tile: dict, owner_tiles, tile_bits: int):
    owners = np.unique(np.asarray(owner_tiles, np.int64).reshape(-1))
    parts = [by_tile[int(t)] for t in owners if int(t) in by_tile]
    for t in _neighbours(owners, tile_bits):
        held = by_tile.get(int(t))
        if held is not None:
            keep = _halo(held[0], owners, tile_bits)
            if keep.any():
                parts.append(tuple(a[keep] for a in held))
    return parts


def needed_records(by_tile: dict, owner_tiles, tile_bits: int):
    """what `mesh_indexed(tiles=owner_tiles)` and `surface(tiles=owner_tiles)` read, out of {tile key: records}: the owner tiles'
    own voxels and the HALO -- every voxel x of another tile with tile_of(x - d) among the owners for some d in {-1, 0, 1,
    2}^3: the 8 corners of an owned cell and the neighbours at +-1 of both ends of its edges, which the normals read.
    Coordinates outside the 21 bits do not exist.  -> (keys, sums, counts) sorted by key.  Host, numpy."""
    parts = _needed_parts(by_tile, owner_tiles, tile_bits)
    return merge_records(*[np.concatenate(p) for p in zip(*parts)]) if parts else tuple(a.copy() for a in NO_RECORDS)


def plan_batches(by_tile: dict, tile_bits: int, scratch_voxels: int):
    """the tiles of {tile key: records} in sorted order, grouped greedily into batches whose `needed_records` -- owners and
    halo -- number at most scratch_voxels // 2 -> [sorted tile keys (int64), ...]; every tile is in exactly one batch.  Half
    the table is a CONDITION for the open-addressing table to stay fast and free of overflow, not a measurement of it.  A
    single tile that does not fit raises ValueError."""
    room, out = int(scratch_voxels) // 2, []
    batch, own, halo = [], 0, {}          # the open batch: its tiles, their voxels, {neighbour tile: voxels of it the batch reads}

    def grown(t):
        """(records needed, halo) of the open batch with tile t added: only t's neighbours read anything new"""
        owners = np.array(sorted(batch + [t]), np.int64)
        h = {n: c for n, c in halo.items() if n != t}
        for n in _neighbours(np.array([t], np.int64), tile_bits).tolist():
            if n in by_tile and n not in batch:
                h[n] = int(_halo(by_tile[n][0], owners, tile_bits).sum())
        return own + len(by_tile[t][0]) + sum(h.values()), h

    for t in sorted(by_tile):
        size, h = grown(t)
        if batch and size > room:
            out.append(np.array(batch, np.int64))
            batch, own, halo = [], 0, {}
            size, h = grown(t)
        if size > room:
            raise ValueError(f"tile {t} needs {size} voxels with its halo, more than half of scratch_voxels={scratch_voxels}; "
                             f"raise scratch_voxels or lower tile_bits")
        batch, own, halo = batch + [t], own + len(by_tile[t][0]), h
    if batch:
        out.append(np.array(batch, np.int64))
    return out


def weld_indexed(batches):
    """indexed meshes of disjoint sets of cells -- [(vertices (v,3), faces (f,3), normals (v,3), vertex_keys (v,), vertex_dirs
    (v,)), ...], numpy -- merged by vertex name -> the same five in `weld`'s order.  A name has one position and one normal:
    a vertex on a seam comes with equal bytes from both sides, and the first is kept."""
    batches = [b for b in batches if len(b[3])]
    if not batches:
        return (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32), np.zeros(0, np.int64),
                np.zeros(0, np.int32))
    p, n = (np.concatenate([np.asarray(b[j], np.float32).reshape(-1, 3) for b in batches]) for j in (0, 2))
    k = np.concatenate([np.asarray(b[3], np.int64).reshape(-1) for b in batches])
    d = np.concatenate([np.asarray(b[4], np.int32).reshape(-1) for b in batches])
    base = np.cumsum([0] + [len(b[3]) for b in batches[:-1]])
    faces = np.concatenate([np.asarray(b[1], np.int64).reshape(-1, 3) + o for b, o in zip(batches, base)])
    index, keep = _first_index(k, d)
    return np.ascontiguousarray(p[keep]), _canonical_faces(index[faces]), np.ascontiguousarray(n[keep]), k[keep], d[keep]


def _batched(m: "TsdfMap", archive, scratch_voxels, batches, extract):
    """extract(scratch map, owner tiles, tile_bits) per batch (`batches`: lists of owner tiles; None: `plan_batches`) over the
    union of the map's export and the archive's records, each batch absorbed into ONE scratch TsdfMap on m's grid, cleared in
    between -> the results"""
    b = 5 if archive is None else archive.tile_bits
    parts = [m.export()] + ([] if archive is None else [archive.records()])
    by_tile = records_by_tile(*[np.concatenate(p) for p in zip(*parts)], b)
    n = m.max_voxels if scratch_voxels is None else int(scratch_voxels)
    out, scratch = [], None
    for owners in (plan_batches(by_tile, b, n) if batches is None else batches):
        if scratch is None:
            scratch = TsdfMap(m.voxel_size, m.truncation, m.step, n, m.min_range, m.max_range, origin=m.origin,
                              device=m.device if m.table is None else m.table.device, distance=m.distance, cos_min=m.cos_min)
        else:
            ops.tsdf_clear(scratch.table, scratch.max_voxels)
        scratch.absorb(*needed_records(by_tile, owners, b)).check()
        out.append(extract(scratch, owners, b))
    return out


def merged_mesh(m: "TsdfMap", archive: Optional[TsdfArchive] = None, min_count: float = 1, scratch_voxels: Optional[int] = None,
                batches=None):
    """the mesh of a map larger than the table -> (vertices (V,3) float32, faces (F,3) int32, normals (V,3) float32) numpy, in
    `weld`'s order.  The records of `m.export()` and `archive.records()` (None: the map alone; neither is changed) are cut
    into batches of tiles (`plan_batches`; scratch_voxels: a power of two, default m.max_voxels); each batch's
    `needed_records` go into one scratch TsdfMap, `mesh_indexed(tiles=owners)` meshes the cells it owns, and the batches are
    merged by vertex name (`weld_indexed`).  THE GUARANTEE: vertices and faces are the bytes of `mesh()`, normals those of
    `mesh_indexed().normals`, of the map that never rolled -- a voxel is (key, sum, count) with additive writes, and an owned
    cell reads nothing outside its batch's records.  Two host synchronisations a batch (check, V and F) and its copy.
    batches: the owner tiles of each batch, every tile once, in place of the planner's (a batch that does not fit raises)."""
    got = _batched(m, archive, scratch_voxels, batches, lambda s, owners, b: [t.cpu().numpy() for t in s.mesh_indexed(min_count, owners, b)])
    return weld_indexed(got)[:3]


def merged_surface(m: "TsdfMap", archive: Optional[TsdfArchive] = None, min_count: float = 1,
                   scratch_voxels: Optional[int] = None, batches=None) -> TsdfSurface:
    """`merged_mesh` for the zero crossings: `surface(tiles=owners)` per batch -> TsdfSurface with HOST tensors, sorted by (key,
    axis): the bytes of `surface()` of the map that never rolled"""
    got = _batched(m, archive, scratch_voxels, batches, lambda s, owners, b: s.surface(min_count, owners, b))
    rows = [(g.keys.cpu(), g.axes.cpu(), g.xyz_map.cpu().t(), g.normals.cpu().t()) for g in got]
    rows = rows or [(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0, 3), torch.zeros(0, 3))]
    return _surface_of(*[torch.cat(c) for c in zip(*rows)], np.zeros(3) if m.origin is None else m.origin.copy())


MISS, HIT, BACK = ops.TSDF_MISS, ops.TSDF_HIT, ops.TSDF_BACK
BLOCKS_OVERFLOW = "the occupied-block set is full (max_blocks={}): ray-casts with skip=True are undefined; raise max_blocks"


class TsdfMap(_HashedMap):
    """A TSDF of `max_voxels` slots (a power of two) with voxels of `voxel_size` metres.  truncation (default 3 voxel_size, at
    most 64 m): how far before and behind a return its ray is sampled, and the clamp of the distance; step (default
    voxel_size / 2): the spacing of the samples.  Coordinates are fp32 relative to `origin` (three float64; default: the
    translation of the first pose), so work far from the world's zero keeps fp32 accuracy.  A return counts when min_range
    <= |p| <= max_range in the sensor frame.  A map that ran out of slots is undefined: `overflow()` is then non-zero and
    `check()` raises ValueError.  The extractions synchronise once each and do not look at that word: call `check()` first.
    distance: "ray" (along the ray; the default) or "plane" (to the tangent plane at the return: `integrate` then needs
    normals), fixed for the map's life; cos_min in [0, 1]: in plane mode a return whose |cos(incidence)| is below it is left
    out and counted in `unusable()`."""

    def __init__(self, voxel_size: float = 0.2, truncation: Optional[float] = None, step: Optional[float] = None,
                 max_voxels: int = 1 << 22, min_range: float = 0.0, max_range: float = 100.0, origin=None, device=None,
                 distance: str = "ray", cos_min: float = 0.0, max_blocks: Optional[int] = None):
        if distance not in ("ray", "plane"):
            raise ValueError("distance is 'ray' or 'plane'")
        if not 0.0 <= float(cos_min) <= 1.0:
            raise ValueError("0 <= cos_min <= 1")
        self.distance, self.cos_min, self.unit = distance, float(cos_min), 256 if distance == "plane" else 1
        if not (voxel_size > 0 and float(np.float32(voxel_size)) > 0):
            raise ValueError("voxel_size > 0")
        if max_voxels < 2 or max_voxels > 1 << 24 or max_voxels & (max_voxels - 1):
            raise ValueError("max_voxels: a power of two in [2, 2^24]")
        self.voxel_size, self.max_voxels = float(voxel_size), int(max_voxels)
        self.max_blocks = max(2, self.max_voxels // 2) if max_blocks is None else int(max_blocks)
        if self.max_blocks < 2 or self.max_blocks > 1 << 24 or self.max_blocks & (self.max_blocks - 1):
            raise ValueError("max_blocks: a power of two in [2, 2^24]")
        self._blocks = {}     # min_count (count units) -> the occupied-block set of the table as it is; every write drops it
        self._ray_tables = {}   # id of a LidarModel's direction table -> (the table, its copy on the device): uploaded once
        self._spare = self._stage = None    # a rolling map's second table and its staging list: made by the first `evict`, kept
        self.wanted = 0                     # voxels the last `evict` wanted out (above its list's length: the rest stayed)
        self.truncation = 3.0 * self.voxel_size if truncation is None else float(truncation)
        self.step = self.voxel_size / 2.0 if step is None else float(step)
        self.min_range, self.max_range = float(min_range), float(max_range)
        ops.tsdf_rays(self.truncation, self.step, self.min_range, self.max_range)
        self.origin = None if origin is None else np.asarray(origin, np.float64).reshape(3).copy()
        self.device = device
        self.table: Optional[torch.Tensor] = None

    # -- plumbing (_ready, _list and _header are odometry._HashedMap's)
    def _new(self):
        self._blocks = {}
        return ops.tsdf_new(self.max_voxels, self.device)

    def _rays(self):
        return self.min_range, self.max_range, self.truncation, self.step

    def _map(self):
        return self.table, self.max_voxels, self.voxel_size, self.origin

    @staticmethod
    def _frame(what, pcd, pose, length):
        """-> (xyz (N,3), count (1,) int32 on the device) of an augment.PointCloud or of xyz with `length`"""
        if isinstance(pcd, torch.Tensor):
            xyz = pcd
            if xyz.dim() != 2 or xyz.shape[1] != 3:
                raise ValueError(f"{what}: xyz (N,3)")
            if isinstance(length, torch.Tensor):
                count = length.reshape(1)
            else:
                n = xyz.shape[0] if length is None else int(length)
                if not 0 <= n <= xyz.shape[0]:
                    raise ValueError(f"{what}: 0 <= length <= N")
                count = torch.full((1,), n, dtype=torch.int32).to(xyz.device)
        else:
            if length is not None:
                raise ValueError(f"{what}: a PointCloud carries its own length")
            xyz, count = pcd.xyz, pcd.count
        if tuple(np.shape(pose)) != (4, 4):
            raise ValueError("pose: (4,4)")
        return xyz, count

    def _estimated(self, xyz, count, radius):
        """dpm_point_normals of the frame's valid rows alone -> (N,3), zeros past them.  Reads the length: one synchronisation."""
        augment._SYNCS[0] += 1
        n = min(max(int(count.item()), 0), xyz.shape[0])
        out = torch.zeros_like(xyz)
        if n:
            lengths = torch.full((1,), n, dtype=torch.int32, device=xyz.device)
            out[:n] = ops.icp_target_normals(xyz[:n].t().contiguous()[None], lengths, lengths[:0], float(radius), host=([0], [n]))[0]
        return out

    # -- fusion: no host synchronisation
    def integrate(self, pcd, pose, length=None, normals=None):
        """one frame under `pose` (4,4 sensor -> world; numpy, or a tensor -- on the GPU it is read there): an
        augment.PointCloud, or xyz (N,3) float32 on the GPU with `length` (an int, or a (1,) int32 tensor on the GPU; None:
        N).  One launch.  distance="plane": `normals` is required -- (N,3) float32 on the GPU, in the SENSOR frame, unit length,
        either sign; or a radius in metres to estimate them from the frame alone (dpm_point_normals), which costs the host read
        of the length, the only synchronisation here.  distance="ray": normals must be None."""
        xyz, count = self._frame("integrate", pcd, pose, length)
        if (normals is None) != (self.distance == "ray"):
            raise ValueError("integrate: normals are required by distance='plane' and refused by distance='ray'")
        if isinstance(normals, torch.Tensor) and normals.shape != xyz.shape:
            raise ValueError("integrate: normals (N,3), one per row")
        self._ready(xyz.device, pose)
        if xyz.shape[0] == 0:
            return self
        self._blocks = {}
        if self.distance == "ray":
            ops.tsdf_integrate(*self._map(), xyz, count, _pose_tensor(pose, self.device), *self._rays())
        else:
            if not isinstance(normals, torch.Tensor):
                normals = self._estimated(xyz, count, normals)
            ops.tsdf_integrate_planes(*self._map(), xyz, normals, count, _pose_tensor(pose, self.device), *self._rays(), self.cos_min)
        return self

    def integrate_frames(self, store, lengths, frames, poses, normals=None):
        """stored frames under a pose each, in one launch for any number of them: row frames[f] of `store` (capacity,3,P) fp32
        channel-major / `lengths` (capacity,) int32 on the device (LoopCloser.store, .lengths) under poses[f] (F,4,4; sensor
        -> world).  frames / poses: host arrays (uploaded, nothing is read back) or device tensors.  The result is that of
        `integrate` of each entry, byte for byte.  distance="plane": normals (capacity,P,3) float32, the store's normals in
        each frame's own sensor frame (LoopCloser.normals), is required; distance="ray": it must be None."""
        if (normals is None) != (self.distance == "ray"):
            raise ValueError("integrate_frames: normals are required by distance='plane' and refused by distance='ray'")
        rows, poses = self._list("integrate_frames", store, frames, poses)
        self._ready(store.device, poses.reshape(-1, 4, 4)[0] if rows.numel() else None)
        if rows.numel() == 0:
            return self
        poses = poses.to(device=self.device, dtype=torch.float64).contiguous()
        self._blocks = {}
        if self.distance == "ray":
            ops.tsdf_integrate_frames(*self._map(), store, lengths, rows, poses, *self._rays())
        else:
            ops.tsdf_integrate_planes_frames(*self._map(), store, normals, lengths, rows, poses, *self._rays(), self.cos_min)
        return self

    # -- carving: no host synchronisation either
    def _carve_args(self, weight, margin):
        margin = self.truncation + self.voxel_size if margin is None else float(margin)
        return ops.tsdf_carve_args(max(1, int(round(float(weight) * self.unit))) if weight > 0 else 0, margin, self.step, self.max_range)

    def carve(self, pcd, pose, length=None, weight: float = 1.0, margin: Optional[float] = None):
        """the free space of one frame (the arguments of `integrate`): every voxel the map holds that a ray crosses before
        `margin` metres (default truncation + voxel_size) short of its return receives `weight` full-weight samples (times
        `unit`, at most 65535 count units) of "free, at the truncation distance".  Lookups only: no voxel is added.  Run it
        after the integrations.  Needs max_range / step <= 65536.  One launch."""
        xyz, count = self._frame("carve", pcd, pose, length)
        w, g = self._carve_args(weight, margin)
        if self.table is None or xyz.shape[0] == 0:      # an empty map holds nothing to carve
            return self
        self._blocks = {}
        ops.tsdf_carve(*self._map(), xyz, count, _pose_tensor(pose, self.device), *self._rays(), w, g)
        return self

    def carve_frames(self, store, lengths, frames, poses, weight: float = 1.0, margin: Optional[float] = None):
        """`carve` of a list of stored frames (the arguments of `integrate_frames`) in one launch"""
        rows, poses = self._list("carve_frames", store, frames, poses)
        w, g = self._carve_args(weight, margin)
        if self.table is None or rows.numel() == 0:
            return self
        self._blocks = {}
        ops.tsdf_carve_frames(*self._map(), store, lengths, rows, poses.to(device=self.device, dtype=torch.float64).contiguous(),
                              *self._rays(), w, g)
        return self

    # -- rolling: far tiles leave for the host and come back by addition
    def evict(self, pose, radius: float, tile_bits: int = 5, max_out: Optional[int] = None):
        """the voxels of every tile (2^tile_bits voxels per axis) whose centre is farther than `radius` metres from the
        translation of `pose` ((4,4); numpy, or a tensor -- on the GPU it is read there) leave the map -> (keys int64, sums
        int64, counts uint32) numpy, sorted by key.  The table is rebuilt into a second one (nothing can be deleted in place),
        made at the first call and kept with a staging list of max_voxels // 4 records: A ROLLING MAP COSTS TWICE THE TABLE, and
        24 bytes for every four slots.  The two tables change places.  max_out (default: the staging list's length): at most so
        many voxels leave; those that found no room STAY in the map for the next call, and `wanted` is the number that wanted
        out.  Two launches and one host synchronisation, the read of that number."""
        if not ops.TSDF_TILE_BITS[0] <= int(tile_bits) <= ops.TSDF_TILE_BITS[1] or not 0.0 <= float(radius) < 1e18:
            raise ValueError(f"evict: radius >= 0, tile_bits in [{ops.TSDF_TILE_BITS[0]}, {ops.TSDF_TILE_BITS[1]}]")
        if max_out is not None and int(max_out) < 0:
            raise ValueError("evict: max_out >= 0")
        if tuple(np.shape(pose)) != (4, 4):
            raise ValueError("pose: (4,4)")
        self.wanted = 0
        if self.table is None:
            return tuple(a.copy() for a in NO_RECORDS)
        dev = self.table.device
        if self._spare is None:
            n = max(1, self.max_voxels // 4)
            with torch.cuda.device(dev):
                self._spare = torch.empty_like(self.table)
                self._stage = (torch.empty(n, device=dev, dtype=torch.int64), torch.empty(n, device=dev, dtype=torch.int64),
                               torch.empty(n, device=dev, dtype=torch.int32), torch.empty(1, device=dev, dtype=torch.int32))
        keys, sums, counts, count = self._stage
        n = keys.numel() if max_out is None else int(max_out)
        if n > keys.numel():                       # a longer list than the one kept: made for this call
            with torch.cuda.device(dev):
                keys, sums, counts = (torch.empty(n, device=dev, dtype=t.dtype) for t in (keys, sums, counts))
        ops.tsdf_evict(self.table, self._spare, self.max_voxels, self.voxel_size, self.origin, _pose_tensor(pose, self.device),
                       radius, tile_bits, keys[:n], sums[:n], counts[:n], count)
        self.table, self._spare = self._spare, self.table
        self._blocks = {}
        augment._SYNCS[0] += 1
        self.wanted = int(count.item())
        n = min(self.wanted, n)
        return merge_records(keys[:n].cpu().numpy(), sums[:n].cpu().numpy(), counts[:n].cpu().numpy().view(np.uint32))

    def absorb(self, keys, sums=None, counts=None):
        """records (key, sum, count) -- numpy, or tensors on the device (int64, int64, int32 holding the uint32 bits) -- are
        added to the map: equal keys and keys the map holds add, in any order to the same bytes; count 0 is skipped, a key with
        bit 63 set is counted in `outside()`.  absorb(archive) takes EVERYTHING a TsdfArchive holds out of it, after checking
        voxel_size, origin and distance.  One launch, no host synchronisation."""
        if isinstance(keys, TsdfArchive):
            if sums is not None or counts is not None:
                raise ValueError("absorb: an archive, or keys, sums and counts")
            archive = keys
            if archive.voxel_size is None:
                raise ValueError("absorb: the archive was never used by a map")
            if self.origin is None:
                self.origin = np.asarray(archive.origin, np.float64).copy()
            archive.bind(self)
            keys, sums, counts = archive.take(list(archive.tiles))
        elif sums is None or counts is None:
            raise ValueError("absorb: keys, sums and counts")
        dev = self.device if self.device is not None else (keys.device if isinstance(keys, torch.Tensor) else augment._device())
        self._ready(torch.device(dev))
        if not isinstance(keys, torch.Tensor):
            k = np.ascontiguousarray(np.asarray(keys).astype(np.int64, copy=False).reshape(-1))      # uint64 keys: the same bits
            s = np.ascontiguousarray(np.asarray(sums, np.int64).reshape(-1))
            c = np.ascontiguousarray(np.asarray(counts).astype(np.uint32, copy=False).reshape(-1)).view(np.int32)
            if not k.size == s.size == c.size:
                raise ValueError("absorb: keys, sums and counts of one length")
            keys, sums, counts = (torch.from_numpy(a).to(self.table.device) for a in (k, s, c))
        if keys.numel():
            self._blocks = {}
            ops.tsdf_absorb(self.table, self.max_voxels, keys, sums, counts)
        return self

    def reach(self, tile_bits: int = 5) -> float:
        """R0: no ray of a frame at a pose touches a voxel, by `integrate` or `carve`, outside the tiles whose centre lies within
        R0 of the pose's translation.  A sample lies within max_range + ceil(truncation / step) * step of it (a carve's, before
        the return), inside its voxel, inside its tile, so within sqrt(3)/2 tile sides of the tile's centre; a voxel_size is
        added for the fp32 rounding of the samples and of the test.  The distance along the ray is taken no smaller than the
        carve's default margin, truncation + voxel_size."""
        along = max(float(np.ceil(self.truncation / self.step)) * self.step, self.truncation + self.voxel_size)
        return self.max_range + along + 0.5 * np.sqrt(3.0) * (1 << int(tile_bits)) * self.voxel_size + self.voxel_size

    def roll(self, pose, archive: TsdfArchive, keep_radius: Optional[float] = None, load_radius: Optional[float] = None,
             slack: float = 10.0):
        """move the map's window to `pose` ((4,4) ON THE HOST: the archive's lookup is there): `evict(pose, keep_radius)` ->
        `archive.add` -> `archive.take(archive.tiles_near(pose, load_radius))` -> `absorb`.  Defaults: load_radius = `reach()` +
        slack and keep_radius = load_radius + slack; keep_radius < load_radius raises (a tile would be loaded and evicted by
        turns).  THE GUARANTEE, under the default radii and while the sensor stays within `slack` of the last roll's centre:
        every tile a frame can touch is whole on the device, so integrate, carve and every read within `reach()` of the sensor
        give the bytes of a map that never rolled, and `merged_export` equals that map's export.  With smaller radii
        integrate alone is still exact in `merged_export` (addition), carve and the reads are not.  Not guaranteed: anything
        once `overflow()` is non-zero; reads beyond the window."""
        if isinstance(pose, torch.Tensor):
            raise ValueError("roll: pose on the host (the archive is looked up there)")
        P = np.asarray(pose, np.float64)
        if P.shape != (4, 4):
            raise ValueError("pose: (4,4)")
        if not float(slack) >= 0.0:
            raise ValueError("roll: slack >= 0")
        load = self.reach(archive.tile_bits) + float(slack) if load_radius is None else float(load_radius)
        keep = load + float(slack) if keep_radius is None else float(keep_radius)
        if not keep >= load >= 0.0:
            raise ValueError("roll: keep_radius >= load_radius >= 0")
        if self.origin is None:
            self.origin = P[:3, 3].copy() if archive.origin is None else np.asarray(archive.origin, np.float64).copy()
        archive.bind(self)
        archive.add(*self.evict(P, keep, archive.tile_bits))
        back = archive.take(archive.tiles_near(P[:3, 3] - self.origin, load, self.voxel_size))
        if len(back[0]):
            self.absorb(*back)
        return self

    # -- read-back: one host synchronisation each
    def overflow(self) -> int:
        """samples that found no free slot so far (0: the map is defined)"""
        return self._header(0)

    def outside(self) -> int:
        """samples that fell outside the 21-bit key range so far (they are left out)"""
        return self._header(1)

    def unusable(self) -> int:
        """plane mode: returns that passed the range gate so far and were left out for their normal -- zero, NaN, or with
        |cos(incidence)| below 1/512 or below cos_min"""
        return self._header(2)

    def _min_count(self, min_count) -> int:
        """min_count in full-weight samples -> the kernel's count units"""
        if not float(min_count) > 0:
            raise ValueError("min_count > 0")
        return max(1, int(round(float(min_count) * self.unit)))

    def check(self):
        n = self.overflow()
        if n:
            raise ValueError(OVERFLOW.format(self.max_voxels) + f" ({n} samples)")
        for blocks in self._blocks.values():          # one read per cached block set
            augment._SYNCS[0] += 1
            n = int(blocks[:4].view(torch.int32).item()) & 0xFFFFFFFF
            if n:
                raise ValueError(BLOCKS_OVERFLOW.format(self.max_blocks) + f" ({n} voxels)")
        return self

    def _extract(self, fn, *args):
        """fn(table, max_voxels, *args) without its count: the one read of that count is the extraction's synchronisation"""
        augment._SYNCS[0] += 1
        return fn(self.table, self.max_voxels, *args)[1:]

    def export(self):
        """(keys (n,) int64, sums (n,) int64 in units of 2^-24 m, counts (n,) uint32) numpy, sorted by key: the same bytes
        whatever the order the frames arrived in"""
        if self.table is None:
            return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.uint32)
        keys, sums, counts = [t.cpu().numpy() for t in self._extract(ops.tsdf_export)]
        order = np.argsort(keys, kind="stable")
        return keys[order], sums[order], counts[order].view(np.uint32)

    def field(self, min_count: float = 1):
        """(keys (m,) int64, D (m,) float32 metres) of the qualified voxels (count >= min_count), sorted by key; D > 0 on the
        sensor's side of the surface.  min_count, here and below, is in full-weight samples: max(1, round(min_count * unit))
        is what the count is compared with."""
        min_count = self._min_count(min_count)
        keys, sums, counts = self.export()
        ok = counts >= np.uint32(min_count)
        return keys[ok], field_values(sums[ok], counts[ok])

    def surface(self, min_count: float = 1, tiles=None, tile_bits: int = 5) -> TsdfSurface:
        """the zero crossings of the field along the axes between qualified voxels, with normals from the field's gradient.
        tiles (as `mesh_indexed` takes them): only the crossings whose voxel k0 lies in one of these tiles, with the bytes
        they have among all of them."""
        min_count = self._min_count(min_count)
        if self.table is None:
            dev = self.device if self.device is not None else "cpu"
            z = torch.zeros(0, 3, dtype=torch.float32, device=dev)
            return _surface_of(z[:, 0].long(), z[:, 0].int(), z, z, np.zeros(3) if self.origin is None else self.origin)
        if tiles is None:
            rows = self._extract(ops.tsdf_surface, self.voxel_size, min_count)
        else:
            rows = self._extract(ops.tsdf_surface_tiles, self.voxel_size, min_count, self._owners("surface", tiles, tile_bits), tile_bits)
        return _surface_of(*rows, self.origin.copy())

    def _owners(self, what, tiles, tile_bits):
        """tile keys (any order, repeats allowed) -> (n,) int64 on the table's device, sorted and unique, as the kernels need"""
        if not ops.TSDF_TILE_BITS[0] <= int(tile_bits) <= ops.TSDF_TILE_BITS[1]:
            raise ValueError(f"{what}: tile_bits in [{ops.TSDF_TILE_BITS[0]}, {ops.TSDF_TILE_BITS[1]}]")
        t = np.unique(np.asarray(tiles.cpu() if isinstance(tiles, torch.Tensor) else tiles, np.int64).reshape(-1))
        if t.size == 0:
            raise ValueError(f"{what}: tiles names no tile (None: every tile)")
        return torch.from_numpy(t).to(self.table.device)

    def mesh_indexed(self, min_count: float = 1, tiles=None, tile_bits: int = 5) -> TsdfMesh:
        """`mesh` welded on the device -> TsdfMesh, on the device, in `weld`'s order: vertices sorted by name (key, direction),
        every face rotated so that its smallest index leads, faces sorted by row; with tiles=None `vertices` and `faces` have
        the bytes of `mesh()`.  `normals`: per vertex, `surface`'s rule on the edge the vertex lies on (its bytes on the axis
        edges).  tiles: tile keys (`tile_of`, 2^tile_bits voxels per axis; host array or tensor, any order) -- only the cells
        whose base voxel lies in one of them are meshed; what such a cell reads is not cut, so its vertices may be named by
        voxels of a neighbouring tile.  One host synchronisation, the read of V and F; the sorts run on the device."""
        min_count = self._min_count(min_count)
        if self.table is None:
            dev = self.device if self.device is not None else "cpu"
            z = torch.zeros(0, 3, dtype=torch.float32, device=dev)
            return TsdfMesh(z, torch.zeros(0, 3, dtype=torch.int32, device=dev), z.clone(), torch.zeros(0, dtype=torch.int64, device=dev),
                            torch.zeros(0, dtype=torch.int32, device=dev))
        own = None if tiles is None else self._owners("mesh_indexed", tiles, tile_bits)
        augment._SYNCS[0] += 1
        _, keys, dirs, xyz, normals, faces = ops.tsdf_mesh_indexed(self.table, self.max_voxels, self.voxel_size, min_count, own, tile_bits)
        order = _by_name(keys, dirs)
        rank = torch.empty_like(order)
        rank[order] = torch.arange(order.numel(), device=order.device)
        faces = rank[faces.long()]
        lead = faces.argmin(dim=1, keepdim=True)                      # a triangle's three names differ: no ties
        faces = torch.gather(faces, 1, (lead + torch.arange(3, device=faces.device)) % 3)
        rows = torch.arange(faces.shape[0], device=faces.device)
        for col in (2, 1, 0):
            rows = rows[torch.sort(faces[rows, col], stable=True).indices]
        return TsdfMesh(xyz[order], faces[rows].to(torch.int32), normals[order], keys[order], dirs[order])

    def mesh(self, min_count: float = 1):
        """(vertices (V,3) float32 in the map frame -- world = vertices + origin --, faces (F,3) int32) from marching
        tetrahedra over the cells whose 8 corner voxels are qualified; welded by vertex name and sorted (`weld`); a face's
        normal (b - a) x (c - a) points to free space"""
        min_count = self._min_count(min_count)
        if self.table is None:
            return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
        return weld(*[t.cpu().numpy() for t in self._extract(ops.tsdf_mesh, self.voxel_size, min_count)])

    write_ply = staticmethod(write_ply)

    # -- the field at points, and registration against it: lookups only, no host synchronisation
    def sample(self, pcd, pose, length=None, min_count: float = 1):
        """the field at the frame's rows under `pose` (the arguments of `integrate`) -> (d (N,) float32 metres, grad (N,3)
        float32 in the map frame's axes, flag (N,) int32) on the device.  d is the trilinear interpolant of D between the 8
        voxel centres round the point and grad its exact gradient inside that cell; flag 1: the point has a value -- all 8
        voxels hold min_count full-weight samples --, 0: it has none (d and grad are zeros; a missing corner is never read as
        0), -1: a row at or past the length.  One launch."""
        min_count = self._min_count(min_count)
        xyz, count = self._frame("sample", pcd, pose, length)
        self._ready(xyz.device, pose)
        return ops.tsdf_sample(*self._map(), xyz, count, _pose_tensor(pose, self.device), min_count)

    def register(self, pcd, init, schedule=None, kernel_scale: float = 0.0, tol_rot: float = 1e-7, tol_trans: float = 1e-6,
                 min_count: float = 1, grad_min: float = 0.5, debug: bool = False, length=None):
        """Gauss-Newton of the frame (the arguments of `integrate`) against the field from `init` (4,4): the residual of a
        point is the field's value there, its Jacobian the field's gradient, so no correspondence is searched.  schedule =
        [(max_dist, max_iter), ...] (None: ((truncation, 30),)); a row is given when the point has a value with |d| <= max_dist
        and |grad| >= grad_min, which keeps the flat, clamped parts of the field out; a max_dist above the truncation raises.
        -> refine.IcpResult with one problem (pose (1,4,4) float64, ...), all on the device[, (flag (N,) int32, system (29,)
        float64) with debug].  fitness = rows / length.  An empty or unallocated map gives NO_MATCH and the pose `init`."""
        schedule = ((self.truncation, 30),) if schedule is None else [(float(d), int(n)) for d, n in schedule]
        if any(not 0.0 < d <= self.truncation for d, _ in schedule):
            raise ValueError("register: every max_dist of the schedule must lie in (0, truncation] (beyond the clamp the field is flat)")
        min_count = self._min_count(min_count)
        xyz, count = self._frame("register", pcd, init, length)
        start = _pose_tensor(init, xyz.device if self.device is None else self.device)
        if self.table is None or xyz.shape[0] == 0:      # nothing to look up: the kernel's answer to an empty table
            dev = start.device
            pose = start.clone().reshape(1, 4, 4)
            pose[0, 3] = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64, device=dev)
            res = IcpResult(pose, torch.zeros(1, device=dev), torch.zeros(1, device=dev),
                            torch.zeros(1, dtype=torch.int32, device=dev), torch.full((1,), NO_MATCH, dtype=torch.int32, device=dev))
            extra = (torch.full((xyz.shape[0],), -1, dtype=torch.int32, device=dev), torch.zeros(ops.ICP_NSUM, dtype=torch.float64, device=dev))
            return (res, extra) if debug else res
        out = ops.tsdf_register(*self._map(), self.truncation, xyz, count, start, schedule, kernel_scale, tol_rot, tol_trans,
                                min_count, grad_min, debug=debug)
        res = IcpResult(out[0].reshape(1, 4, 4), *out[1:5])
        return (res, out[5:]) if debug else res

    # -- looking at the map as the sensor does: lookups only, no host synchronisation
    def blocks(self, min_count: float = 1) -> torch.Tensor:
        """the occupied-block set of the table as it is now for `min_count` (full-weight samples): built on first use, kept
        until a method writes the table.  `check()` reports a set that ran out of room (max_blocks)."""
        mc = self._min_count(min_count)
        if self.table is None:
            raise ValueError("blocks: the map holds no table yet")
        if mc not in self._blocks:
            self._blocks[mc] = ops.tsdf_blocks(self.table, self.max_voxels, mc, self.max_blocks)
        return self._blocks[mc]

    def _cast_device(self, dirs=None):
        if self.device is not None:
            return torch.device(self.device)
        return dirs.device if dirs is not None and dirs.is_cuda else augment._device()

    def _ray_table(self, model) -> torch.Tensor:
        """model.directions() on the device, uploaded at its first use: later casts of the model copy nothing"""
        table = model.directions()
        held = self._ray_tables.get(id(table))
        if held is None or held[0] is not table:      # a map lives on one device
            held = self._ray_tables[id(table)] = (table, torch.from_numpy(table).to(self._cast_device()))
        return held[1]

    def raycast(self, poses, rays, min_range: Optional[float] = None, max_range: Optional[float] = None,
                step: Optional[float] = None, min_count: float = 1, skip: bool = True) -> TsdfCast:
        """what a sensor at each of `poses` ((4,4) or (F,4,4), sensor -> world; numpy, or a tensor -- on the GPU it is read
        there) sees in the map along `rays`: a lidar_sim.LidarModel (its directions(), and its range limits as the defaults), or
        (R,3) float32 unit directions in the sensor frame (numpy or tensor; the defaults are then the map's min_range and
        max_range).  The ray is sampled every `step` metres (default: the map's) from min_range to max_range and ends at the
        first sign change between two samples that both have a value (all 8 voxels round them hold min_count full-weight
        samples) -> TsdfCast(range (F,R), normals (F,R,3) in the sensor frame, flag (F,R): MISS / HIT / BACK).  skip: pass
        empty space by the occupied-block set (the same bytes as skip=False, which looks up every sample).  One launch (and the
        set's two at first use).  An unallocated map gives MISS everywhere."""
        mc = self._min_count(min_count)
        if hasattr(rays, "directions"):
            lo, hi, dirs = rays.min_range, rays.max_range, self._ray_table(rays)
        else:
            lo, hi, dirs = self.min_range, self.max_range, rays
        lo, hi, h = ops.tsdf_cast_args(lo if min_range is None else min_range, hi if max_range is None else max_range,
                                       self.step if step is None else step)
        if not isinstance(poses, torch.Tensor):
            poses = torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float64))
        if poses.dim() == 2:
            poses = poses[None]
        if poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4) or poses.shape[0] > 65535:
            raise ValueError("raycast: poses (4,4) or (F,4,4), F <= 65535")
        if not isinstance(dirs, torch.Tensor):
            dirs = torch.from_numpy(np.ascontiguousarray(dirs))
        if dirs.dim() != 2 or dirs.shape[1] != 3 or dirs.dtype != torch.float32:
            raise ValueError("raycast: rays is a LidarModel or (R,3) float32 directions")
        dev = self._cast_device(dirs)
        poses, dirs = poses.to(device=dev, dtype=torch.float64).contiguous(), dirs.to(dev).contiguous()
        F, R = poses.shape[0], dirs.shape[0]
        if self.table is None:
            return TsdfCast(torch.zeros(F, R, device=dev), torch.zeros(F, R, 3, device=dev), torch.zeros(F, R, dtype=torch.int32, device=dev))
        return TsdfCast(*ops.tsdf_raycast(*self._map(), self.blocks(min_count) if skip else None, self.max_blocks, poses, dirs,
                                          lo, hi, h, mc))

    def render(self, pose, model, min_count: float = 1):
        """the scan `model` (a lidar_sim.LidarModel) would take of the map from `pose` (4,4) -> (augment.PointCloud, normals):
        xyz = direction * range in the SENSOR frame of the HIT rays only, compacted in ray order on the device (the frame's
        count stays there); idx = the ray index, so ring and column stay recoverable as for the simulator's frames; R, T = the
        pose when it is on the host; normals (rays,3) float32 = the matching rows, zeros past the count.  Taken as it is by
        ScanContext, transform_frames, `integrate(..., normals=)` and `register`."""
        if tuple(np.shape(pose)) != (4, 4):
            raise ValueError("render: pose (4,4)")
        cast = self.raycast(pose, model, min_count=min_count)
        dev = cast.range.device
        dirs = self._ray_table(model)
        n = dirs.shape[0]
        host = None if isinstance(pose, torch.Tensor) else np.asarray(pose, np.float64)
        pcd = augment.PointCloud.from_buffers(dirs * cast.range[0][:, None], torch.arange(n, device=dev, dtype=torch.int32),
                                              torch.full((1,), n, device=dev, dtype=torch.int32),
                                              R=None if host is None else host[:3, :3].copy(),
                                              T=None if host is None else host[:3, 3:].copy(), host_n=None)
        if n == 0:
            return pcd, cast.normals[0]
        pcd = augment.mask_select(pcd, u=(cast.flag[0] == HIT).to(torch.float32), ratio=0.5)    # keeps u >= ratio, in ray order
        kept = torch.arange(n, device=dev) < pcd.count                                           # rows past the count are not defined
        rows = torch.where(kept, pcd.idx.long(), torch.zeros_like(kept, dtype=torch.long))
        return pcd, cast.normals[0][rows] * kept[:, None]


class TsdfStep(NamedTuple):
    """what `TsdfTracker.step` did with a frame: the registration's status, fitness, rmse and iterations on the host, and whether
    the frame was integrated"""
    status: int
    fitness: float
    rmse: float
    iterations: int
    integrated: bool


class TsdfTracker:
    """Frame-to-model odometry on one TsdfMap: every frame is registered against the fused field (`TsdfMap.register`) and then
    fused into it under the registered pose.  The constructor takes TsdfMap's arguments and schedule, kernel_scale, min_count,
    grad_min (those of `register`), min_fitness and register_every: the registration reads every register_every-th row of the
    frame, the integration all of them.  `poses` is the trajectory ((4,4) float64 on the host), `steps` a TsdfStep per frame,
    `lost` the number of frames whose registration failed.

    archive: a TsdfArchive (True: a new one of `tile_bits`) makes the map ROLL: at the start pose of a frame, before its
    registration, whenever that pose's translation is at least slack / 2 from the centre of the last roll (the first frame's
    pose counts as one), `TsdfMap.roll(start, archive, slack=slack)` sends the far tiles to the host and fetches the near ones, so
    the trajectory may be longer than max_voxels covers; `rolls` counts them.  The poses and steps are those of the tracker
    without an archive, byte for byte, while that one does not overflow and the frames' rows lie within max_range: a
    registration reads the field at every row, and beyond the window the rolled map's tiles are on the host.  It costs the
    second table and one more synchronisation per roll.  Without an archive nothing changes.

    What it is NOT: no deskew (a sweep is taken as one rigid frame), no pruning without an archive (the map then only grows, to
    max_voxels), no loop closure, no coarse level (the start must lie within the truncation band), and no normals of its own:
    distance="plane" needs them per frame, as `TsdfMap.integrate` does."""

    def __init__(self, voxel_size: float = 0.2, truncation: Optional[float] = None, step: Optional[float] = None,
                 max_voxels: int = 1 << 22, min_range: float = 0.0, max_range: float = 100.0, origin=None, device=None,
                 distance: str = "ray", cos_min: float = 0.0, schedule=None, kernel_scale: float = 0.0, min_count: float = 1,
                 grad_min: float = 0.5, min_fitness: float = 0.3, register_every: int = 1, archive=None, slack: float = 10.0,
                 tile_bits: int = 5):
        self.map = TsdfMap(voxel_size, truncation, step, max_voxels, min_range, max_range, origin, device, distance, cos_min)
        if int(register_every) < 1:
            raise ValueError("register_every >= 1")
        if not float(slack) > 0.0:
            raise ValueError("slack > 0")
        self.archive = TsdfArchive(tile_bits) if archive is True else archive
        self.slack, self.rolls, self._rolled = float(slack), 0, None    # _rolled: the centre of the last roll
        self.schedule, self.kernel_scale, self.min_count, self.grad_min = schedule, float(kernel_scale), min_count, float(grad_min)
        self.min_fitness, self.register_every = float(min_fitness), int(register_every)
        self.poses, self.steps, self.lost = [], [], 0

    def predict(self) -> np.ndarray:
        """the constant-velocity prediction from the last two poses, float64 on the host (one pose: that pose)"""
        if len(self.poses) < 2:
            return self.poses[-1].copy()
        return self.poses[-1] @ (np.linalg.inv(self.poses[-2]) @ self.poses[-1])

    def predicted(self, model):
        """the scan the map predicts for the next frame: `TsdfMap.render` at the constant-velocity prediction, with the
        tracker's min_count -> (augment.PointCloud, normals).  `step` does not use it."""
        if not self.poses:
            raise ValueError("predicted: no frame yet")
        return self.map.render(self.predict(), model, min_count=self.min_count)

    def step(self, pcd, normals=None, pose=None):
        """one frame (an augment.PointCloud, or xyz (N,3) float32 on the GPU; normals as `TsdfMap.integrate` takes them) ->
        (pose (4,4) float64, TsdfStep).  The first frame is integrated under `pose` (default: the identity).  A later frame starts from `pose` if given, else
        from the prediction; it is registered, pose, status and fitness are fetched in ONE host read -- the step's only
        synchronisation when the normals come as a tensor -- and when the status is CONVERGED or MAX_ITER with fitness >=
        min_fitness the WHOLE frame is integrated under the registered pose.  Otherwise the start is kept as the pose,
        nothing is integrated and `lost` counts the frame: a failed registration never writes to the map."""
        m = self.map
        xyz, length = m._frame("step", pcd, np.eye(4), None)
        if not self.poses:
            P = np.eye(4) if pose is None else np.array(pose, np.float64).reshape(4, 4)
            m.integrate(xyz, P, length, normals)
            self._rolled = P[:3, 3].copy()
            done = TsdfStep(CONVERGED, 1.0, 0.0, 0, True)
        else:
            start = self.predict() if pose is None else np.array(pose, np.float64).reshape(4, 4)
            if self.archive is not None and np.linalg.norm(start[:3, 3] - self._rolled) >= 0.5 * self.slack:
                m.roll(start, self.archive, slack=self.slack)
                self._rolled, self.rolls = start[:3, 3].copy(), self.rolls + 1
            k = self.register_every
            rows, count = xyz, length
            if k > 1:                                   # rows 0, k, 2k, ... below the length: ceil(length / k) of them, formed on the device
                rows, count = xyz[::k].contiguous(), torch.div(length + (k - 1), k, rounding_mode="floor").to(torch.int32)
            res = m.register(rows, start, self.schedule, self.kernel_scale, min_count=self.min_count, grad_min=self.grad_min,
                             length=count)
            augment._SYNCS[0] += 1
            host = torch.cat([res.pose.reshape(16), res.fitness.double(), res.rmse.double(), res.iterations.double(),
                              res.status.double()]).cpu().numpy()
            status, fitness = int(host[19]), float(host[16])
            ok = status in (CONVERGED, MAX_ITER) and fitness >= self.min_fitness
            P = host[:16].reshape(4, 4).copy() if ok else start
            if ok:
                m.integrate(xyz, P, length, normals)
            else:
                self.lost += 1
            done = TsdfStep(status, fitness, float(host[17]), int(host[18]), ok)
        self.poses.append(P)
        self.steps.append(done)
        return P, done
