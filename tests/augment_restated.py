"""numpy / torch-CPU restatement of the training transforms (reference dataloader/transforms.py), every random quantity an
explicit argument, held to the reference's own outputs by tests/test_augment_host.py and used as the checker of the HIP
kernels by tests/test_gpu_augment.py.

Selections return the kept INPUT POSITIONS (int64, in output order).  Where the reference's result is not reproducible
(GroundFilter's order and representatives: unstable np.argsort over cell ids) the restatement is the stable definition the
library documents, and the tests compare what the two share: the non-ground set, the sparse cells, and that a
representative is the lowest position of its cell."""
import math

import numpy as np
import torch

F32_ULP_180 = 2.0 ** -16          # one float32 ulp at 128..256
BAND_ULPS = 64


# ---------------------------------------------------------------------------------------------- selections
def ground_cells(xyz, img_len, img_width, grid_width):
    """cell id per point (-1 outside the image): int32(x / grid_width + img_len / 2) in float32, truncating"""
    xyz = np.asarray(xyz, dtype=np.float32)
    row = (xyz[:, 0] / np.float32(grid_width) + np.float32(img_len / 2)).astype(np.int32)
    col = (xyz[:, 1] / np.float32(grid_width) + np.float32(img_width / 2)).astype(np.int32)
    inside = (row >= 0) & (row < img_len) & (col >= 0) & (col < img_width)
    return np.where(inside, row.astype(np.int64) * img_width + col, -1)


def ground_filter(xyz, img_len, img_width, grid_width, ground_height, preserve_sparse_ground=True):
    """-> dict(keep (ascending positions), nonground (positions), sparse_cells (cell ids), reps (positions))"""
    xyz = np.asarray(xyz, dtype=np.float32)
    n = xyz.shape[0]
    if ground_height <= 0:
        return dict(keep=np.arange(n), nonground=np.arange(n), sparse_cells=np.zeros(0, np.int64), reps=np.zeros(0, np.int64))
    cell = ground_cells(xyz, img_len, img_width, grid_width)
    ncell = img_len * img_width
    ins = np.nonzero(cell >= 0)[0]
    cnt = np.bincount(cell[ins], minlength=ncell)
    zmin = np.full(ncell, np.inf, np.float32)
    zmax = np.full(ncell, -np.inf, np.float32)
    first = np.full(ncell, n, np.int64)
    np.minimum.at(zmin, cell[ins], xyz[ins, 2])
    np.maximum.at(zmax, cell[ins], xyz[ins, 2])
    np.minimum.at(first, cell[ins], ins)
    with np.errstate(invalid="ignore"):
        high = (zmax - zmin) > np.float32(ground_height)
    non_cell, sparse_cell = (cnt >= 3) & high, (cnt >= 3) & ~high
    nonground = ins[non_cell[cell[ins]]]
    reps = first[sparse_cell] if preserve_sparse_ground else np.zeros(0, np.int64)
    return dict(keep=np.sort(np.concatenate([nonground, reps])), nonground=nonground,
                sparse_cells=np.nonzero(sparse_cell)[0] if preserve_sparse_ground else np.zeros(0, np.int64), reps=reps)


def check_ground(g, name, xyz, keep):
    """the comparison the ground filter is held to: non-ground SET equal to the reference's, sparse-cell SET equal, every
    representative the lowest position of its cell, kept positions ascending"""
    L, W, gw, gh = g[name + ".params"]
    L, W = int(L), int(W)
    ref, k = g[name + ".idx"].astype(np.int64), int(g[name + ".n_nonground"])
    cell = ground_cells(xyz, L, W, gw)
    keep = np.asarray(keep, dtype=np.int64)
    assert np.all(np.diff(keep) > 0)
    ref_non, ref_sparse_cells = set(ref[:k].tolist()), set(cell[ref[k:]].tolist())
    assert len(ref_sparse_cells) == ref.shape[0] - k
    non_cells = set(cell[ref[:k]].tolist())
    got_non = [i for i in keep.tolist() if cell[i] in non_cells]
    reps = [i for i in keep.tolist() if cell[i] not in non_cells]
    assert set(got_non) == ref_non and len(got_non) == k
    assert set(cell[reps].tolist()) == ref_sparse_cells and len(reps) == len(ref_sparse_cells)
    for i in reps:
        assert i == int(np.nonzero(cell == cell[i])[0][0])


def voxel_sample(xyz, voxel_size, retention="center"):
    xyz = np.asarray(xyz, dtype=np.float32)
    if xyz.shape[0] == 0:
        return np.zeros(0, np.int64)
    lo, hi = xyz.min(0), xyz.max(0)
    X, Y, _ = ((hi - lo) / voxel_size).astype(np.int32) + 1
    rel = xyz - lo
    v = (rel / voxel_size).astype(np.int32)
    vid = (v[:, 0] + v[:, 1] * X + v[:, 2] * X * Y).astype(np.int32)
    if retention == "first":
        return np.unique(vid, return_index=True)[1]
    dis = np.sum((rel - v * voxel_size - voxel_size / 2) ** 2, axis=-1)      # float64, as in the reference
    order = np.lexsort((np.arange(xyz.shape[0]), dis, vid))                  # per voxel: nearest the centre, then lowest position
    return order[np.unique(vid[order], return_index=True)[1]]


def center_distance(xyz, voxel_size):
    """(voxel id, float64 centre distance) per point: the fixture generator asserts no two are equal within a voxel"""
    xyz = np.asarray(xyz, dtype=np.float32)
    lo, hi = xyz.min(0), xyz.max(0)
    X, Y, _ = ((hi - lo) / voxel_size).astype(np.int32) + 1
    rel = xyz - lo
    v = (rel / voxel_size).astype(np.int32)
    return (v[:, 0] + v[:, 1] * X + v[:, 2] * X * Y).astype(np.int32), np.sum((rel - v * voxel_size - voxel_size / 2) ** 2, axis=-1)


def _t(xyz):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(xyz, dtype=np.float32)))


def distance_sample(xyz, min_dis, max_dis):
    d = torch.norm(_t(xyz), p=2, dim=1)
    return torch.nonzero((min_dis <= d) & (d <= max_dis)).flatten().numpy()


def random_drop(u, ratio):
    return torch.nonzero(_t(u) >= ratio).flatten().numpy()


def shield_terms(xyz):
    x = _t(xyz)
    return torch.atan2(x[:, 1], x[:, 0]) * 180 / torch.pi, torch.norm(x, p=2, dim=1)


def random_shield(xyz, wedges):
    """wedges (k,4) float32: start, end (reduced by 360 where it wraps), wraps, dis_threshold"""
    az, d = shield_terms(xyz)
    keep = torch.ones(az.shape[0], dtype=torch.bool)
    for s, e, wraps, thr in torch.from_numpy(np.asarray(wedges, dtype=np.float32).reshape(-1, 4)):
        inside = ((az >= s) | (az <= e)) if wraps else ((az >= s) & (az <= e))
        keep &= ~(inside & (d >= thr))
    return torch.nonzero(keep).flatten().numpy()


def shield_band(xyz, wedges):
    """points whose verdict a device atan2f / sqrtf a few ulp off the host's could flip: azimuth within 64 float32 ulp
    (at 180 degrees) of a wedge edge, or distance within 64 ulp (relative) of the wedge's threshold"""
    az, d = (t.double().numpy() for t in shield_terms(xyz))
    band = np.zeros(az.shape[0], bool)
    for s, e, _, thr in np.asarray(wedges, dtype=np.float64).reshape(-1, 4):
        band |= (np.abs(az - s) <= BAND_ULPS * F32_ULP_180) | (np.abs(az - e) <= BAND_ULPS * F32_ULP_180)
        band |= np.abs(d - thr) <= BAND_ULPS * 2.0 ** -23 * abs(thr)
    return band


def gather(sel, n, limit=-1):
    sel = np.asarray(sel, dtype=np.int64)
    if limit >= 0:
        return np.arange(n) if n <= limit else sel[:limit]
    return sel[:n]


# ---------------------------------------------------------------------------------------------- point-wise maps
def affine(xyz, R, t):
    """(R x + t, the bound 4 * 2^-24 * (sum_k |R_ik||x_k| + |t_i|) per component), the value in float64"""
    x, R, t = np.asarray(xyz, np.float64), np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3)
    return x @ R.T + t, 4 * 2.0 ** -24 * (np.abs(x) @ np.abs(R).T + np.abs(t))


def random_rt_pose(R, T, calib, R_aug, T_aug):
    """R_new = R R_aug^T, T_new = T - R_new T_aug, calib <- [R_aug|T_aug] calib, in float32 torch as the reference writes them"""
    R, T, calib, R_aug, T_aug = (torch.as_tensor(np.asarray(a), dtype=torch.float32) for a in (R, T, calib, R_aug, T_aug))
    R_new = R @ R_aug.T
    T_new = T - R_new @ T_aug.reshape(3, 1)
    se3 = torch.eye(4)
    se3[:3, :3], se3[:3, 3:] = R_aug, T_aug.reshape(3, 1)
    return R_new.numpy(), T_new.numpy(), (se3 @ calib).numpy()


def random_pos_jitter(xyz, jitter):
    return (_t(xyz) + _t(jitter)).numpy()


def coordinates_normalization(xyz, ratio):
    x = _t(xyz).clone()
    x /= ratio
    return x.numpy()


def vertical_correct_matrices(xyz, angle):
    """per point the rotation by `angle` degrees about normalize(x cross z), Rodrigues in float64, rounded to float32"""
    x = np.asarray(xyz, np.float64)
    k = np.stack([x[:, 1], -x[:, 0], np.zeros(x.shape[0])], axis=1)
    k = k / np.sqrt((k * k).sum(1, keepdims=True))
    th = math.radians(angle)
    K = np.zeros((x.shape[0], 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    return (np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)).astype(np.float32)


def vertical_correct(xyz, angle):
    """(value in float64 from the float32 matrices, bound)"""
    x = np.asarray(xyz, np.float64)
    if angle == 0:
        return x, np.zeros_like(x)
    M = vertical_correct_matrices(xyz, angle).astype(np.float64)
    return np.einsum("nij,nj->ni", M, x), 4 * 2.0 ** -24 * np.einsum("nij,nj->ni", np.abs(M), np.abs(x))


def pack(frames, padding_to):
    """frames: list of (n_i,3) arrays -> points (S,3,P) zero-filled, padding (S,P) bool; RuntimeError past padding_to"""
    P = padding_to if padding_to > 0 else max(f.shape[0] for f in frames)
    pts, pad = np.zeros((len(frames), 3, P), np.float32), np.ones((len(frames), P), bool)
    for s, f in enumerate(frames):
        if f.shape[0] > P:
            raise RuntimeError(f"The number of Point Cloud ({f.shape[0]}) is greater than `padding_to` ({P})")
        pts[s, :, :f.shape[0]], pad[s, :f.shape[0]] = np.asarray(f, np.float32).T, False
    return pts, pad


# ---------------------------------------------------------------------------------------------- a frame, replayed
class Frame:
    """xyz (float64 value of the chain so far), err (accumulated bound), idx (original indices), pose in float32"""

    def __init__(self, xyz, R=None, T=None):
        self.xyz = np.asarray(xyz, np.float32)
        self.err = np.zeros(self.xyz.shape, np.float64)
        self.idx = np.arange(self.xyz.shape[0])
        self.R = np.eye(3, dtype=np.float32) if R is None else np.asarray(R, np.float32)
        self.T = np.zeros((3, 1), np.float32) if T is None else np.asarray(T, np.float32)
        self.calib = np.eye(4, dtype=np.float32)

    def _take(self, keep):
        self.xyz, self.err, self.idx = self.xyz[keep], self.err[keep], self.idx[keep]


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def replay(frame, records):
    """the records of deeppointmap_amd.augment.DrawSource (functional name, keyword arguments) through this restatement.
    Coordinates are carried as the float32 value the restatement computes plus a bound on the distance to any other
    correctly rounded evaluation (only RandomRT / VerticalCorrect contribute; later maps scale it)."""
    for name, kw in records:
        n = frame.xyz.shape[0]
        if name == "frame":
            continue
        if name == "ground_filter":
            frame._take(ground_filter(frame.xyz, **kw)["keep"])
        elif name == "voxel_sample":
            frame._take(voxel_sample(frame.xyz, kw["voxel_size"], kw["retention"]))
        elif name == "distance_sample":
            frame._take(distance_sample(frame.xyz, kw["min_dis"], kw["max_dis"]))
        elif name == "random_drop":
            frame._take(random_drop(_np(kw["u"])[:n], kw["ratio"]))
        elif name == "random_shield":
            frame._take(random_shield(frame.xyz, kw["wedges"]))
        elif name == "random_shuffle":
            frame._take(gather(_np(kw["perm"]), n))
        elif name == "random_sample":
            frame._take(gather(_np(kw["perm"]), n, kw["num"]))
        elif name == "random_rt":
            R_aug, T_aug = _np(kw["R_aug"]), _np(kw["T_aug"])
            val, bound = affine(frame.xyz, R_aug, T_aug)
            frame.err = frame.err @ np.abs(R_aug.astype(np.float64)).T + bound
            frame.xyz = val.astype(np.float32)
            frame.R, frame.T, frame.calib = random_rt_pose(frame.R, frame.T, frame.calib, R_aug, T_aug)
        elif name == "vertical_correct":
            val, bound = vertical_correct(frame.xyz, kw["angle"])
            if kw["angle"] != 0:
                M = np.abs(vertical_correct_matrices(frame.xyz, kw["angle"]).astype(np.float64))
                frame.err = np.einsum("nij,nj->ni", M, frame.err) + bound
            frame.xyz = val.astype(np.float32)
        elif name == "random_pos_jitter":
            frame.xyz = random_pos_jitter(frame.xyz, _np(kw["jitter"])[:n])
            frame.err = frame.err + 2.0 ** -24 * np.abs(frame.xyz)
        elif name == "coordinates_normalization":
            frame.xyz = coordinates_normalization(frame.xyz, kw["ratio"])
            frame.err = frame.err / abs(kw["ratio"]) + 2.0 ** -24 * np.abs(frame.xyz)
        else:
            raise KeyError(name)
    return frame
