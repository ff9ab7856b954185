"""A small deterministic dataset tree for the dataset / loader / trainer tests and their fixture generators.

Closed-form coordinates on a 0.5 m lattice, no random numbers: every numpy build writes the same values.  Each frame's
`lidar_pcd[0, 0]` is its global frame id (0..47 in the order SlamDatasets numbers the frames).

  KITTI/00       40 frames round a 25 m square, 2.5 m apart; frames 0-24 are agent `0`, 25-39 agent `1`; z alternates
                 0 / 0.5.  Frame 0 is within range of frames 37-39 (a loop).
  KITTI/01       3 frames 4 m apart: fewer than K candidates, `_map_query` replicates them.
  Carla_Town/00  5 frames, the last 2 km away: it has no candidate and pairs with itself.  The name makes
                 `refined_SE3_file == ''`.

Config: registration = {K: 6, K_max: 12, fill: True, distance: 10.0}, loop_detection = {distance: 6.0}.
"""
import os

import numpy as np

N_FRAMES = 48


def _square(k):
    """frame k of 40 round a 25 m square at 2.5 m spacing"""
    side, step = divmod(k, 10)
    d = 2.5 * step
    return [(d, 0.0), (25.0, d), (25.0 - d, 25.0), (0.0, 25.0 - d)][side]


def poses():
    """[(dataset, scene, agent, file number, (x, y, z))] in global frame order"""
    out = []
    for k in range(40):
        x, y = _square(k)
        out.append(("KITTI", "00", "0" if k < 25 else "1", k, (x, y, 0.5 * (k % 2))))
    for k in range(3):
        out.append(("KITTI", "01", "0", k, (4.0 * k, 100.0, 0.0)))
    for k in range(5):
        out.append(("Carla_Town", "00", "0", k, (2000.0 if k == 4 else 3.0 * k, -50.0, 0.0)))
    return out


def scan(gid, points):
    """(points,3) float32 on a 0.5 m lattice, different for every frame; [0,0] = the global frame id"""
    k = np.arange(points, dtype=np.int64)
    xyz = np.stack([0.5 * ((k * 7 + gid) % 41 - 20), 0.5 * ((k * 13 + 3 * gid) % 37 - 18), 0.5 * ((k * 3 + gid) % 5)], axis=1)
    xyz = xyz.astype(np.float32)
    xyz[0, 0] = gid
    return xyz


def rotation(gid):
    """a quarter turn about z, gid % 4 times: exact in float32"""
    c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][gid % 4]
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float32)


def write_tree(root, points=64):
    """write the tree under `root` (npz files); returns the list of file paths in global frame order"""
    files = []
    for gid, (ds, scene, agent, num, xyz) in enumerate(poses()):
        d = os.path.join(root, ds, scene, agent)
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, f"{num}.npz")
        np.savez(path, lidar_pcd=scan(gid, points), ego_rotation=rotation(gid),
                 ego_translation=np.array(xyz, dtype=np.float32).reshape(3, 1))
        files.append(path)
    return files


def write_refined_tables(root):
    """refined_SE3.pkl of the two KITTI scenes: {(a, b): pose of frame b in frame a} for consecutive frames, from the tree's
    own poses (exact: quarter turns and multiples of 0.5 m); every other pair falls back to the global poses"""
    import pickle
    all_poses = poses()
    for scene, first, n in (("00", 0, 40), ("01", 40, 3)):
        table = {}
        for a in range(n - 1):
            Pa, Pb = np.eye(4), np.eye(4)
            Pa[:3, :3], Pa[:3, 3] = rotation(first + a), all_poses[first + a][4]
            Pb[:3, :3], Pb[:3, 3] = rotation(first + a + 1), all_poses[first + a + 1][4]
            table[(a, a + 1)] = np.linalg.inv(Pa) @ Pb
        with open(os.path.join(root, "KITTI", scene, "refined_SE3.pkl"), "wb") as f:
            pickle.dump(table, f)


def tree_config(root):
    """the plain dict of the config (wrap it in the attribute dict of whichever side reads it)"""
    reader = {"type": "npz"}
    return {
        "dataset": [
            {"name": "KITTI", "root": os.path.join(root, "KITTI"), "scenes": ["00", "01"], "reader": dict(reader)},
            {"name": "Carla_Town", "root": os.path.join(root, "Carla_Town"), "scenes": ["00"], "reader": dict(reader)},
        ],
        "train": {
            "registration": {"K": 6, "K_max": 12, "fill": True, "distance": 10.0, "map_size_max": 4},
            "loop_detection": {"distance": 6.0},
        },
    }


def write_reader_files(root, points=12):
    """one .npz, one .npy and one .bin file for the reader checks.  The .bin file has NaNs in columns 0, 1, 2 and 3 of
    different rows (rows 1, 4, 7 and 9): the first three go, the row with the NaN intensity stays."""
    os.makedirs(root, exist_ok=True)
    out = {}
    out["npz"] = os.path.join(root, "5.npz")
    np.savez(out["npz"], lidar_pcd=scan(5, points), ego_rotation=rotation(5).astype(np.float64),
             ego_translation=np.array([[1.5], [-2.0], [0.5]], dtype=np.float32))
    out["npy"] = os.path.join(root, "6.npy")
    np.save(out["npy"], scan(6, points))
    rec = np.concatenate([scan(7, points), (np.arange(points, dtype=np.float32) / 16).reshape(-1, 1)], axis=1)
    for row, col in ((1, 0), (4, 1), (7, 2), (9, 3)):
        rec[row, col] = np.nan
    out["bin"] = os.path.join(root, "7.bin")
    rec.astype(np.float32).tofile(out["bin"])
    return out
