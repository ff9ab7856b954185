"""Scenes, poses and hand-made rule cases shared by tests/test_lidar_sim_host.py and tests/test_gpu_lidar_sim.py."""
import math
import os
from types import SimpleNamespace

import numpy as np

from deeppointmap_amd import lidar_sim as LS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def log(line):
    """what a test observed: test_logs/lidar_sim_errors.log (scripts/lidar_sim_bench.py --accuracy makes the profile of it)"""
    print(line)
    try:
        os.makedirs(os.path.join(ROOT, "test_logs"), exist_ok=True)
        with open(os.path.join(ROOT, "test_logs", "lidar_sim_errors.log"), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


def random_scene(seed, P, extent, centre=(0.0, 0.0), z0=0.0):
    """P boxes and cylinders (two to one) scattered over a square of half side `extent` about `centre`: any yaw, most
    standing on the ground, some floating, many overlapping"""
    rng = np.random.Generator(np.random.PCG64(seed))
    u = lambda a, b: a + (b - a) * float(rng.random())
    scene = LS.Scene(z0=z0)
    for p in range(P):
        x, y = centre[0] + u(-extent, extent), centre[1] + u(-extent, extent)
        lift = u(0.0, 3.0) if p % 7 == 0 else 0.0
        cls = 1 + p % 4
        if p % 3 < 2:
            h = (u(0.3, 4.0), u(0.3, 4.0), u(0.3, 5.0))
            scene.add_box((x, y, (z0 or 0.0) + lift + h[2]), h, u(-math.pi, math.pi), cls, u(0.1, 0.9))
        else:
            scene.add_cylinder((x, y, (z0 or 0.0) + lift), u(0.05, 0.7), u(1.0, 10.0), cls, u(0.1, 0.9))
    return scene


def pose(x, y, z, yaw=0.0, pitch=0.0, roll=0.0):
    cz, sz, cy, sy, cx, sx = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
    Ry = np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
    Rx = np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = Rz @ Ry @ Rx, (x, y, z)
    return M


def free_pose(scene, x, y, z, **kw):
    """pose() moved along +x until the sensor is at least 1.5 m clear of every primitive's bounding sphere footprint"""
    prims = scene.arrays()[0]
    while len(prims) and (np.hypot(prims[:, 0] - x, prims[:, 1] - y) < prims[:, 9].clip(max=6.0) + 1.5).any():
        x += 0.73
    return pose(x, y, z, **kw)


# ------------------------------------------------------------------------------------------------------------
# the kernel-against-restatement scene: ~600 primitives, three frames with different kept counts, one with none
# ------------------------------------------------------------------------------------------------------------
MODEL_385 = LS.LidarModel(np.linspace(12.0, -28.0, 5), 77, 0.9, 40.0)       # 385 rays: six blocks of 64 and one ray


def scene_600():
    scene = random_scene(11, 600, 45.0)
    poses = np.stack([free_pose(scene, 2.0, -3.0, 1.7, yaw=0.4, pitch=0.05, roll=-0.08),      # in the middle
                      free_pose(scene, 58.0, 36.0, 2.2, yaw=-2.1, pitch=-0.11, roll=0.06),    # off the edge: fewer kept
                      pose(400.0, -300.0, 1.9, yaw=1.0, pitch=0.03, roll=0.02)])              # far away: none kept
    return scene, poses


def scene_far():
    """the float64 comparison: the same kind of scene 1 km from the world's origin"""
    scene = random_scene(12, 400, 50.0, centre=(1000.0, -1000.0))
    model = LS.LidarModel(np.linspace(8.0, -22.0, 8), 192, 0.9, 60.0)
    poses = np.stack([free_pose(scene, 1003.0, -998.0, 1.8, yaw=2.3, pitch=0.07, roll=-0.05),
                      free_pose(scene, 980.0, -1021.0, 2.4, yaw=-0.6, pitch=-0.09, roll=0.1)])
    return scene, poses, model


# ------------------------------------------------------------------------------------------------------------
# hand-made rule cases: identity rotation, numbers that are exact in float32
# ------------------------------------------------------------------------------------------------------------
def _dirs(*rows):
    return np.ascontiguousarray(np.asarray(rows, np.float32).reshape(-1, 3))


def rule_cases():
    """[case]: scene, pose (4,4), dirs (n,3) float32, min_range, max_range, want_prim, want_range, want_cos per ray"""
    X, NX, DOWN = (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, -1.0)
    cases = []

    def case(name, scene, at, dirs, want, min_range=0.5, max_range=50.0):
        M = np.eye(4)
        M[:3, 3] = at
        cases.append(SimpleNamespace(name=name, scene=scene, pose=M, dirs=_dirs(*dirs), min_range=min_range, max_range=max_range,
                                     want_prim=[w[0] for w in want], want_range=[w[1] for w in want],
                                     want_cos=[w[2] for w in want]))

    s = LS.Scene(z0=None)                       # two coincident boxes: the lower index wins the tie
    s.add_box((10, 0, 0), (1, 2, 2)), s.add_box((10, 0, 0), (1, 2, 2))
    case("tie between coincident boxes", s, (0, 0, 0), [X], [(0, 9.0, 1.0)])

    s = LS.Scene(z0=0.0)                        # the sensor inside a box standing on the ground: exit face; floor ties with ground
    s.add_box((0, 0, 1), (2, 3, 1))
    case("origin inside a box", s, (0, 0, 1), [X, NX, DOWN], [(0, 2.0, 1.0), (0, 2.0, 1.0), (0, 1.0, 1.0)])

    s = LS.Scene(z0=None)                       # a near hit below min_range occludes the wall behind it
    s.add_box((10, 0, 0), (1, 5, 5)), s.add_box((0.5, 0, 0), (0.125, 0.25, 0.25))
    case("near hit occludes", s, (0, 0, 0), [X, NX], [(-1, 0.0, 0.0), (-1, 0.0, 0.0)], min_range=0.9)

    s = LS.Scene(z0=None)                       # beyond max_range: no return; just inside: a return
    s.add_box((101, 0, 0), (1, 5, 5)), s.add_box((-41, 0, 0), (1, 5, 5))
    case("beyond max_range", s, (0, 0, 0), [X, NX], [(-1, 0.0, 0.0), (1, 40.0, 1.0)], max_range=50.0)

    s = LS.Scene(z0=-10.0)                      # cylinder: top cap from above, side from the side, through the axis from inside
    s.add_cylinder((0, 0, 0), 1.0, 2.0)
    case("cylinder cap", s, (0, 0, 5), [DOWN], [(0, 3.0, 1.0)])
    case("cylinder side", s, (-5, 0, 1), [X], [(0, 4.0, 1.0)])
    case("origin inside a cylinder", s, (0, 0, 1), [X, DOWN, (0.0, 0.0, 1.0)], [(0, 1.0, 1.0), (0, 1.0, 1.0), (0, 1.0, 1.0)])

    s = LS.Scene(z0=0.0)                        # nothing within max_range but the ground
    s.add_box((500, 0, 1), (1, 1, 1)), s.add_cylinder((0, 500, 0), 0.5, 3.0)
    case("no primitive in range", s, (0, 0, 2), [X, DOWN], [(-1, 0.0, 0.0), (2, 2.0, 1.0)])

    s = LS.Scene(z0=None)                       # no ground: a ray down returns nothing
    s.add_box((4, 0, 0), (1, 1, 1))
    case("scene without ground", s, (0, 0, 0), [X, DOWN], [(0, 3.0, 1.0), (-1, 0.0, 0.0)])
    return cases
