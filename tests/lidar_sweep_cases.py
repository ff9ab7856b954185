"""Motions and scenes shared by tests/test_lidar_sweep_host.py, tests/test_gpu_lidar_sweep.py and tests/test_gpu_deskew.py."""
import os

import numpy as np

import lidar_sim_cases as C
from deeppointmap_amd import lidar_sim as LS

ROOT = C.ROOT


def log(line, name="lidar_sweep_errors.log"):
    """what a test observed: test_logs/<name> (profiles/deskew_accuracy.md is a copy of the deskew lines)"""
    print(line)
    try:
        os.makedirs(os.path.join(ROOT, "test_logs"), exist_ok=True)
        with open(os.path.join(ROOT, "test_logs", name), "a") as f:
            f.write(line + "\n")
    except OSError:
        pass


# the sensor's pose at the end of a sweep in its frame at the start
CORNER = C.pose(1.5, 0.12, -0.03, yaw=0.25, pitch=0.01, roll=-0.02)        # 1.5 m and 0.25 rad: a corner of the circuit
TINY = C.pose(1e-7, 0.0, 0.0, yaw=1e-9)                                    # an angle of 1e-9: no 0 / 0
ZERO = np.eye(4)
MOTIONS = {"corner": CORNER, "tiny": TINY, "zero": ZERO}


def far_sweep():
    """lidar_sim_cases.scene_far with sweep motion: scene, P0, P1 (2,4,4), model; both frames move like a corner"""
    scene, poses, model = C.scene_far()
    return scene, poses, np.stack([poses[0] @ CORNER, poses[1] @ np.linalg.inv(CORNER)]), model


def street_sweep(frames=(7,)):
    """street_scene(2), circuit(spacing=1.5), SMALL16: the sensor turns once between consecutive poses"""
    scene = LS.street_scene(2)
    P0, P1 = LS.sweep_poses(LS.circuit(scene, spacing=1.5))
    sel = list(frames)
    return scene, P0[sel], P1[sel], LS.SMALL16
