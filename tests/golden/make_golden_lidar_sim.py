"""tests/golden/lidar_sim_scene.npz: what street_scene and circuit of THIS project produce (there is no reference to ask),
kept so that a numpy whose generator or elementary functions drift is noticed.  `python tests/golden/make_golden_lidar_sim.py`"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SEED, BLOCKS, SPACING, LAPS = 5, (2, 1), 4.0, 2


def make():
    from deeppointmap_amd import lidar_sim
    scene = lidar_sim.street_scene(SEED, blocks=BLOCKS)
    poses = lidar_sim.circuit(scene, SPACING, LAPS)
    return dict(kind=scene.kind, params=scene.params, class_id=scene.class_id, albedo=scene.albedo, poses=poses)


if __name__ == "__main__":
    np.savez(os.path.join(HERE, "lidar_sim_scene.npz"), **make())
    print({k: v.shape for k, v in make().items()})
