"""reference import path pipeline.modules.trainer -> deeppointmap_amd/trainer.py (TrainStep + EpochLoader; no codes.zip, no
tqdm, no autocast)."""
from deeppointmap_amd.trainer import Trainer  # noqa: F401
