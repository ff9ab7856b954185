"""reference import path dataloader.heads.pcd -> deeppointmap_amd/dataset.py"""
from deeppointmap_amd.dataset import PcdReader  # noqa: F401
