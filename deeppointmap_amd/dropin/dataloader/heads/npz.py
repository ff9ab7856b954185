"""reference import path dataloader.heads.npz -> deeppointmap_amd/dataset.py"""
from deeppointmap_amd.dataset import NPZReader  # noqa: F401
