"""reference import path dataloader.heads.npy -> deeppointmap_amd/dataset.py"""
from deeppointmap_amd.dataset import NPYReader  # noqa: F401
