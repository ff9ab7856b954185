"""reference import path dataloader.heads.bin -> deeppointmap_amd/dataset.py"""
from deeppointmap_amd.dataset import BinReader  # noqa: F401
