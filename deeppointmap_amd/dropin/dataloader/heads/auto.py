"""reference import path dataloader.heads.auto -> deeppointmap_amd/dataset.py"""
from deeppointmap_amd.dataset import PointCloudReader  # noqa: F401
