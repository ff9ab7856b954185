"""reference import path dataloader.body -> the dataset tree of deeppointmap_amd/dataset.py (plans, `read_raw`, chunked
frame_dis; `reader(path)` gives a frame on the GPU)."""
from deeppointmap_amd.dataset import (  # noqa: F401
    READER, BasicAgent, BasicDataset, BasicScene, BinReader, NPYReader, NPZReader, PcdReader, PointCloudReader, SlamDatasets,
    get_frame_dis, get_length_range,
)
