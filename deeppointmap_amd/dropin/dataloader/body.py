"""reference import path dataloader.body -> the dataset tree of deeppointmap_amd/dataset.py (plans, `read_raw`, chunked
frame_dis; `reader(path)` gives a frame on the GPU).  `SceneLoader` (deeppointmap_amd/loader.py) is exported beside
`BasicAgent`: it stands where pipeline/infer.py:98 builds its DataLoader over one."""
from deeppointmap_amd.dataset import (  # noqa: F401
    READER, BasicAgent, BasicDataset, BasicScene, BinReader, NPYReader, NPZReader, PcdReader, PointCloudReader, SlamDatasets,
    get_frame_dis, get_length_range,
)
from deeppointmap_amd.loader import SceneLoader  # noqa: F401,E402
