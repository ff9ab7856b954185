"""reference import path dataloader.transforms -> the GPU transforms (the frame lives on the GPU, `ToGPU` /
`ToCPU` do nothing, GroundFilter's order is the documented stable one)."""
from deeppointmap_amd.augment import (  # noqa: F401
    Compose, CoordinatesNormalization, DistanceSample, FarthestPointSample, GroundFilter, LowPassFilter, OutlierFilter,
    PointCloud, PointCloudTransforms, RandomChoice, RandomDrop, RandomOcclusion, RandomPosJitter, RandomRT, RandomSample,
    RandomShuffle, ToCPU, ToGPU, ToTensor, VerticalCorrect, VoxelSample, collate_frames, get_transforms, pointcloud_transforms,
)
