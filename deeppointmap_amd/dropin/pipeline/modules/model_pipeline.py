"""reference import path pipeline.modules.model_pipeline -> the MI355X training step ("Training: the whole step")."""
from deeppointmap_amd.train_pipeline import DeepPointModelPipeline, TrainStep  # noqa: F401
