"""reference import path pipeline.modules.utils -> the one-launch optimisers behind the reference's factories, its schedulers,
Recorder and try_load_state_dict (no open3d, no colorlog)."""
from contextlib import nullcontext as fakecast  # noqa: F401  (the reference's no-op stand-in for autocast)

from deeppointmap_amd.optim import IdentityScheduler, Optimizer, Recorder, Scheduler, try_load_state_dict  # noqa: F401
