"""reference import path network.loss -> MI355X RegistrationLoss (training; see INTEGRATION.md for binding this file alone)."""
from deeppointmap_amd.loss import RegistrationLoss  # noqa: F401
