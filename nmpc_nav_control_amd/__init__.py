"""MI355X-native batched NMPC SQP-RTI solve path (drop-in for the acados solve of
JorgeDFR/nmpc_nav_control). The compute lives in libnmpc_amd.so (HIP, gfx950); this package is the
host-side mirror of the reference's controller interface plus device-memory plumbing."""
from ._lib import LIB_PATH, MODEL_IDS, MODEL_NAMES, ModelParams, default_params, lib, model_dims  # noqa: F401
from ._lib import (NODE_BREAK, NODE_ERROR, NODE_EV_ARRIVED, NODE_EV_BREAK, NODE_EV_GOAL_TOO_FAR,  # noqa: F401
                   NODE_EV_INPUT_INVALID, NODE_EV_NEXT_PART, NODE_EV_NONE, NODE_EV_OFF_PATH, NODE_EV_SOLVE_FAILED, NODE_EV_SOLVED,
                   NODE_FOLLOW_PATH, NODE_GOTO_POSE, NODE_IDLE)

__version__ = "0.1.0"
