"""The reference's FCOS loss with both of its mode switches, restated on the CPU: oracle/fcos_loss_modes.py under the name the
tests import (it lives in the oracle package so that oracle/launch_replay.py can differentiate the same restatement)."""
from oracle.fcos_loss_modes import *          # noqa: F401,F403
from oracle.fcos_loss_modes import INF, LOC_LOSS_TYPES, MODES, SIZES, fcos_loss, fcos_targets, iou_loss, sample_region      # noqa: F401
