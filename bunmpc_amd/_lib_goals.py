"""The former binding of include/bunmpc_goals.h, kept as a name for its callers: the header is bound by bunmpc_amd._lib like every other,
and what this module added to the binding lives in bunmpc_amd.cc_goal_batch."""
from ._lib import CcGait, CcGoalBatch, CcGoalWbBatch, lib  # noqa: F401
from .cc_goal_batch import gait_struct, plan_knots  # noqa: F401
