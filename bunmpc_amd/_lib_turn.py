"""The former binding of include/bunmpc_turn.h, kept as a name for its callers: the header is bound by bunmpc_amd._lib like every other,
and turn_struct lives in bunmpc_amd.plan_batch."""
from ._lib import Turn, lib  # noqa: F401
from .plan_batch import turn_struct  # noqa: F401
