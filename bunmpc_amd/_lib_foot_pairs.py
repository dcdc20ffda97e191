"""The former binding of include/bunmpc_foot_pairs.h, kept as a name for its callers: the header is bound by bunmpc_amd._lib like every
other."""
from ._lib import lib  # noqa: F401
