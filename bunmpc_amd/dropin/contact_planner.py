"""PYTHONPATH shim: `from contact_planner import ContactPlanner` resolves to bunmpc_amd.contact_planner."""
from bunmpc_amd.contact_planner import *  # noqa: F401,F403
