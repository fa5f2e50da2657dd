"""Controllers that are not networks: the batched shooting MPC."""
from .mpc import MPC  # noqa: F401
