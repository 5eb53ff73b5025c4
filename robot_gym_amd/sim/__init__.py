"""Batched physics on the GPU: the single-rigid-body simulator (an extension; the reference simulates in PyBullet)."""
from robot_gym_amd.sim.srb import BatchedSRBSim, clone, rollout  # noqa: F401
