"""The DDPG agent on the device (include/rg_ddpg.h): acting with Ornstein-Uhlenbeck noise, the replay ring, sampling, the critic's
and the actor's gradients, clipped Adam and the soft target update as HIP kernels; the collector and the deterministic player."""
from robot_gym_amd.agents.ddpg.agent import BatchedDDPGAgent
from robot_gym_amd.agents.ddpg.rollout import collect, play

__all__ = ["BatchedDDPGAgent", "collect", "play"]
