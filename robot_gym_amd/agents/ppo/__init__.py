"""The PPO agent on the device: acting, sampling, normalisers, rollout storage and returns as HIP kernels
(include/rg_policy.h); the update in torch (PPO) or as HIP kernels (DevicePPO, include/rg_ppo.h) on the same parameter memory.
The recurrent policy (include/rg_rnn.h) acts and evaluates sequences in HIP kernels; its update is torch autograd through the
ticks (RecurrentPPO) or HIP kernels with back-propagation through time on the device (DeviceRecurrentPPO, include/rg_bptt.h)."""
from robot_gym_amd.agents.ppo.algorithm import PPO, diag_normal_kl, diag_normal_logpdf
from robot_gym_amd.agents.ppo.device_recurrent import DeviceRecurrentPPO
from robot_gym_amd.agents.ppo.device_update import DevicePPO
from robot_gym_amd.agents.ppo.policy import BatchedGaussianPolicy
from robot_gym_amd.agents.ppo.recurrent import (RecurrentGaussianPolicy, RecurrentPPO, RecurrentRolloutBuffer, collect_recurrent,
                                                play_recurrent)
from robot_gym_amd.agents.ppo.rollout import RolloutBuffer, collect, play

__all__ = ["BatchedGaussianPolicy", "RolloutBuffer", "PPO", "DevicePPO", "collect", "play", "diag_normal_kl", "diag_normal_logpdf",
           "RecurrentGaussianPolicy", "RecurrentRolloutBuffer", "RecurrentPPO", "DeviceRecurrentPPO", "collect_recurrent", "play_recurrent"]
