"""Batched physics on the GPU: the single-rigid-body simulator (an extension; the reference simulates in PyBullet) and the
ground it stands on."""
from robot_gym_amd.sim.motor_model import MotorModel  # noqa: F401
from robot_gym_amd.sim.randomizer import DomainRandomizer  # noqa: F401
from robot_gym_amd.sim.sensor_model import SensorModel  # noqa: F401
from robot_gym_amd.sim.srb import BatchedSRBSim, clone, rollout  # noqa: F401
from robot_gym_amd.sim.state_estimator import StateEstimator  # noqa: F401
from robot_gym_amd.sim.terrain import GridTerrain, RandomTerrain  # noqa: F401
