"""Spatial (graph coverage) envs (reference: gym_flock/envs/spatial/__init__.py)."""
from gym_flock.envs.spatial.coverage import CoverageEnv
from gym_flock.envs.spatial.coverage_arl import CoverageARLEnv
from gym_flock.envs.spatial.coverage_explore import ExploreEnv
from gym_flock.envs.spatial.coverage_full import CoverageFullEnv

__all__ = ["CoverageEnv", "CoverageARLEnv", "CoverageFullEnv", "ExploreEnv"]
