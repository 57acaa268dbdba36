"""Shepherding env (reference: gym_flock/envs/shepherding/__init__.py, which is empty, so
the reference's own registry entry cannot resolve; this one exports the class)."""
from gym_flock.envs.shepherding.shepherding import ShepherdingEnv

__all__ = ["ShepherdingEnv"]
