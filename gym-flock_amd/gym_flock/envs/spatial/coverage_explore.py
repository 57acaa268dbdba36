"""ExploreEnv-v0 / -v1 on the MI355X engine — drop-in for gym_flock/envs/spatial/coverage_explore.py.

CoverageARLEnv with hidden nodes: the observation shows only what the robots have seen so
far. Each observation first adds to `discovered_nodes` every node within 4 * DELTA = 22 of
a robot (not the node a robot stands on: its distance is 0), then masks the node features
of undiscovered nodes, flags discovered nodes next to an undiscovered one in a fourth
feature, and hides the senders of edges with an undiscovered end (coverage.py:334-346). The
greedy expert only heads for discovered targets (:819-820). All of it runs on the device
after the step (cov_set_hidden). The constructor keeps the reference's signature; reset()'s
draws move to the device with gym_flock.make(..., reset_mode="device") or
set_reset_mode("device") (CoverageEnv).
"""
from .coverage_arl import CoverageARLEnv


class ExploreEnv(CoverageARLEnv):

    def __init__(self, occupancy=None, device=0):
        super(ExploreEnv, self).__init__(hide_nodes=True, n_node_feat=4, horizon=19, episode_length=50,
                                         occupancy=occupancy, device=device)
