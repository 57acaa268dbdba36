"""CoverageFull-v0 — drop-in for gym_flock/envs/spatial/coverage_full.py: the whole
occupancy-map pool as one graph (no subgraph sampling, unpadded nodes), 10 robots."""
from .coverage_arl import CoverageARLEnv

DOWNSAMPLE_RATE = 10
PERIMETER_DELTA = 2.0


class CoverageFullEnv(CoverageARLEnv):

    def __init__(self, occupancy=None, device=0, reset_mode="reference"):
        super(CoverageFullEnv, self).__init__(n_robots=10, episode_length=10000, pad_nodes=False, max_nodes=1500,
                                              nearby_starts=True, num_subgraphs=1, check_connected=True,
                                              downsample_rate=DOWNSAMPLE_RATE, perimeter_delta=PERIMETER_DELTA,
                                              horizon=19, occupancy=occupancy, device=device, reset_mode=reset_mode)
