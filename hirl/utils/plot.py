"""hirl/utils/plot.py of the reference -> hirl4ucav_amd.utils.plot (plot_3d_trajectories, plot_distance, plot_2d_trajectories)."""
from hirl4ucav_amd.utils.plot import *  # noqa: F401,F403
from hirl4ucav_amd.utils.plot import plot_2d_trajectories, plot_3d_trajectories, plot_distance  # noqa: F401
