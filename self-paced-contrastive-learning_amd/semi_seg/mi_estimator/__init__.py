from .mine import MineEstimator, MineEstimatorArray  # noqa: F401
