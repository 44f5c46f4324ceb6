from .mine import MineEstimator, MineEstimatorArray  # noqa: F401
from .discrete_mi_estimator import IICEstimator, IICEstimatorArray  # noqa: F401
