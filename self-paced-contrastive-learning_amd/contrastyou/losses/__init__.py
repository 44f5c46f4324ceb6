from .dice import DiceKLLoss, SoftDiceLoss, WeightedKL, build_sup_criterion  # noqa: F401
from .boundary import BoundaryLoss  # noqa: F401
