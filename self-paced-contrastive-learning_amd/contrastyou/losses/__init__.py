from .dice import DiceKLLoss, SoftDiceLoss, WeightedKL, build_sup_criterion  # noqa: F401
