"""Mirror of ``contrastyou/losses/wrappers.py`` (:4-24): ``LossWrapperBase``, the container the per-feature criteria of
``IICLossWrapper`` / ``PICALossWrapper`` (semi_seg/utils.py) live in.  Same interface: iterating yields the criteria in
registration order, ``wrapper[feature]`` raises ``IndexError`` for an unknown feature, ``items()`` pairs names and criteria;
the criteria are registered in ``_LossModuleDict`` (so ``.to()`` and ``state_dict()`` reach them)."""
from torch import nn


class LossWrapperBase(nn.Module):

    def __init__(self):
        super().__init__()
        self._LossModuleDict = nn.ModuleDict()

    def __iter__(self):
        return iter(self._LossModuleDict.values())

    def __getitem__(self, feature_name):
        try:
            return self._LossModuleDict[feature_name]
        except KeyError:
            raise IndexError(feature_name) from None

    def items(self):
        return self._LossModuleDict.items()
