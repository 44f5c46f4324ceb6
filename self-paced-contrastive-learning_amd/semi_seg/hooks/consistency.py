"""Mirror of ``semi_seg/hooks/consistency.py`` (:8-35): ``weight * MSELoss(softmax(unlabeled_logits_tf).detach(),
softmax(unlabeled_tf_logits))`` in one launch (functional.consistency_softmax_mse: both softmaxes, the flip of
``unlabeled_logits`` by the batch's flags, a fixed-order mean and the gradient of ``unlabeled_tf_logits``).  Meter ``loss``."""
from torch import nn

from ... import functional as F_hip
from ...contrastyou.hooks.base import EpocherHook, TrainerHook
from ...contrastyou.meters import AverageValueMeter
from .utils import meter_focus


class ConsistencyTrainerHook(TrainerHook):

    def __init__(self, name: str, weight: float):
        super().__init__(name)
        self._weight = weight
        self._criterion = nn.MSELoss()

    def __call__(self):
        return _ConsistencyEpocherHook(name=self._hook_name, weight=self._weight, criterion=self._criterion)


class _ConsistencyEpocherHook(EpocherHook):
    def __init__(self, name: str, weight: float, criterion) -> None:
        super().__init__(name)
        self._weight = weight
        self._criterion = criterion

    @meter_focus
    def configure_meters(self, meters):
        self.meters.register_meter("loss", AverageValueMeter())

    @meter_focus
    def __call__(self, *, unlabeled_tf_logits, unlabeled_logits_tf, seed, affine_transformer, unlabeled_logits=None,
                 flip_flags=None, **kwargs):
        if unlabeled_logits is not None and flip_flags is not None:
            loss = F_hip.consistency_softmax_mse(unlabeled_logits, unlabeled_tf_logits, 1.0, flip_flags)
        else:
            loss = F_hip.consistency_softmax_mse(unlabeled_logits_tf, unlabeled_tf_logits, 1.0, None)
        self.meters["loss"].add(loss.detach())
        return self._weight * loss
