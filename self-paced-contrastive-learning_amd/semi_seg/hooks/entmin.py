"""Mirror of ``semi_seg/hooks/entmin.py`` (:8-34): ``weight * Entropy()(softmax(unlabeled_logits_tf))`` in one launch
(functional.entropy_softmax: the softmax, the fixed-order mean and the gradient of the logits).  Meter ``loss``."""
from ... import functional as F_hip
from ...contrastyou.hooks.base import EpocherHook, TrainerHook
from ...contrastyou.losses.kl import Entropy
from ...contrastyou.meters import AverageValueMeter
from .utils import meter_focus


class EntropyMinTrainerHook(TrainerHook):

    def __init__(self, name: str, weight: float):
        super().__init__(name)
        self._weight = weight
        self._criterion = Entropy()

    def __call__(self):
        return _EntropyEpocherHook(name=self._hook_name, weight=self._weight, criterion=self._criterion)


class _EntropyEpocherHook(EpocherHook):
    def __init__(self, name: str, weight: float, criterion) -> None:
        super().__init__(name)
        self._weight = weight
        self._criterion = criterion

    @meter_focus
    def configure_meters(self, meters):
        self.meters.register_meter("loss", AverageValueMeter())

    @meter_focus
    def __call__(self, *, unlabeled_tf_logits, unlabeled_logits_tf, seed, affine_transformer, **kwargs):
        loss = F_hip.entropy_softmax(unlabeled_logits_tf, self._criterion._eps, 1.0)
        self.meters["loss"].add(loss.detach())
        return self._weight * loss
