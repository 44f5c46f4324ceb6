"""The IIC-estimator baseline as a hook: the regulariser of ``IICTrainer`` (semi_seg/trainers/trainer.py:64-95, registry key
``iic``) on one UNet feature -- ``_MIMixin._mi_regularization`` (semi_seg/epochers/_mixins.py:57-101) with an ``IICEstimator``
(semi_seg/mi_estimator/discrete_mi_estimator.py:14-65) as its estimator.  Pattern, names and meter (``mi``) of
``MineTrainHook``; the learnable module is the estimator (its cluster head), which joins the trainer's flat parameter.

The estimator sees ``feature[n:]`` (the transformed images' feature) and ``feature[:n]`` through the batch's flips; the hook
returns ``weight * loss`` and records ``-loss``, the mutual-information estimate, as the reference's meters do.  With several
features the reference averages the per-feature losses by ``feature_importance`` and multiplies by one ``weight``: hook
weights ``w_i = weight * imp_i / sum(imp)`` give the same sum (``create_iic_estimator_hooks``)."""
from typing import List

from torch import nn

from ...contrastyou.hooks.base import EpocherHook, TrainerHook
from ...contrastyou.meters import AverageValueMeter
from ..arch.hook import SingleFeatureExtractor
from .discretemi import flip_flags_of
from .infonce import decoder_names, encoder_names
from .utils import meter_focus


class IICEstimatorTrainHook(TrainerHook):

    def __init__(self, *, name, model: nn.Module, feature_name: str, estimator, weight: float = 1.0) -> None:
        super().__init__(hook_name=name)
        assert feature_name in encoder_names + decoder_names, feature_name
        self._feature_name = feature_name
        self._weight = weight
        self._extractor = SingleFeatureExtractor(model, feature_name=feature_name)
        self._estimator = estimator

    @property
    def learnable_modules(self) -> List[nn.Module]:
        return [self._estimator, ]

    def __call__(self):
        return _IICEstimatorEpochHook(name=self._hook_name, weight=self._weight, extractor=self._extractor,
                                      estimator=self._estimator)


class _IICEstimatorEpochHook(EpocherHook):

    def __init__(self, *, name: str, weight: float, extractor, estimator) -> None:
        super().__init__(name)
        self._extractor = extractor
        self._extractor.bind()
        self._weight = weight
        self._estimator = estimator

    @meter_focus
    def configure_meters(self, meters):
        meters.register_meter("mi", AverageValueMeter())

    def before_forward_pass(self, **kwargs):
        self._extractor.clear()
        self._extractor.set_enable(True)

    def after_forward_pass(self, **kwargs):
        self._extractor.set_enable(False)

    @meter_focus
    def __call__(self, *, unlabeled_image, affine_transformer, seed, flip_flags=None, **kwargs):
        n_unl = len(unlabeled_image)
        feature_ = self._extractor.feature()[-n_unl * 2:]
        if flip_flags is None and not self._estimator.is_encoder:
            flip_flags = flip_flags_of(affine_transformer, seed, n_unl, feature_.device)
        loss = self._estimator.from_feature(feature_, flip_flags)
        self.meters["mi"].add(-loss.detach())  # (a device scalar: no host synchronisation)
        return loss * self._weight

    def close(self):
        try:
            self._estimator.flush_check()
        finally:
            self._extractor.remove()
