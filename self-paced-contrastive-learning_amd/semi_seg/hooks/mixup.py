"""Mirror of ``semi_seg/hooks/mixup.py`` (:19-94), the mix-up baseline: under the step's seed draw ``lam ~ Beta(1, 1)`` and a
permutation of the 2B samples of ``cat([labeled_image, labeled_image_tf])``, blend images and one-hot targets with their
permuted selves, run the model on the mixed images and take ``weight * KL_div(softmax(prediction), mixed target)``.

Two launches around the model's pass (functional.mixup_images, functional.mixup_kl_onehot): neither the concatenations nor
the one-hot maps nor the mixed target are ever built, the permutation reaches the device as one pinned int32 copy, and the
meter ``mixup_ls`` takes the device scalar -- no host synchronisation per call (the reference's ``KL_div`` asserts and
``.item()`` are three)."""
from contextlib import nullcontext

import torch

from ... import functional as F_hip
from ...contrastyou.hooks.base import EpocherHook, TrainerHook
from ...contrastyou.losses.kl import KL_div
from ...contrastyou.meters import AverageValueMeter
from ..epochers.helper import FixAllSeed
from .utils import meter_focus


def mixup_draw(seed, batch_size: int, alpha: float = 1.0):
    """the draws of ``mixup_data`` (mixup.py:21-28) under ``fix_all_seed_within_context(seed)`` (:69), in its order: ``lam``
    from numpy's generator, then ``torch.randperm(batch_size)`` from torch's CPU generator; the generators' states are restored"""
    import numpy as np
    with FixAllSeed(seed):
        lam = np.random.beta(alpha, alpha) if alpha > 0 else 1
        index = torch.randperm(batch_size)
    return lam, index


class MixUpHook(TrainerHook):
    def __init__(self, *, hook_name: str, weight: float, enable_bn=True):
        super().__init__(hook_name)
        self._weight = weight
        self._enable_bn = enable_bn

    def __call__(self, **kwargs):
        return _MixUpEpocherHook(name="mix_reg", weight=self._weight, criterion=KL_div(), enable_bn=self._enable_bn)


class _MixUpEpocherHook(EpocherHook):
    def __init__(self, *, name: str, weight: float, alpha: float = 1.0, criterion, enable_bn=True) -> None:
        super().__init__(name)
        self._weight = weight
        self._alpha = alpha
        self._criterion = criterion
        self._enable_bn = enable_bn

    @meter_focus
    def configure_meters(self, meters):
        self.meters.register_meter("mixup_ls", AverageValueMeter())

    @meter_focus
    def __call__(self, *, labeled_image, labeled_image_tf, labeled_target, labeled_target_tf, seed, **kwargs):
        lam, index = mixup_draw(seed, 2 * len(labeled_image), self._alpha)
        plan = F_hip.MixupPlan(index, lam, labeled_image.device)
        mixed_image = F_hip.mixup_images(labeled_image, labeled_image_tf, plan)
        model = self.epocher._model
        with (nullcontext() if self._enable_bn else model.set_bn_track(False)):
            mixed_pred = model(mixed_image)
        loss = F_hip.mixup_kl_onehot(mixed_pred, labeled_target, labeled_target_tf, plan, self._criterion._eps, 1.0)
        self.meters["mixup_ls"].add(loss.detach())
        return self._weight * loss
