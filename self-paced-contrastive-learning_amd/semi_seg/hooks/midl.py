"""The MIDL baseline (``"midl"`` of semi_seg/trainers/__init__.py): ``MIDLTrainer`` (semi_seg/trainers/trainer.py:39-60)
driving ``MIDLPaperEpocher`` (semi_seg/epochers/comparable.py:195-224), as a hook.  Its regulariser is the softmax-consistency
term of ``consistency.py`` plus ``IIDSegmentationSmallPathLoss`` on the segmentation output itself (comparable.py:222):

    iic_segcriterion(softmax(unlabeled_tf_logits), softmax(unlabeled_logits_tf).detach())

This hook is the second term; ``create_midl_hook`` (creator.py) combines it with the consistency hook.  All patches are one
pass of csrc/iic_patch.hip on the LOGITS (contrastyou/losses/iic_loss.py ``from_logits``).  With the epocher's
``unlabeled_logits`` and ``flip_flags`` the flipped copy is not read: the kernels index ``unlabeled_logits`` through the flags.
Meter ``iic_mi`` (comparable.py:207,223) is added from the device scalar -- no readback per step -- and the criterion's NaN
check is the lagged one, flushed by ``close()``."""
from ...contrastyou.hooks.base import EpocherHook, TrainerHook
from ...contrastyou.meters import AverageValueMeter
from .utils import meter_focus


class MIDLPaperTrainerHook(TrainerHook):

    def __init__(self, name: str, weight: float, padding: int = 1, patch_size: int = 1024):
        super().__init__(name)
        from ...contrastyou.losses.iic_loss import IIDSegmentationSmallPathLoss
        self._weight = weight
        self._criterion = IIDSegmentationSmallPathLoss(padding=int(padding), patch_size=int(patch_size))

    def __call__(self):
        return _MIDLPaperEpocherHook(name=self._hook_name, weight=self._weight, criterion=self._criterion)


class _MIDLPaperEpocherHook(EpocherHook):
    def __init__(self, name: str, weight: float, criterion) -> None:
        super().__init__(name)
        self._weight = weight
        self._criterion = criterion

    @meter_focus
    def configure_meters(self, meters):
        self.meters.register_meter("iic_mi", AverageValueMeter())

    @meter_focus
    def __call__(self, *, unlabeled_tf_logits, unlabeled_logits_tf, seed, affine_transformer, unlabeled_logits=None,
                 flip_flags=None, **kwargs):
        if unlabeled_logits is not None and flip_flags is not None:
            loss = self._criterion.from_logits(unlabeled_tf_logits, unlabeled_logits.detach(), flags=flip_flags)
        else:
            loss = self._criterion.from_logits(unlabeled_tf_logits, unlabeled_logits_tf.detach())
        self.meters["iic_mi"].add(loss.detach())
        return self._weight * loss

    def close(self):
        self._criterion.flush_check()
