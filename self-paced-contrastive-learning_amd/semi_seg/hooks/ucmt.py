"""The uncertainty-aware mean teacher (``"ucmeanteacher"`` of semi_seg/trainers/__init__.py): ``UCMeanTeacherTrainer``
(semi_seg/trainers/trainer.py:274-290) driving ``UCMeanTeacherEpocher`` (semi_seg/epochers/comparable.py:54-105), as a hook
on top of the mean-teacher hook of ``mt.py`` -- the teacher copy, its flat buffer and the one-launch moving average are
reused as they are.

Each call runs the teacher once on the unlabelled images and ``num_samples`` (8) more times on noisy copies of them with
its BatchNorm statistics tracking switched off, all without autograd, and hands the ``num_samples + 2`` class maps to ONE
launch (functional.ucmt_softmax_mse): the consistency term ``mse(softmax(student), softmax(flip(teacher)))`` -- here the
teacher IS soft-maxed (comparable.py:86), unlike mt.py -- is kept only at the pixels where the normalised entropy of the
soft-maxed average of the noisy predictions does not exceed the epoch's threshold.  Then the teacher moves towards the
student, before the optimizer step, as in ``mt.py``.  Meters ``loss``, ``uc_weight`` (the threshold) and ``uc_ratio`` (the
kept share of the pixels, accumulated on the device: no synchronisation per step).

The noise is ``noise_std * torch.randn_like(image)`` from torch's ambient device generator, as in the reference.  With
``cumulative_noise=True`` (the default: parity) the k-th noisy pass sees the image plus the SUM of the first k noises: that
is what comparable.py:76's in-place ``uimage += noise`` computes.  ``cumulative_noise=False`` gives every pass the image
plus its own noise.  The one deliberate difference from the reference: the noise is added to a private copy, the caller's
``unlabeled_image`` is never modified (the reference leaves it with all eight noises added) -- the other hooks of a
``CombineTrainerHook`` read it after this one.

The threshold is any object with ``.value`` and ``.step()``; by default the reference's ``RampScheduler(0, max_epoch // 3 *
2, min_value=0.75, max_value=1)``.  It is read and then stepped once per epoch, in the trainer hook's ``__call__``
(trainer.py:286-289); like ``PScheduler``'s, its epoch counter is not checkpointed."""
from contextlib import contextmanager

import torch
from torch import nn

from ... import functional as F_hip
from ...contrastyou.meters import AverageValueMeter
from ...contrastyou.schedulers import RampScheduler
from ..epochers.helper import FixRandomSeed
from .mt import MeanTeacherTrainerHook, _MeanTeacherEpocherHook
from .utils import meter_focus


@contextmanager
def bn_track_off(model: nn.Module):
    """``_disable_tracking_bn_stats`` (comparable.py:89): the model's ``set_bn_track(False)`` where it has one, otherwise
    ``track_running_stats = False`` on every module that carries the flag; restored on the way out"""
    if hasattr(model, "set_bn_track"):
        with model.set_bn_track(False):
            yield model
        return
    held = [(m, m.track_running_stats) for m in model.modules() if hasattr(m, "track_running_stats")]
    try:
        for m, _ in held:
            m.track_running_stats = False
        yield model
    finally:
        for m, flag in held:
            m.track_running_stats = flag


class UCMeanTeacherTrainerHook(MeanTeacherTrainerHook):

    def __init__(self, name: str, weight: float, model: nn.Module, max_epoch: int, alpha: float = 0.999,
                 weight_decay: float = 1e-5, num_samples: int = 8, noise_std: float = 0.05, threshold=None,
                 cumulative_noise: bool = True):
        super().__init__(name, weight, model, alpha=alpha, weight_decay=weight_decay, teacher_softmax=True)
        if not 1 <= int(num_samples) <= F_hip.UCMT_MAX_NOISY:
            raise ValueError(f"UCMeanTeacherTrainerHook: num_samples = {num_samples} (1 .. {F_hip.UCMT_MAX_NOISY})")
        if threshold is None:
            threshold = RampScheduler(begin_epoch=0, max_epoch=int(max_epoch) // 3 * 2, min_value=0.75, max_value=1)
        if not (hasattr(threshold, "value") and callable(getattr(threshold, "step", None))):
            raise TypeError(f"UCMeanTeacherTrainerHook: `threshold` needs .value and .step(), got {type(threshold).__name__}")
        self._threshold = threshold
        self._num_samples, self._noise_std = int(num_samples), float(noise_std)
        self._cumulative_noise = bool(cumulative_noise)

    def __call__(self):
        value = float(self._threshold.value)  # this epoch's threshold, then advance the schedule (trainer.py:286-289)
        self._threshold.step()
        return _UCMeanTeacherEpocherHook(name=self._hook_name, weight=self._weight, criterion=self._criterion,
                                         teacher_model=self._teacher_model, updater=self._updater, owner=self,
                                         threshold=value, num_samples=self._num_samples, noise_std=self._noise_std,
                                         cumulative_noise=self._cumulative_noise)


class _UCMeanTeacherEpocherHook(_MeanTeacherEpocherHook):
    def __init__(self, *, threshold: float, num_samples: int, noise_std: float, cumulative_noise: bool, **kwargs) -> None:
        super().__init__(**kwargs)
        self._threshold = threshold
        self._num_samples, self._noise_std, self._cumulative_noise = num_samples, noise_std, cumulative_noise

    @meter_focus
    def configure_meters(self, meters):
        self.meters.register_meter("loss", AverageValueMeter())
        self.meters.register_meter("uc_weight", AverageValueMeter())
        self.meters.register_meter("uc_ratio", AverageValueMeter())

    def _teacher_maps(self, unlabeled_image):
        """the clean prediction and the ``num_samples`` noisy ones (comparable.py:85,89-92), none of them flipped"""
        teacher = self._teacher_model
        with torch.no_grad():
            clean = teacher(unlabeled_image)
            noisy = []
            image = unlabeled_image.clone() if self._cumulative_noise else None
            with bn_track_off(teacher):
                for _ in range(self._num_samples):
                    noise = self._noise_std * torch.randn_like(unlabeled_image)
                    if self._cumulative_noise:
                        image += noise
                        noisy.append(teacher(image))
                    else:
                        noisy.append(teacher(unlabeled_image + noise))
        return clean, noisy

    @meter_focus
    def __call__(self, *, unlabeled_tf_logits, unlabeled_image, seed, affine_transformer, flip_flags=None, **kwargs):
        student = self.epocher._model
        self._match_compute_dtype(student)
        clean, noisy = self._teacher_maps(unlabeled_image)
        if flip_flags is None:
            with FixRandomSeed(seed):
                dec = affine_transformer.decisions(len(unlabeled_image))
            flip_flags = torch.tensor([int(d[0]) | (int(d[1]) << 1) for d in dec], dtype=torch.uint8,
                                      device=unlabeled_tf_logits.device)
        out = []
        loss = F_hip.ucmt_softmax_mse(clean, noisy, unlabeled_tf_logits, self._threshold, 1.0, flip_flags, out=out)
        kept, mask = out
        self.meters["loss"].add(loss.detach())
        self.meters["uc_weight"].add(self._threshold)
        self.meters["uc_ratio"].add(kept.to(torch.float32) / float(mask.numel()))
        if self._owner is not None:
            self._owner.ema_step(student)
        else:
            self._updater(ema_model=self._teacher_model, student_model=student)
        return self._weight * loss
