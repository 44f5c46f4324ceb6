"""``deepclustering2.models.ema_updater`` as ``semi_seg/hooks/mt.py:5,19,54`` uses it, restated from its published
definition (deepclustering2 is not vendored), arithmetic in HIP (``spcl_ema_update``)."""
from torch import nn

from .. import functional as F_hip


class EMAUpdater:
    """``EMAUpdater(alpha=0.999, justify_alpha=True, weight_decay=1e-5, update_bn=False)(ema_model, student_model)``:
    every parameter of ``ema_model`` becomes ``(alpha_t * ema + (1 - alpha_t) * student) * (1 - weight_decay)`` with
    ``alpha_t = min(1 - 1 / (step + 1), alpha)`` when ``justify_alpha`` (else ``alpha``); then ``step`` grows by one.
    Buffers (BatchNorm running statistics) are left alone; ``update_bn=True`` is not mirrored.

    ``step`` lives on this object and is NOT part of any ``state_dict``, as in the reference: a resumed run starts again at
    ``alpha_t = 0``, so its first update makes the teacher a copy of the student (times ``1 - weight_decay``).

    One launch per parameter tensor here; ``update_flat`` is the one-launch form for two flat buffers that hold all
    parameters in the same order (the mean-teacher hook arranges that)."""

    def __init__(self, alpha=0.999, justify_alpha=True, weight_decay=1e-5, update_bn=False):
        if update_bn:
            raise NotImplementedError("EMAUpdater mirror: update_bn=True is not mirrored")
        self.alpha = alpha
        self.justify_alpha = justify_alpha
        self.weight_decay = weight_decay
        self.update_bn = update_bn
        self.step = 0

    @property
    def alpha_t(self) -> float:
        if self.justify_alpha:
            return min(1 - 1 / (self.step + 1), self.alpha)
        return self.alpha

    def __call__(self, ema_model: nn.Module, student_model: nn.Module):
        alpha = self.alpha_t
        for e, s in zip(ema_model.parameters(), student_model.parameters()):
            F_hip.ema_update_(e.data, s.data, alpha, self.weight_decay)
        self.step += 1

    def update_flat(self, ema_flat, student_flat):
        F_hip.ema_update_(ema_flat, student_flat, self.alpha_t, self.weight_decay)
        self.step += 1


ema_updater = EMAUpdater  # the reference's name
