"""``deepclustering2.schedulers.customized_scheduler.RampScheduler`` as the uncertainty-aware mean teacher uses it
(semi_seg/trainers/trainer.py:278-279,289; semi_seg/epochers/comparable.py:97): a value that ramps from ``min_value`` to
``max_value`` along a Gaussian-shaped curve, read through ``.value`` and advanced by ``.step()`` once per epoch.

deepclustering2 is neither vendored in the reference nor importable here, so the formula below is NOT copied from its source:
it is fixed by this project, from the maintainers' memory of that library (the sigmoid ramp-up of the mean-teacher
literature, ``exp(-5 (1 - t)^2)``).  Whoever has the library at hand should compare.

    value(e) = min_value                                                        for e <  begin_epoch
    value(e) = max_value                                                        for e >= max_epoch
    value(e) = min_value + (max_value - min_value) * exp(ramp_mult * (1 - (e - begin_epoch) / (max_epoch - begin_epoch))^2)
                                                                                otherwise

Bracket semantics as ``PScheduler`` (semi_seg/hooks/infonce.py): the epoch counter starts at 0, the trainer hook reads
``.value`` for the epoch it is about to run and then calls ``.step()``."""
import math


class RampScheduler:

    def __init__(self, begin_epoch, max_epoch, min_value, max_value, ramp_mult=-5.0):
        self.begin_epoch, self.max_epoch = int(begin_epoch), int(max_epoch)
        self.min_value, self.max_value = float(min_value), float(max_value)
        self.mult = float(ramp_mult)
        self.epoch = 0

    def get_lr(self, cur_epoch):
        if cur_epoch < self.begin_epoch:
            return self.min_value
        if cur_epoch >= self.max_epoch:
            return self.max_value
        progress = (cur_epoch - self.begin_epoch) / (self.max_epoch - self.begin_epoch)
        return self.min_value + (self.max_value - self.min_value) * math.exp(self.mult * (1.0 - progress) ** 2)

    value = property(lambda self: self.get_lr(self.epoch))

    def step(self):
        self.epoch += 1

    def state_dict(self):
        return {"epoch": self.epoch}

    def load_state_dict(self, sd):
        self.epoch = sd["epoch"]
