"""Strong intensity view of the unlabelled pair (FixMatch, Sohn et al., NeurIPS 2020; UniMatch, Yang et al., CVPR 2023).  Not
in the reference; off unless a config carries ``StrongViewParameters``.

``SemiSupervisedEpocher.step`` forms the second view of the unlabelled batch as ``flip_batch(unlabeled_image_cf, flags)``: the
same pixels mirrored.  The reference's semi-stage recipes carry no intensity op, so a hook whose teacher is the student's own
first view (``PseudoLabelParameters`` with ``teacher: self``) asks the student to repeat itself.  With this hook registered the
epocher takes the second view from ``strong_view(image_cf, flags)`` instead: the same flip with gamma, contrast about the
sample's mean, brightness, a binomial blur and additive noise applied on the way (nnU-Net's intensity family), each behind a
gate of its own -- ``functional.strong_view``: one launch that draws the per-sample table, one that replaces ``flip_batch``'s.

Everything downstream of ``unlabeled_image_tf`` sees the strong image: the student's forward, the CPS peer's
(``_forward_pass(..., model=peer)``) and the ``unlabeled_image_tf`` keyword of the regularisation call (INTEGRATION.md lists
its readers).  The teachers read ``unlabeled_image`` / ``unlabeled_logits`` and stay weak; ``unlabeled_logits_tf`` stays
``flip_batch(unlabeled_logits, flags)``: intensity ops move no pixel.

The trainer hook owns the int32 buffer ``draw``, first value ``seed``: the seed word the table kernel reads from device
memory, advanced by one after each call, checkpointed and broadcast with ``__hooks__`` -- a resumed run draws what the
uninterrupted one would.  The hook adds no loss (``contributes_loss = False``: ``_regularization`` leaves it out of the sum).
Meter ``ops``: the mean number of applied ops per slice, read from the table on the device (no synchronisation).

``MixUpEpocher`` and ``AdversarialEpocher`` run steps of their own that form no unlabelled pair; registering the hook with
them raises in ``set_epocher``.  Two strong-view hooks under one epocher raise in ``add_hook``, and so does one
inside a ``CombineEpochHook``: a combined hook sums its members' results, and this hook has none to add."""
import torch

from ... import functional as F_hip
from ...contrastyou.hooks.base import EpocherHook, TrainerHook
from ...contrastyou.meters import AverageValueMeter
from .utils import meter_focus


class StrongViewTrainerHook(TrainerHook):

    def __init__(self, name: str = "strongview", seed: int = 0, config: F_hip.StrongViewConfig = None, **ops):
        if config is not None and ops:
            raise ValueError(f"StrongViewTrainerHook: both `config` and the op sections {sorted(ops)} are given")
        if config is not None and not isinstance(config, F_hip.StrongViewConfig):
            raise ValueError(f"StrongViewTrainerHook: `config` must be a StrongViewConfig, given {type(config).__name__}")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 31:
            raise ValueError(f"StrongViewTrainerHook: seed must be an integer in [0, 2^31), given {seed!r}")
        config = config if config is not None else F_hip.StrongViewConfig(**ops)  # (unknown keys are refused by name)
        super().__init__(name)
        self._config = config
        self.register_buffer("draw", torch.tensor([seed], dtype=torch.int32))

    @property
    def config(self) -> F_hip.StrongViewConfig:
        return self._config

    def seed_word(self, device):
        """the table kernel's seed word on ``device`` (moved once when the hook itself was not)"""
        if self.draw.device != device:
            self.draw = self.draw.to(device)
        return self.draw

    def __call__(self):
        return _StrongViewEpocherHook(name=self._hook_name, owner=self)


class _StrongViewEpocherHook(EpocherHook):
    contributes_loss = False  # SemiSupervisedEpocher._regularization calls the hook and leaves its result out of the sum

    def __init__(self, name: str, owner: StrongViewTrainerHook) -> None:
        super().__init__(name)
        self._owner = owner
        self._table = None

    def set_epocher(self, epocher):
        from ..epochers.semi import SemiSupervisedEpocher
        if not isinstance(epocher, SemiSupervisedEpocher) or type(epocher).step is not SemiSupervisedEpocher.step:
            raise RuntimeError(
                f"{type(self._owner).__name__}: {type(epocher).__name__} runs a step of its own that forms no (weak, flipped) "
                "unlabelled pair, so there is no second view to make strong -- the hook runs under SemiSupervisedEpocher's step "
                "(not under MixUpEpocher or AdversarialEpocher)")
        super().set_epocher(epocher)

    @meter_focus
    def configure_meters(self, meters):
        self.meters.register_meter("ops", AverageValueMeter())

    def graph_key(self):
        return (type(self).__name__, self._owner.config.key())  # (the seed is device state)

    def strong_view(self, image_cf, flags):
        """the strong second view of ``image_cf`` under the flips ``flags``; advances ``draw``"""
        owner = self._owner
        image = image_cf.detach().contiguous()
        draw = owner.seed_word(image.device)
        out = []
        image_tf = F_hip.strong_view(image, flags, draw, owner.config, out=out)
        draw.add_(1)
        self._table = out[0]
        return image_tf

    @meter_focus
    def __call__(self, **kwargs):
        table, self._table = self._table, None
        if table is not None:
            self.meters["ops"].add(table[:, 8].mean())
        return None
