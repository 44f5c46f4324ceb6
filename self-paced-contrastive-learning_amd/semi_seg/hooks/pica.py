"""The PICA baseline as a hook: the partition-uncertainty-index criteria of ``contrastyou/losses/pica_loss.py`` (``PUILoss`` on
an encoder feature, ``PUISegLoss`` on a decoder feature -- what ``PICALossWrapper``, semi_seg/utils.py:242-263, pairs with the
cluster heads) on one UNet feature.  ``DiscreteMITrainHook`` with its ``criterion_class`` overridden (the override point of
semi_seg/hooks/discretemi.py:58-66); extractor, cluster head and flip flags are that hook's.

Meters: ``pui`` is the returned criterion (mean over the subheads, before the hook's weight), ``pui_ce`` its cross-entropy
part.  On a decoder feature the two differ by the constant ``lamda * (log M - (M / K) log K)`` (M = N H W; see
contrastyou/losses/pica_loss.py): ``pui`` is a large negative number there and ``pui_ce`` is the one to read."""
from ...contrastyou.meters import AverageValueMeter
from .discretemi import DiscreteMITrainHook, _DiscreteMIEpochHook, flip_flags_of
from .infonce import encoder_names
from .utils import meter_focus


class PICATrainHook(DiscreteMITrainHook):

    def __init__(self, *, name, model, feature_name: str, weight: float = 1.0, num_clusters=20, num_subheads=5, padding=None,
                 lamda: float = 2.0) -> None:
        self._lamda = lamda  # (init_criterion runs inside the base constructor)
        super().__init__(name=name, model=model, feature_name=feature_name, weight=weight, num_clusters=num_clusters,
                         num_subheads=num_subheads, padding=padding)

    def __call__(self):
        return _PICAEpochHook(name=self._hook_name, weight=self._weight, extractor=self._extractor,
                              projector=self._projector, criterion=self._criterion)

    def init_criterion(self, padding: int = None):
        if self._feature_name in encoder_names:
            return self.criterion_class(lamda=self._lamda)
        return self.criterion_class(lamda=self._lamda, padding=padding or 0)

    @property
    def criterion_class(self):
        from ...contrastyou.losses.pica_loss import PUILoss, PUISegLoss
        return PUILoss if self._feature_name in encoder_names else PUISegLoss


class _PICAEpochHook(_DiscreteMIEpochHook):

    @meter_focus
    def configure_meters(self, meters):
        meters.register_meter("pui", AverageValueMeter())
        meters.register_meter("pui_ce", AverageValueMeter())

    @meter_focus
    def __call__(self, *, unlabeled_image, unlabeled_image_tf, affine_transformer, seed, flip_flags=None, **kwargs):
        n_unl = len(unlabeled_image)
        feature_ = self._extractor.feature()[-n_unl * 2:]
        if flip_flags is None:
            flip_flags = flip_flags_of(affine_transformer, seed, n_unl, feature_.device)
        logits = self._projector.logits(feature_)  # rows of proj_feature, then of proj_tf_feature
        lx, ly = logits[:n_unl], logits[n_unl:]
        S = len(self._projector._headers)
        K = logits.shape[1] // S
        loss = self._criterion.from_logits(lx, ly, num_subheads=S, num_clusters=K, scale=1.0 / S, flags=flip_flags)
        self.meters["pui"].add(loss.detach())
        self.meters["pui_ce"].add(self._criterion.last_ce)
        return loss * self._weight
