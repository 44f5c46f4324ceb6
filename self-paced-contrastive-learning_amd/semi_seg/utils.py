"""Mirror of the criterion wrappers of ``semi_seg/utils.py``: ``_filter_encodernames`` / ``_filter_decodernames`` (:27-34),
``_nlist`` (:37-44), ``IIDLoss`` (:210-213, the criterion that returns the loss alone), ``IICLossWrapper`` (:217-239) and
``PICALossWrapper`` (:242-263).  The criteria they hold are the HIP-backed ones of ``contrastyou.losses``.  The projector
wrappers of that file are not mirrored: the hooks build their heads themselves (semi_seg/hooks/discretemi.py)."""
from collections.abc import Iterable
from typing import List, Union

from torch import Tensor

from ..contrastyou.losses.iic_loss import IIDLoss as _IIDLoss, IIDSegmentationSmallPathLoss
from ..contrastyou.losses.pica_loss import PUILoss, PUISegLoss
from ..contrastyou.losses.wrappers import LossWrapperBase
from .hooks.infonce import decoder_names, encoder_names


def _filter_encodernames(feature_list):
    return [f for f in feature_list if f in encoder_names]


def _filter_decodernames(feature_list):
    return [f for f in feature_list if f in decoder_names]


def _nlist(n):
    """a scalar (or a string) repeated n times; a sequence must already have n entries"""

    def parse(x):
        if isinstance(x, Iterable) and not isinstance(x, str):
            assert len(x) == n, (len(x), n)
            return x
        return [x] * n

    return parse


class IIDLoss(_IIDLoss):

    def forward(self, x_out: Tensor, x_tf_out: Tensor):
        return super().forward(x_out, x_tf_out)[0]


class _EncoderDecoderLossWrapper(LossWrapperBase):
    """one criterion per feature: ``encoder_criterion()`` for an encoder feature, ``decoder_criterion(*params)`` for a decoder
    feature, with one list of ``params`` per decoder feature (scalars are repeated); encoder features come first"""

    def __init__(self, feature_names: Union[str, List[str]], encoder_criterion, decoder_criterion, *decoder_params) -> None:
        super().__init__()
        if isinstance(feature_names, str):
            feature_names = [feature_names]
        self._encoder_features = _filter_encodernames(feature_names)
        self._decoder_features = _filter_decodernames(feature_names)
        assert len(feature_names) == len(self._encoder_features) + len(self._decoder_features)
        for f in self._encoder_features:
            self._LossModuleDict[f] = encoder_criterion()
        per_feature = [_nlist(len(self._decoder_features))(p) for p in decoder_params]
        for f, *params in zip(self._decoder_features, *per_feature):
            self._LossModuleDict[f] = decoder_criterion(*params)

    @property
    def feature_names(self):
        return self._encoder_features + self._decoder_features


class IICLossWrapper(_EncoderDecoderLossWrapper):
    """``IIDLoss`` on encoder features, ``IIDSegmentationSmallPathLoss(padding, patch_size)`` on decoder features"""

    def __init__(self, feature_names: Union[str, List[str]], paddings: Union[int, List[int]],
                 patch_sizes: Union[int, List[int]]) -> None:
        super().__init__(feature_names, IIDLoss, lambda p, size: IIDSegmentationSmallPathLoss(padding=p, patch_size=size),
                         paddings, patch_sizes)


class PICALossWrapper(_EncoderDecoderLossWrapper):
    """``PUILoss`` on encoder features, ``PUISegLoss(padding)`` on decoder features"""

    def __init__(self, feature_names: Union[str, List[str]], paddings: Union[int, List[int]]) -> None:
        super().__init__(feature_names, PUILoss, lambda p: PUISegLoss(padding=p), paddings)
