"""Mirror of ``semi_seg/hooks/discretemi.py`` (:14-114): the UDA-IIC discrete mutual-information hook on one UNet feature.
Same names, meter (``mi``), learnable module (the cluster head) and loss.  The head's logits of the unlabelled images and
of their flipped copies come from one product (the 1x1 head commutes with the flip), and csrc/iic.hip reads the first
half through the batch's flip flags: the flipped feature map is never made.

The epocher hands the flags over as ``flip_flags`` (uint8 [n], bit 0 flips H, bit 1 flips W -- what ``TensorRandomFlip``
draws under ``FixRandomSeed(seed)``); a caller without them gets them drawn here from ``seed`` and ``affine_transformer``."""
from typing import List

import torch
from torch import nn

from ...contrastyou.hooks.base import EpocherHook, TrainerHook
from ...contrastyou.meters import AverageValueMeter
from ..arch.hook import SingleFeatureExtractor
from ..epochers.helper import FixRandomSeed
from .infonce import decoder_names, encoder_names
from .utils import meter_focus


def flip_flags_of(affine_transformer, seed, n, device):
    """the per-sample flags ``affine_transformer`` applies under ``FixRandomSeed(seed)`` (axis 1 -> bit 0, axis 2 -> bit 1)"""
    with FixRandomSeed(seed):
        dec = affine_transformer.decisions(n)
    return torch.tensor([int(d[0]) | (int(d[1]) << 1) for d in dec], dtype=torch.uint8).to(device, non_blocking=True)


class DiscreteMITrainHook(TrainerHook):

    def __init__(self, *, name, model: nn.Module, feature_name: str, weight: float = 1.0, num_clusters=20,
                 num_subheads=5, padding=None) -> None:
        super().__init__(hook_name=name)
        assert feature_name in encoder_names + decoder_names, feature_name
        self._feature_name = feature_name
        self._weight = weight
        self._extractor = SingleFeatureExtractor(model, feature_name=feature_name)
        input_dim = model.get_channel_dim(feature_name)
        self._projector = self.init_projector(input_dim=input_dim, num_clusters=num_clusters, num_subheads=num_subheads)
        self._criterion = self.init_criterion(padding=padding)

    @property
    def learnable_modules(self) -> List[nn.Module]:
        return [self._projector, ]

    def __call__(self):
        return _DiscreteMIEpochHook(name=self._hook_name, weight=self._weight, extractor=self._extractor,
                                    projector=self._projector, criterion=self._criterion)

    def init_projector(self, *, input_dim, num_clusters, num_subheads=5):
        return self.projector_class(input_dim=input_dim, num_clusters=num_clusters, num_subheads=num_subheads,
                                    head_type="linear", T=1, normalize=False)

    def init_criterion(self, padding: int = None):
        if self._feature_name in encoder_names:
            return self.criterion_class()
        return self.criterion_class(padding=padding or 0)

    @property
    def projector_class(self):
        from ...contrastyou.projectors.heads import ClusterHead, DenseClusterHead
        return ClusterHead if self._feature_name in encoder_names else DenseClusterHead

    @property
    def criterion_class(self):
        from ...contrastyou.losses.iic_loss import IIDLoss, IIDSegmentationLoss
        return IIDLoss if self._feature_name in encoder_names else IIDSegmentationLoss


class _DiscreteMIEpochHook(EpocherHook):

    def __init__(self, *, name: str, weight: float, extractor, projector, criterion) -> None:
        super().__init__(name)
        self._extractor = extractor
        self._extractor.bind()
        self._weight = weight
        self._projector = projector
        self._criterion = criterion

    @meter_focus
    def configure_meters(self, meters):
        meters.register_meter("mi", AverageValueMeter())

    def before_forward_pass(self, **kwargs):
        self._extractor.clear()
        self._extractor.set_enable(True)

    def after_forward_pass(self, **kwargs):
        self._extractor.set_enable(False)

    @meter_focus
    def __call__(self, *, unlabeled_image, unlabeled_image_tf, affine_transformer, seed, flip_flags=None, **kwargs):
        from ...contrastyou.losses.iic_loss import IIDSegmentationLoss
        from ... import functional as F_hip
        n_unl = len(unlabeled_image)
        feature_ = self._extractor.feature()[-n_unl * 2:]
        if flip_flags is None:
            flip_flags = flip_flags_of(affine_transformer, seed, n_unl, feature_.device)
        logits = self._projector.logits(feature_)  # rows of proj_feature, then of proj_tf_feature
        lx, ly = logits[:n_unl], logits[n_unl:]
        S = len(self._projector._headers)
        K = logits.shape[1] // S
        if isinstance(self._criterion, IIDSegmentationLoss):
            loss = self._criterion.from_logits(lx, ly, num_subheads=S, num_clusters=K, scale=1.0 / S, flags=flip_flags)
        else:
            loss = F_hip.iic_loss(lx, ly, num_subheads=S, num_clusters=K, padding=0, dense=False, scale=1.0 / S)
        self.meters["mi"].add(loss.detach())
        return loss * self._weight

    def close(self):
        flush = getattr(self._criterion, "flush_check", None)
        try:
            if flush is not None:
                flush()
        finally:
            self._extractor.remove()
