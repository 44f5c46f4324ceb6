"""Mirror of ``semi_seg/mi_estimator/discrete_mi_estimator.py`` (:14-137): the IIC estimator of one UNet layer -- S cluster
subheads on the feature, then the mean over subheads of ``IIDLoss`` (encoder layers, :46-47) or
``IIDSegmentationSmallPathLoss(padding, patch_size)`` (decoder layers, :48-49) between the heads of two features -- and the
array of them that ``IICTrainer`` builds from ``IICRegParameters`` (semi_seg/trainers/trainer.py:64-95).

On HIP the heads produce LOGITS (one product over the stacked subheads, then ``Normalize()`` / the division by ``T`` in one
launch when configured) and the criteria apply the softmax as they read them: the encoder criterion is csrc/iic.hip's global
joint, the decoder criterion csrc/iic_patch.hip's patch-wise joint over S subheads.  No probability map is written.

``forward(feat1, feat2)`` is the reference's signature: X = heads(feat1), Y = heads(feat2).  ``from_feature(feature, flags)``
is the form the hook uses on the extracted feature [2n, C, H, W] of ``cat([image, image_tf])``: X is rows ``n..``, Y is rows
``..n`` read through the batch's flip flags -- ``mi_estimator(unlabeled_tf_features, flip(unlabeled_features))`` of
semi_seg/epochers/_mixins.py:86 with nothing flipped or concatenated (the 1x1 heads commute with the flip; the encoder heads
pool globally, which makes the flags irrelevant there).

The reference reads the layer's channel count through ``get_config``; here the caller passes ``input_dim``
(``model.get_channel_dim(layer_name)``), as ``MineEstimator`` does.  The NaN ``RuntimeError`` (:63-64) is raised one call late, or by ``flush_check``, as
``IIDSegmentationLoss`` raises its own."""
from collections.abc import Iterable
from itertools import repeat
from typing import Dict, List, Union

import torch
from torch import nn

from ... import functional as F_hip
from ... import native as _n
from ...contrastyou.losses.iic_loss import IIDLoss, IIDSegmentationSmallPathLoss, LaggedNanCheck
from ...contrastyou.projectors.heads import ClusterHead as _EncoderClusterHead, DenseClusterHead as _LocalClusterHead
from ..arch import UNet

__all__ = ["IICEstimator", "IICEstimatorArray"]

encoder_names = list(UNet.encoder_names)
decoder_names = list(UNet.decoder_names)


def _nlist(n):
    """semi_seg/utils.py:37-44: a scalar is repeated n times, a list must have n entries"""

    def parse(x):
        if isinstance(x, Iterable) and not isinstance(x, str):
            assert len(x) == n, (len(x), n)
            return x
        return list(repeat(x, n))

    return parse


def _filter_encodernames(feature_list):
    return [f for f in feature_list if f in encoder_names]


def _filter_decodernames(feature_list):
    return [f for f in feature_list if f in decoder_names]


class IICEstimator(nn.Module):
    """the estimator of one layer of the UNet"""

    def __init__(self):
        super().__init__()
        self._projector_initialized = False
        self._criterion_initialized = False
        self._nan = LaggedNanCheck()

    def init_projector(self, *, layer_name: str, input_dim: int, head_type: str = "linear", num_subhead: int = 5,
                       num_cluster: int = 10, normalize: bool = False, temperature: float = 1.0):
        assert layer_name in encoder_names + decoder_names, layer_name
        self._layer_name = layer_name
        self._input_dim = int(input_dim)
        self._head_type = head_type
        self._normalize = normalize
        self._num_subhead = int(num_subhead)
        self._num_clusters = int(num_cluster)
        self._t = temperature
        if not 2 <= self._num_clusters <= 32:
            raise ValueError(f"IICEstimator({layer_name}): num_cluster = {num_cluster} outside [2, 32] (the joint kernels)")
        head = _EncoderClusterHead if layer_name in encoder_names else _LocalClusterHead
        self._projector = head(input_dim=self._input_dim, num_clusters=self._num_clusters, num_subheads=self._num_subhead,
                               head_type=head_type, T=temperature, normalize=normalize)
        self._projector_initialized = True

    def init_criterion(self, *, padding: int, patch_size: int):
        if self._layer_name in encoder_names:
            self._criterion = IIDLoss()
        else:
            self._criterion = IIDSegmentationSmallPathLoss(padding=padding, patch_size=patch_size)
        self._criterion_initialized = True

    @property
    def is_encoder(self) -> bool:
        return self._layer_name in encoder_names

    def _check(self, feature):
        if not (self._criterion_initialized and self._projector_initialized):
            raise RuntimeError("initialize projector and criterion first")
        _n.require_gpu(feature)
        if feature.dim() != 4 or feature.shape[1] != self._input_dim or feature.shape[0] % 2:
            raise ValueError(f"IICEstimator({self._layer_name}): expected [2n, {self._input_dim}, H, W], got "
                             f"{tuple(feature.shape)}")

    def _loss(self, lx, ly, flags, out):
        S, K = self._num_subhead, self._num_clusters
        res = []
        if self.is_encoder:
            loss = F_hip.iic_loss(lx, ly, num_subheads=S, num_clusters=K, padding=0, dense=False, scale=1.0 / S, out=res)
        else:
            crit = self._criterion
            loss = F_hip.iic_patch_heads_loss(lx, ly, num_subheads=S, num_clusters=K, padding=crit.padding,
                                              patch_size=crit._patch_size[0], scale=1.0 / S, flags=flags, out=res)
        if out is not None:
            out.extend(res)
        self._nan.push(res[1], loss)
        return loss

    def from_feature(self, feature, flip_flags=None, out=None):
        """``forward(feature[n:], flip(feature[:n]))`` from the extracted feature [2n, C, H, W] itself.  ``flip_flags``: uint8
        [n] (bit 0 flips H, bit 1 flips W) or None.  ``out`` (a list) receives what the criterion's launch reports."""
        self._check(feature)
        n = feature.shape[0] // 2
        lg = self._projector.logits(feature)
        return self._loss(lg[n:], lg[:n], None if self.is_encoder else flip_flags, out)

    def forward(self, feat1, feat2):
        """discrete_mi_estimator.py:53-65 on two given [n, C, H, W] features (``feat2`` already transformed)"""
        _n.require_gpu(feat1, feat2)
        if feat1.shape != feat2.shape:
            raise ValueError(f"IICEstimator: two features of one shape, got {tuple(feat1.shape)} and {tuple(feat2.shape)}")
        return self.from_feature(torch.cat([feat2, feat1], dim=0))

    def flush_check(self):
        self._nan.flush()


class IICEstimatorArray(nn.Module):
    """``IICEstimatorArray`` (:68-137) over ``EstimatorList``: one estimator per feature name, iterated in insertion order.
    The interfaces take ``model`` for the channel counts the reference looked up through ``get_config``."""

    def __init__(self):
        super().__init__()
        self._estimator_dictionary = nn.ModuleDict()

    def add(self, *, name: str, input_dim: int = None, model=None, projector_params: Dict = None,
            criterion_params: Dict = None, **kwargs):
        assert name not in self._estimator_dictionary, self._estimator_dictionary.keys()
        if input_dim is None:
            input_dim = model.get_channel_dim(name)
        single_estimator = IICEstimator()
        single_estimator.init_projector(layer_name=name, input_dim=input_dim, **(projector_params or {}))
        single_estimator.init_criterion(**(criterion_params or {"padding": 0, "patch_size": 1000}))
        self._estimator_dictionary[name] = single_estimator

    def add_encoder_interface(self, feature_names: Union[str, List[str]], head_types: Union[str, List[str]] = "linear",
                              num_subheads: Union[int, List[int]] = 5, num_clusters: Union[int, List[int]] = 10,
                              normalize: Union[bool, List[bool]] = False, temperature: Union[float, List[float]] = 1.0, *,
                              model):
        if isinstance(feature_names, str):
            feature_names = [feature_names, ]
        feature_names = _filter_encodernames(feature_names)
        self._feature_names = feature_names
        n_pair = _nlist(len(feature_names))
        for f, h, c, s, n, t in zip(feature_names, n_pair(head_types), n_pair(num_clusters), n_pair(num_subheads),
                                    n_pair(normalize), n_pair(temperature)):
            self.add(name=f, model=model, criterion_params={"padding": 0, "patch_size": 0},
                     projector_params={"head_type": h, "num_cluster": c, "num_subhead": s, "normalize": n, "temperature": t})

    def add_decoder_interface(self, feature_names: Union[str, List[str]], head_types: Union[str, List[str]] = "linear",
                              num_subheads: Union[int, List[int]] = 5, num_clusters: Union[int, List[int]] = 10,
                              normalize: Union[bool, List[bool]] = False, temperature: Union[float, List[float]] = 1.0,
                              paddings: Union[int, List[int]] = 0, patch_sizes: Union[int, List[int]] = 1000, *, model):
        if isinstance(feature_names, str):
            feature_names = [feature_names, ]
        feature_names = _filter_decodernames(feature_names)
        self._feature_names = feature_names
        n_pair = _nlist(len(feature_names))
        for f, h, c, s, n, t, p, ps in zip(feature_names, n_pair(head_types), n_pair(num_clusters), n_pair(num_subheads),
                                           n_pair(normalize), n_pair(temperature), n_pair(paddings), n_pair(patch_sizes)):
            self.add(name=f, model=model, criterion_params={"padding": p, "patch_size": ps},
                     projector_params={"head_type": h, "num_cluster": c, "num_subhead": s, "normalize": n, "temperature": t})

    def __iter__(self):
        return iter(self._estimator_dictionary.values())

    def __len__(self):
        return len(self._estimator_dictionary)

    def __getitem__(self, name):
        return self._estimator_dictionary[name]
