"""Mirror of ``semi_seg/mi_estimator/mineestimator.py`` (:9-50): the MINE statistics network on one UNet feature,
``Conv2d(2C, C, 3, 1, 1) -> BatchNorm2d -> ReLU -> Conv2d(C, C/2, 3, 1, 1) -> BatchNorm2d -> ReLU -> AdaptiveMaxPool2d((1, 1))
-> Flatten -> Linear(C/2, 1)``, and ``Em - Ej`` over the joint and the batch-rolled pairs.

``_projector`` is the reference's ``nn.Sequential`` of stock torch modules, kept as the CONTAINER of parameters and buffers:
``state_dict()`` has the reference's keys and shapes by construction, the construction order is the reference's (one seed
draws the same initial weights), ``train()`` / ``eval()`` / ``to()`` reach the BatchNorms.  None of those modules is ever
called: ``forward`` runs on HIP (functional.mine_loss: csrc/mine.hip around the conv3x3 + BatchNorm + ReLU kernels of the
UNet).  A CPU tensor raises: there is no fallback.

The reference reads ``C`` from ``UNet.dimension_dict[layer_name]``, which its ``contrastyou.arch.unet`` never had; here the
caller passes ``input_dim`` (``model.get_channel_dim(layer_name)``).

Both convolutions have a bias (torch's default) in front of a BatchNorm.  In train mode it cannot change any output: the
kernels never read it, its gradient is exact zeros (torch's is rounding noise around 1e-16), and ``running_mean`` moves by
``momentum * bias`` per pass as if it had been added.  In eval mode it is folded into the BatchNorm shift (and, being a
constant there, gets no gradient)."""
from torch import nn

from ... import functional as F_hip
from ... import native as _n


class MineEstimator(nn.Module):

    def __init__(self, *, layer_name, input_dim):
        super().__init__()
        if input_dim < 2 or input_dim % 2 or input_dim // 2 > 256:
            raise ValueError(f"MineEstimator: input_dim must be even, 2 .. 512 (the fused head pools at most 256 channels), "
                             f"got {input_dim}")
        self._layer_name = layer_name
        self._input_dim = input_dim
        self._projector = nn.Sequential(
            nn.Conv2d(input_dim * 2, input_dim, 3, 1, 1),
            nn.BatchNorm2d(input_dim),
            nn.ReLU(inplace=True),

            nn.Conv2d(input_dim, input_dim // 2, 3, 1, 1),
            nn.BatchNorm2d(input_dim // 2),
            nn.ReLU(inplace=True),
            nn.AdaptiveMaxPool2d((1, 1)),
            nn.Flatten(),
            nn.Linear(input_dim // 2, 1)
        )

    def _layer(self, conv, bn):
        c, m = self._projector[conv], self._projector[bn]
        if m.momentum is None:
            raise NotImplementedError("MineEstimator: cumulative-average BatchNorm (momentum=None) is not mirrored")
        track = m.track_running_stats and m.running_mean is not None
        if not track:
            raise NotImplementedError("MineEstimator: BatchNorm without running statistics is not mirrored")
        return (c.weight, c.bias, m.weight, m.bias,
                F_hip.MineBN(m.running_mean, m.running_var, m.num_batches_tracked, self.training, self.training, m.momentum,
                             m.eps))

    def from_feature(self, feature, flip_flags=None, out=None):
        """``forward(feature[n:], flip(feature[:n]))`` from the extracted feature [2n, C, H, W] itself: neither half, nor the
        flipped copy, nor the rolled one is materialised.  ``flip_flags``: uint8 [n] (bit 0 flips H, bit 1 flips W) or None."""
        _n.require_gpu(feature)
        if feature.dim() != 4 or feature.shape[1] != self._input_dim:
            raise ValueError(f"MineEstimator({self._layer_name}): expected [2n, {self._input_dim}, H, W], got "
                             f"{tuple(feature.shape)}")
        lin = self._projector[8]
        return F_hip.mine_loss(feature, flip_flags, (self._layer(0, 1), self._layer(3, 4)), (lin.weight, lin.bias), out=out)

    def forward(self, feat1, feat2):
        """``Em - Ej`` (mineestimator.py:32-36) of two given [n, C, H, W] features (``feat2`` already transformed)"""
        import torch
        _n.require_gpu(feat1, feat2)
        if feat1.shape != feat2.shape:
            raise ValueError(f"MineEstimator: two features of one shape, got {tuple(feat1.shape)} and {tuple(feat2.shape)}")
        return self.from_feature(torch.cat([feat2, feat1], dim=0))


class MineEstimatorArray(nn.Module):
    """``MineEstimatorArray`` (mineestimator.py:39-50) over ``EstimatorList``: one estimator per feature name, iterated in
    insertion order.  ``add`` takes the channel count the reference looked up in ``UNet.dimension_dict``."""

    def __init__(self):
        super().__init__()
        self._estimator_dictionary = nn.ModuleDict()

    def add(self, name: str, *, input_dim: int, **params):
        self._estimator_dictionary[name] = MineEstimator(layer_name=name, input_dim=input_dim)

    def add_interface(self, feature_names, *, model):
        if isinstance(feature_names, str):
            feature_names = [feature_names, ]
        for f in feature_names:
            self.add(name=f, input_dim=model.get_channel_dim(f))

    def __iter__(self):
        return iter(self._estimator_dictionary.values())

    def __len__(self):
        return len(self._estimator_dictionary)

    def __getitem__(self, name):
        return self._estimator_dictionary[name]
