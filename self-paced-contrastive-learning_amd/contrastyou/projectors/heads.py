"""HIP-backed mirror of ``contrastyou/projectors/heads.py``: ``get_contrastive_projector`` (:9-25) / ``ProjectionHead``
(:78-92) -- global pool -> Linear -> LeakyReLU(0.01) -> Linear -> L2 normalise, one fused call (csrc/projector.hip) -- and
``get_contrastive_dense_projector`` (:28-39) / ``DenseProjectionHead`` (:96-120) -- 1x1-conv MLP on every pixel ->
adaptive pool to ``spatial_size`` -> L2 normalise over channels.  Parameters live at the reference's ``nn.Sequential``
indices so checkpoints interchange (``_header.2.*`` / ``_header.4.*``; ``_projector.0.*`` / ``_projector.2.*``)."""
from torch import nn

from ... import functional as F_hip
import torch

from .nn import _ProjectorHeadBase, Flatten, Normalize, Identical, SoftmaxWithT

__all__ = ["ProjectionHead", "DenseProjectionHead", "ClusterHead", "DenseClusterHead", "get_contrastive_projector",
           "get_contrastive_dense_projector"]


def get_contrastive_projector(*, head_type: str, pool_module, input_dim, hidden_dim, output_dim, normalize: bool):
    if head_type == "mlp":
        return nn.Sequential(pool_module, Flatten(), nn.Linear(input_dim, hidden_dim),
                             nn.LeakyReLU(0.01, inplace=True), nn.Linear(hidden_dim, output_dim),
                             Normalize() if normalize else Identical())
    return nn.Sequential(pool_module, Flatten(), nn.Linear(input_dim, output_dim),
                         Normalize() if normalize else Identical())


def get_contrastive_dense_projector(*, head_type: str, input_dim, hidden_dim, output_dim):
    if head_type == "mlp":
        return nn.Sequential(nn.Conv2d(input_dim, hidden_dim, 1, 1, 0), nn.LeakyReLU(0.01, inplace=True),
                             nn.Conv2d(hidden_dim, output_dim, 1, 1, 0))
    return nn.Sequential(nn.Conv2d(input_dim, output_dim, 1, 1, 0))


class ProjectionHead(_ProjectorHeadBase):
    """``pool_name="adaptive_max"`` pools with the HIP adaptive-max kernel first and hands the [N, C] rows to the fused
    projector.  A ``spatial_size`` other than (1, 1) is accepted by the constructor like the reference's, and fails in
    ``forward`` like the reference's: ``Flatten`` would hand ``C * h * w`` features to ``Linear(C, ...)``."""

    def __init__(self, *, input_dim: int, hidden_dim=256, output_dim: int, head_type: str, normalize: bool,
                 pool_name="adaptive_avg", spatial_size=(1, 1)):
        assert pool_name in ("adaptive_avg", "adaptive_max")
        super().__init__(input_dim=input_dim, output_dim=output_dim, head_type=head_type, normalize=normalize,
                         pool_name=pool_name, spatial_size=spatial_size)
        self._header = get_contrastive_projector(head_type=self._head_type, pool_module=self._pooling_module,
                                                 input_dim=self._input_dim, hidden_dim=hidden_dim,
                                                 output_dim=output_dim, normalize=normalize)

    def forward(self, features, normalize=None):
        """``normalize`` (not in the reference): overrides the constructor's setting for this call -- ``False`` returns the
        rows before ``F.normalize`` for a criterion that normalises in its own launch (``normalize_inputs=True``)"""
        norm = self._normalize if normalize is None else bool(normalize)
        h = self._header
        if tuple(self._spatial_size) != (1, 1):
            k = self._spatial_size[0] * self._spatial_size[1]
            raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({features.shape[0]}x{self._input_dim * k} and "
                               f"{self._input_dim}x{h[2].out_features})")
        if self._pool_name == "adaptive_max":
            features = F_hip.adaptive_pool2d(features, (1, 1), "max")
        if self._head_type == "mlp":
            return F_hip.projector(features, h[2].weight, h[2].bias, h[4].weight, h[4].bias, norm)
        return F_hip.projector(features, h[2].weight, h[2].bias, None, None, norm)


class DenseProjectionHead(_ProjectorHeadBase):
    """heads.py:96-120: the pixel-wise projection of a decoder feature map"""

    def __init__(self, *, input_dim: int, hidden_dim=128, output_dim: int, head_type: str, normalize: bool,
                 pool_name="adaptive_avg", spatial_size=(16, 16)):
        super().__init__(input_dim=input_dim, output_dim=output_dim, head_type=head_type, normalize=normalize,
                         pool_name=pool_name, spatial_size=spatial_size)
        self._projector = get_contrastive_dense_projector(head_type=self._head_type, input_dim=self._input_dim,
                                                          hidden_dim=hidden_dim, output_dim=output_dim)

    def forward(self, features):
        p = self._projector
        if (self._head_type == "mlp" and self._pool_name == "adaptive_avg"
                and F_hip.pixelwise_mlp_pooled_supported(features, p[0].weight, p[2].weight)):
            # average pooling commutes with the (linear) second layer: pool the hidden activation, project the pooled rows
            out = F_hip.pixelwise_mlp_pooled(features, p[0].weight, p[0].bias, p[2].weight, p[2].bias, self._spatial_size)
            return F_hip.l2norm_channels(out) if self._normalize else out
        if self._head_type == "mlp":
            out = F_hip.pixelwise_mlp(features, p[0].weight, p[0].bias, p[2].weight, p[2].bias)
        else:
            out = F_hip.pixelwise_mlp(features, p[0].weight, p[0].bias)
        if self._pool_name in ("adaptive_avg", "adaptive_max"):  # "change resolution here" (:111-112)
            out = F_hip.adaptive_pool2d(out, self._spatial_size, "max" if self._pool_name == "adaptive_max" else "avg")
        if self._normalize:
            return F_hip.l2norm_channels(out)
        return out


# ---------------------------------------------------------------------------------------------- IIC cluster heads
def init_sub_header(*, head_type, input_dim, num_clusters, normalize, T):
    """heads.py:42-58 (same modules, same construction order: same initial weights under one seed)"""
    if head_type == "linear":
        return nn.Sequential(nn.AdaptiveAvgPool2d((1, 1)), Flatten(), nn.Linear(input_dim, num_clusters),
                             Normalize() if normalize else Identical(), SoftmaxWithT(1, T=T))
    return nn.Sequential(nn.AdaptiveAvgPool2d((1, 1)), Flatten(), nn.Linear(input_dim, 128), nn.LeakyReLU(0.01, inplace=True),
                         nn.Linear(128, num_clusters), Normalize() if normalize else Identical(), SoftmaxWithT(1, T=T))


def init_dense_sub_header(head_type, input_dim, hidden_dim, num_clusters, normalize, T):
    """heads.py:61-75"""
    if head_type == "linear":
        return nn.Sequential(nn.Conv2d(input_dim, num_clusters, 1, 1, 0), Normalize() if normalize else Identical(),
                             SoftmaxWithT(1, T=T))
    return nn.Sequential(nn.Conv2d(input_dim, hidden_dim, 1, 1, 0), nn.LeakyReLU(0.01, inplace=True),
                         nn.Conv2d(hidden_dim, num_clusters, 1, 1, 0), Normalize() if normalize else Identical(),
                         SoftmaxWithT(1, T=T))


class _ClusterHeadBase(_ProjectorHeadBase):
    """``logits()`` is what the fused criteria consume: the subheads' outputs after ``Normalize()`` (when ``normalize``) and
    ``SoftmaxWithT``'s division, before the softmax -- one launch of ``functional.group_l2norm_temp`` behind the product,
    none when ``normalize`` is off and ``T == 1``."""

    def _temper(self, lg):
        return F_hip.group_l2norm_temp(lg, num_subheads=len(self._headers), num_clusters=self._output_dim,
                                       normalize=self._normalize, T=self._T)

    def forward(self, features):
        """list of S probability maps, as the reference returns them"""
        lg = self.logits(features)
        K = self._output_dim
        return [lg[:, s * K:(s + 1) * K].softmax(1) for s in range(len(self._headers))]


class ClusterHead(_ClusterHeadBase):
    """heads.py:124-145: S subheads of global average pool -> Linear(C, K) -> softmax; parameters at ``_headers.{s}.2.*``"""

    def __init__(self, *, input_dim: int, num_clusters=5, num_subheads=10, head_type="linear", T=1, normalize=False):
        super().__init__(input_dim=input_dim, output_dim=num_clusters, head_type=head_type, normalize=normalize,
                         pool_name="none", spatial_size=(1, 1))
        self._num_clusters, self._num_subheads, self._T = num_clusters, num_subheads, T
        self._headers = nn.ModuleList([
            init_sub_header(head_type=head_type, input_dim=self._input_dim, num_clusters=self._num_clusters,
                            normalize=self._normalize, T=self._T) for _ in range(self._num_subheads)])

    def logits(self, features):
        """[N, S*K, 1, 1] f32 logits of every subhead (pool + one product over the stacked weights: csrc/projector.hip);
        ``mlp`` subheads: the pooled rows through the stacked first layers, then the S second layers on column slices"""
        if self._head_type == "mlp":
            hs = self._headers
            pooled = F_hip.adaptive_pool2d(features, (1, 1), "avg")
            return self._temper(F_hip.cluster_mlp_logits(
                pooled, torch.cat([h[2].weight for h in hs], 0), torch.cat([h[2].bias for h in hs], 0),
                torch.stack([h[4].weight for h in hs], 0), torch.stack([h[4].bias for h in hs], 0)))
        w = torch.cat([h[2].weight for h in self._headers], 0)
        b = torch.cat([h[2].bias for h in self._headers], 0)
        out = self._temper(F_hip.projector(features, w, b, None, None, False))
        return out.view(out.shape[0], out.shape[1], 1, 1)


class DenseClusterHead(_ClusterHeadBase):
    """heads.py:149-169: S subheads of a 1x1 conv (C -> K) -> softmax over channels; parameters at ``_headers.{s}.0.*``"""

    def __init__(self, *, input_dim: int, num_clusters=10, hidden_dim=64, num_subheads=10, T=1, head_type: str = "linear",
                 normalize: bool = False):
        super().__init__(input_dim=input_dim, output_dim=num_clusters, head_type=head_type, normalize=normalize,
                         pool_name="none", spatial_size=(1, 1))
        self._T = T
        self._headers = nn.ModuleList([
            init_dense_sub_header(head_type=head_type, input_dim=self._input_dim, hidden_dim=hidden_dim,
                                  num_clusters=num_clusters, normalize=self._normalize, T=self._T)
            for _ in range(num_subheads)])

    def logits(self, features):
        """[N, S*K, H, W] f32 logits (channels-last) of every subhead: one pixel-row product over the stacked weights; ``mlp``
        subheads: one product over the stacked first layers, then the S second layers on its column slices"""
        if self._head_type == "mlp":
            hs = self._headers
            return self._temper(F_hip.cluster_mlp_logits(
                features, torch.cat([h[0].weight for h in hs], 0), torch.cat([h[0].bias for h in hs], 0),
                torch.stack([h[2].weight.flatten(1) for h in hs], 0), torch.stack([h[2].bias for h in hs], 0)))
        w = torch.cat([h[0].weight for h in self._headers], 0)
        b = torch.cat([h[0].bias for h in self._headers], 0)
        return self._temper(F_hip.pixelwise_mlp(features, w, b))
