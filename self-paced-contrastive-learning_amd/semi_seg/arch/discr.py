"""Mirror of ``semi_seg/arch/discr.py``: the DCGAN discriminator of the adversarial baseline, five convolutions
C -> h -> 2h -> 4h -> 8h -> 1 (4 x 4, stride 2, padding 1; the last one stride 1, no padding) with BatchNorm2d after the
second to fourth, LeakyReLU(0.2) between them and a sigmoid at the end.

``_main`` is the reference's ``nn.Sequential`` of stock torch modules, kept as the CONTAINER of parameters and buffers:
``state_dict()`` has the reference's keys and shapes by construction (a reference checkpoint loads with ``strict=True``),
``weights_init`` draws what the reference draws, ``train()`` / ``eval()`` / ``to()`` reach the BatchNorms.  None of those
modules is ever called: ``forward`` / ``bce`` run the layers on HIP (functional.discr_*: patch rows + the exact-f32 rows
product, rows BatchNorm, fused head; csrc/discr.hip).  The contiguous [Cout, C, 4, 4] parameter is the product's weight
matrix as it lies, nothing is repacked.  A CPU tensor raises: there is no fallback."""
from contextlib import contextmanager

from torch import nn

from ... import functional as F_hip
from ... import native as _n


def weights_init(m):
    """discr.py:5-11: N(0, 0.02) for convolutions, N(1, 0.02) / 0 for BatchNorm (torch's CPU generator, the caller's seed)"""
    classname = m.__class__.__name__
    if classname.find('Conv') != -1:
        nn.init.normal_(m.weight.data, 0.0, 0.02)
    elif classname.find('BatchNorm') != -1:
        nn.init.normal_(m.weight.data, 1.0, 0.02)
        nn.init.constant_(m.bias.data, 0)


class Discriminator(nn.Module):
    def __init__(self, input_dim, hidden_dim):
        super().__init__()
        if hidden_dim <= 0 or hidden_dim % 4 != 0:
            raise ValueError(f"Discriminator: hidden_dim must be a positive multiple of 4 (the rows product's output width), "
                             f"got {hidden_dim}")
        if input_dim <= 0:
            raise ValueError(f"Discriminator: input_dim {input_dim}")
        self._input_dim, self._hidden_dim = input_dim, hidden_dim
        h = hidden_dim
        self._main = nn.Sequential(
            nn.Conv2d(input_dim, h, 4, 2, 1, bias=False),
            nn.LeakyReLU(0.2, inplace=True),
            nn.Conv2d(h, h * 2, 4, 2, 1, bias=False),
            nn.BatchNorm2d(h * 2),
            nn.LeakyReLU(0.2, inplace=True),
            nn.Conv2d(h * 2, h * 4, 4, 2, 1, bias=False),
            nn.BatchNorm2d(h * 4),
            nn.LeakyReLU(0.2, inplace=True),
            nn.Conv2d(h * 4, h * 8, 4, 2, 1, bias=False),
            nn.BatchNorm2d(h * 8),
            nn.LeakyReLU(0.2, inplace=True),
            nn.Conv2d(h * 8, 1, 4, 1, 0, bias=False),
            nn.Sigmoid()
        )
        self.apply(weights_init)
        self._weight_grads = True

    @contextmanager
    def no_weight_grads(self):
        """passes inside compute no gradient of the discriminator's own parameters and keep nothing for one (the
        segmentation update, new_comparable.py:155-166, whose discriminator gradients :177 throws away); the gradient
        w.r.t. the input is unchanged"""
        prev, self._weight_grads = self._weight_grads, False
        try:
            yield self
        finally:
            self._weight_grads = prev

    def _bn(self, idx):
        m = self._main[idx]
        if m.momentum is None:
            raise NotImplementedError("Discriminator: cumulative-average BatchNorm (momentum=None) is not mirrored")
        track = m.track_running_stats and m.running_mean is not None
        training = self.training or not track
        if training and track:
            m.num_batches_tracked += 1
        return m.weight, m.bias, F_hip.RowsBN(m.running_mean if track else None, m.running_var if track else None, training,
                                              m.momentum, m.eps)

    def _features(self, x, image=None):
        """-> the fourth convolution's pre-BN map; ``image``: stacked in front of ``x`` (read in place, no concatenation)"""
        _n.require_gpu(x, image)
        C = x.shape[1] + (image.shape[1] if image is not None else 0)
        if x.dim() != 4 or C != self._input_dim:
            raise ValueError(f"Discriminator: expected [N, {self._input_dim}, H, W], got {tuple(x.shape)}"
                             + (f" behind an image {tuple(image.shape)}" if image is not None else ""))
        wg = self._weight_grads
        m = self._main
        if image is not None:
            y = F_hip.discr_conv(image, m[0].weight, x2=x, weight_grads=wg)
        else:
            y = F_hip.discr_conv(x, m[0].weight, weight_grads=wg)
        y = F_hip.discr_conv(y, m[2].weight, leaky_in=True, weight_grads=wg)
        for bn, conv in ((3, 5), (6, 8)):
            gamma, beta, cfg = self._bn(bn)
            y = F_hip.discr_bn_conv(y, gamma, beta, m[conv].weight, cfg, weight_grads=wg)
        return y

    def forward(self, input_, image=None):
        """sigmoid(t) [N, 1, h, w] (discr.py:39-40)"""
        y = self._features(input_, image)
        gamma, beta, cfg = self._bn(9)
        return F_hip.discr_bn_head(y, gamma, beta, self._main[11].weight, cfg, weight_grads=self._weight_grads)

    def bce(self, x, label, image=None):
        """``nn.BCELoss()(self(x), full_like(., label))`` with the constant ``label`` 0 or 1, the head, the sigmoid and the
        loss in one launch (what ``AdversarialEpocher`` calls)"""
        y = self._features(x, image)
        gamma, beta, cfg = self._bn(9)
        return F_hip.discr_bn_head(y, gamma, beta, self._main[11].weight, cfg, label=int(label),
                                   weight_grads=self._weight_grads)
