"""HIP-backed mirror of ``contrastyou/losses/pica_loss.py``: ``PUILoss`` (:9-38) and ``PUISegLoss`` (:41-84), the
partition-uncertainty-index criteria of the PICA baseline, same call signatures.  The criteria and their gradients are
csrc/pica.hip (functional.pica_loss); the dense one shares the displacement joint and its backward with the IIC criteria
(csrc/iic.hip).  The hooks hand LOGITS to ``from_logits`` (the softmax is applied as they are read).

The balance term of ``PUISegLoss`` (pica_loss.py:76-77) keeps the reference's quirk: ``x_out`` has been permuted to
[K, N, H, W] when ``p = x_out.mean(0).view(-1)`` is taken, so the mean runs over the CLASSES and ``p`` has M = N H W entries,
each 1/K on the simplex.  The term is therefore the constant ``log M - (M / K) log K`` with no gradient (in f32 the reference's
own gradient of it is rounding noise).  The mirror computes it on the host in float64 and returns ``f32(ce + lamda * ne)`` as
the reference does -- at decoder sizes a large negative number plus ``ce`` -- and hands ``ce`` out separately: ``last_ce``.

The reference's ``simplex`` asserts are host synchronisations; ``check_inputs=True`` restores them.  The reference has no
NaN check and neither has the mirror: a call makes no host synchronisation and can be captured in the step's hipGraph."""
from torch import Tensor, nn

from ... import functional as F_hip
from .iic_loss import _as_logits, _simplex


class PUILoss(nn.Module):
    """forward(x [n, k], y [n, k]) -> cross-entropy of the cosine matrix of the columns against its diagonal + lamda * the
    negative entropy of x's column means (+ log k); ``last_ce`` is the first part of the last call"""

    def __init__(self, lamda=2.0, check_inputs: bool = False):
        super().__init__()
        self.lamda, self.check_inputs = lamda, check_inputs
        self.last_ce = None

    def forward(self, x: Tensor, y: Tensor) -> Tensor:
        assert x.shape == y.shape, ('Inputs are required to have same shape')
        if self.check_inputs:
            assert _simplex(x) and _simplex(y)
        n, k = x.shape
        return self.from_logits(_as_logits(x).view(n, k, 1, 1), _as_logits(y).view(n, k, 1, 1), num_subheads=1,
                                num_clusters=k)

    def from_logits(self, lx: Tensor, ly: Tensor, *, num_subheads: int, num_clusters: int, scale: float = 1.0,
                    flags: Tensor = None) -> Tensor:
        """``scale * sum_s self(softmax(lx_s), softmax(ly_s))`` of [n, S*K, 1, 1] logits (the hooks' entry); ``flags`` are
        accepted and ignored: a pooled feature has no orientation"""
        out = []
        loss = F_hip.pica_loss(lx, ly, num_subheads=num_subheads, num_clusters=num_clusters, padding=0, dense=False,
                               lamda=float(self.lamda), scale=scale, out=out)
        self.last_ce = out[0]
        return loss


class PUISegLoss(nn.Module):
    """forward(x_out [n, k, h, w], x_tf_out) -> ce + lamda * ne (padding = the half window of displacements); ``ne`` is the
    constant of the module docstring, ``last_ce`` the ``ce`` of the last call"""

    def __init__(self, lamda=2.0, padding=3, check_inputs: bool = False):
        super().__init__()
        self.lamda, self.padding, self.check_inputs = lamda, padding, check_inputs
        self.last_ce = None

    def forward(self, x_out: Tensor, x_tf_out: Tensor) -> Tensor:
        assert x_out.shape == x_tf_out.shape, ('Inputs are required to have same shape')
        if self.check_inputs:
            assert _simplex(x_out) and _simplex(x_tf_out)
        return self.from_logits(_as_logits(x_out), _as_logits(x_tf_out), num_subheads=1, num_clusters=x_out.shape[1])

    def from_logits(self, lx: Tensor, ly: Tensor, *, num_subheads: int, num_clusters: int, scale: float = 1.0,
                    flags: Tensor = None) -> Tensor:
        """``scale * sum_s self(softmax(flip(lx)_s), softmax(ly_s))`` of [n, S*K, h, w] logits (the hooks' entry)"""
        out = []
        loss = F_hip.pica_loss(lx, ly, num_subheads=num_subheads, num_clusters=num_clusters, padding=self.padding,
                               dense=True, lamda=float(self.lamda), scale=scale, flags=flags, out=out)
        self.last_ce = out[0]
        return loss
