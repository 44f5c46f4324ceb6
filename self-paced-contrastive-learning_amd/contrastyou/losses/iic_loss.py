"""HIP-backed mirror of ``contrastyou/losses/iic_loss.py``: ``IIDLoss`` (:17-51), ``IIDSegmentationLoss`` (:54-100),
``IIDSegmentationSmallPathLoss`` (:103-128), ``compute_joint`` (:131-151) and ``patch_generator`` (:154-162), same call
signatures.  The joint, the criterion and its gradient are csrc/iic.hip (functional.iic_loss) and, patch-wise, csrc/iic_patch.hip
(functional.iic_patch_loss); the hooks hand LOGITS to them (the softmax is applied as they are read).

The reference's ``simplex`` asserts are host synchronisations; its UDA-IIC jobs run with PYTHONOPTIMIZE=1
(script/script_generator_discreteMI.py:92), where they are compiled out.  The mirror leaves them out of the hot path:
``check_inputs=True`` restores them for a caller that wants them.  The dense criterion's NaN ``RuntimeError`` is raised
through ``LaggedNanCheck`` (one step late, no per-step readback), or at once when ``lagged=False``."""
import sys

import torch
from torch import Tensor, nn

from ... import functional as F_hip


def _simplex(t: Tensor, dim=1) -> bool:
    s = t.sum(dim)
    return bool(torch.allclose(s, torch.ones_like(s), rtol=1e-4, atol=1e-4)) and bool((t >= 0).all())


def _as_logits(p: Tensor) -> Tensor:
    """probabilities -> logits whose softmax they are (log p; softmax(log p) = p / sum p = p on the simplex)"""
    return torch.log(p.float().clamp_min(1e-38))


class LaggedNanCheck:
    """The NaN guard of IIDSegmentationLoss (iic_loss.py:97-98) without a readback per step: the device flag of step k is
    copied to pinned memory behind the step (with an event) and LOOKED AT when step k + 1 is checked, or by ``flush``
    (the hooks call it when they close), as ``SupCon*Loss.check_lagged`` does."""

    def __init__(self):
        self._slots, self._pending, self._next = [], None, 0

    def push(self, flag: Tensor, loss: Tensor):
        if not flag.is_cuda:
            if int(flag[0]):
                raise RuntimeError(loss)
            return
        if not self._slots:
            self._slots = [[torch.empty(1, dtype=torch.int32).pin_memory(), torch.cuda.Event(), None] for _ in range(2)]
        slot = self._slots[self._next]
        slot[0].copy_(flag.reshape(-1)[:1], non_blocking=True)
        slot[1].record()
        slot[2] = loss.detach()
        prev, self._pending = self._pending, self._next
        self._next ^= 1
        if prev is not None:
            self._look(prev)

    def _look(self, idx):
        host, ev, loss = self._slots[idx]
        ev.synchronize()
        if int(host[0]):
            raise RuntimeError(loss)

    def flush(self):
        if self._pending is not None:
            idx, self._pending = self._pending, None
            self._look(idx)


class IIDLoss(nn.Module):
    """forward(x_out [n, k], x_tf_out [n, k]) -> (loss, loss_no_lamb, p_i_j), lamb = 1"""

    def __init__(self, lamb: float = 1.0, eps: float = sys.float_info.epsilon, check_inputs: bool = False):
        super().__init__()
        self.lamb, self.eps, self.check_inputs = float(lamb), float(eps), check_inputs
        if self.lamb != 1.0:
            raise NotImplementedError("IIDLoss: lamb != 1 (the UDA-IIC hooks use the default)")

    def forward(self, x_out: Tensor, x_tf_out: Tensor):
        assert len(x_out.shape) == 2, x_out.shape
        if self.check_inputs:
            assert _simplex(x_out), "x_out not normalized."
            assert _simplex(x_tf_out), "x_tf_out not normalized."
        n, k = x_out.shape
        out = []
        loss = F_hip.iic_loss(_as_logits(x_out).view(n, k, 1, 1), _as_logits(x_tf_out).view(n, k, 1, 1), num_subheads=1,
                              num_clusters=k, padding=0, dense=False, out=out)
        j = out[0].view(k, k)
        p_i_j = (j + j.t()) / 2.0
        return loss, loss, p_i_j / p_i_j.sum()


class IIDSegmentationLoss(nn.Module):
    """__call__(x_out [n, k, h, w], x_tf_out, mask=None) -> loss (padding = the half window of displacements)"""

    def __init__(self, lamda=1.0, padding=7, eps: float = sys.float_info.epsilon, check_inputs: bool = False,
                 lagged: bool = True):
        super().__init__()
        if float(lamda) != 1.0:
            raise NotImplementedError("IIDSegmentationLoss: lamda != 1 (the UDA-IIC hooks use the default)")
        self.lamda, self.padding, self.eps = lamda, padding, eps
        self.check_inputs = check_inputs
        self._nan = LaggedNanCheck() if lagged else None

    def __call__(self, x_out: Tensor, x_tf_out: Tensor, mask: Tensor = None) -> Tensor:
        if mask is not None:
            raise NotImplementedError("IIDSegmentationLoss: masks (not used by the UDA-IIC hooks)")
        if self.check_inputs:
            assert _simplex(x_out)
        assert x_out.shape == x_tf_out.shape
        k = x_out.shape[1]
        return self.from_logits(_as_logits(x_out), _as_logits(x_tf_out), num_subheads=1, num_clusters=k)

    def from_logits(self, lx: Tensor, ly: Tensor, *, num_subheads: int, num_clusters: int, scale: float = 1.0,
                    flags: Tensor = None) -> Tensor:
        """``scale * sum_s self(softmax(flip(lx)_s), softmax(ly_s))`` of [n, S*K, h, w] logits (the hooks' entry)"""
        out = []
        loss = F_hip.iic_loss(lx, ly, num_subheads=num_subheads, num_clusters=num_clusters, padding=self.padding,
                              dense=True, scale=scale, flags=flags, out=out)
        if self._nan is not None:
            self._nan.push(out[1], loss)
        elif int(out[1][0]):
            raise RuntimeError(loss)
        return loss

    def flush_check(self):
        if self._nan is not None:
            self._nan.flush()


class IIDSegmentationSmallPathLoss(IIDSegmentationLoss):
    """__call__(x_out [n, k, h, w], x_tf_out, mask=None) -> the mean of ``IIDSegmentationLoss`` over the overlapping
    ``patch_size`` patches of the two maps (stride ``patch_size // 2``, the last patch pushed back to the border), all patches
    in one pass of csrc/iic_patch.hip.  The NaN ``RuntimeError`` of iic_loss.py:123 carries the loss (not the list of patch
    losses)."""

    def __init__(self, lamda=1.0, padding=7, eps: float = sys.float_info.epsilon, patch_size=32, check_inputs: bool = False,
                 lagged: bool = True) -> None:
        if float(lamda) != 1.0:
            raise NotImplementedError("IIDSegmentationSmallPathLoss: lamda != 1 (the MIDL baseline uses the default)")
        super().__init__(lamda, padding, eps, check_inputs=check_inputs, lagged=lagged)
        if isinstance(patch_size, (tuple, list)):
            if len(set(patch_size)) != 1:
                raise NotImplementedError(f"IIDSegmentationSmallPathLoss: square patches only, got {patch_size}")
            patch_size = patch_size[0]
        F_hip.iic_patch_starts(1, patch_size)  # (refuses patch_size < 2)
        self._patch_size = (int(patch_size), int(patch_size))
        self._step_size = (int(patch_size) // 2, int(patch_size) // 2)

    def __call__(self, x_out: Tensor, x_tf_out: Tensor, mask: Tensor = None) -> Tensor:
        assert x_out.shape == x_tf_out.shape, (x_out.shape, x_tf_out.shape)
        if mask is not None:
            raise NotImplementedError("IIDSegmentationSmallPathLoss: masks (not used by the MIDL baseline)")
        if self.check_inputs:
            assert _simplex(x_out)
        return self.from_logits(_as_logits(x_out), _as_logits(x_tf_out))

    def from_logits(self, lx: Tensor, ly: Tensor, *, num_subheads: int = 1, num_clusters: int = None, scale: float = 1.0,
                    flags: Tensor = None) -> Tensor:
        """``scale * self(softmax(lx), softmax(flip(ly)))`` of [n, k, h, w] logits (the hook's entry).  ``num_subheads`` /
        ``num_clusters`` are the base class's keywords: one subhead of all k channels is the only layout here.  NOTE the
        flags flip Y here (the MIDL epocher flips the detached map), where the base class's flip X."""
        if int(num_subheads) != 1 or (num_clusters is not None and int(num_clusters) != lx.shape[1]):
            raise NotImplementedError("IIDSegmentationSmallPathLoss: one subhead over all channels only")
        out = []
        loss = F_hip.iic_patch_loss(lx, ly, padding=self.padding, patch_size=self._patch_size[0], scale=scale, flags=flags,
                                    out=out)
        if self._nan is not None:
            self._nan.push(out[1], loss)
        elif int(out[1][0]):
            raise RuntimeError(loss)
        return loss

    def __repr__(self):
        return f"{self.__class__.__name__} with patch_size={self._patch_size} and padding={self.padding}."


def compute_joint(x_out: Tensor, x_tf_out: Tensor, symmetric=True) -> Tensor:
    """iic_loss.py:131-151 (a small [n, k] product: plain tensor ops)"""
    p_i_j = (x_out.unsqueeze(2) * x_tf_out.unsqueeze(1)).sum(dim=0)
    if symmetric:
        p_i_j = (p_i_j + p_i_j.t()) / 2.0
    return p_i_j / p_i_j.sum()


def patch_generator(feature_map, patch_size=(32, 32), step_size=(16, 16)):
    """the crops ``IIDSegmentationSmallPathLoss`` averages over, in row-major order of their starts, for callers that import
    the generator (the criterion above does not go through it).  The starts are ``functional.iic_patch_starts``; a
    ``step_size`` other than half the patch is not what that rule describes and is refused."""
    height, width = feature_map.shape[-2:]
    if tuple(step_size) != (patch_size[0] // 2, patch_size[1] // 2):
        raise NotImplementedError(f"patch_generator: step_size {tuple(step_size)} is not half of patch_size {tuple(patch_size)}")
    for top in F_hip.iic_patch_starts(height, patch_size[0]):
        for left in F_hip.iic_patch_starts(width, patch_size[1]):
            yield feature_map[..., top:top + patch_size[0], left:left + patch_size[1]]
