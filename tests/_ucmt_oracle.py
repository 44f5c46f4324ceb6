"""Float64 CPU restatement of the uncertainty-aware mean teacher's criterion (semi_seg/epochers/comparable.py:84-105), for
the tests of ``spcl_ucmt_softmax_mse``.  Flags follow spcl_flip_batch: bit 0 flips H, bit 1 flips W.  All maps are logical
[N, C, H, W]; every teacher map (the clean one and the noisy ones) is read through the flips."""
import math

import torch

from tests._iic_oracle import flip


def entropy(noisy, flags, eps=1e-16):
    """the normalised entropy [N, H, W] of the soft-maxed average of the flipped noisy maps (comparable.py:94-96)"""
    avg = sum(flip(t.double(), flags) for t in noisy) / float(len(noisy))
    q = avg.softmax(1)
    return -(q * (q + eps).log()).sum(1) / math.log(q.shape[1])


def mask_of(noisy, flags, threshold, eps=1e-16):
    return (entropy(noisy, flags, eps) <= threshold).double()


def loss(teacher, student64, mask, weight=1.0, flags=None):
    """``weight * (mse(softmax(s), softmax(flip(T)), reduction="none").mean(1) * mask).mean()`` (comparable.py:86,105);
    ``student64`` may require grad, ``mask`` is a given [N, H, W] map (the oracle's own or the kernel's)"""
    t = flip(teacher.double(), flags).softmax(1).detach()
    reg = (student64.softmax(1) - t) ** 2
    return weight * (reg.mean(1) * mask.double()).mean()


def unmasked_mse(teacher, student64, weight=1.0, flags=None):
    """``weight * mse(softmax(flip(T)), softmax(s))``: what the criterion is when every pixel is kept"""
    t = flip(teacher.double(), flags).softmax(1).detach()
    return weight * torch.nn.functional.mse_loss(student64.softmax(1), t)
