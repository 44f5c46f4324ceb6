"""Float64 CPU restatement of the mix-up baseline (semi_seg/hooks/mixup.py: ``mixup_data`` :19-32 and the hook's call
:66-75), written as the reference writes it, for the tests of the mix-up kernels, hook and epocher: the draws under the
step's seed, ``mixed_x``, ``mixed_y`` and the criterion through ``oracle.spcl_oracle.kl_div``."""
import random

import numpy as np
import torch

from oracle import spcl_oracle as O


def draw(seed, batch_size, alpha=1.0):
    """``fix_all_seed_within_context(seed)`` then ``mixup_data``'s draws in its order: ``np.random.beta`` and
    ``torch.randperm(batch_size)``; the three generators are put back as they were"""
    states = random.getstate(), np.random.get_state(), torch.get_rng_state()
    try:
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)
        lam = np.random.beta(alpha, alpha) if alpha > 0 else 1
        index = torch.randperm(batch_size)
    finally:
        random.setstate(states[0])
        np.random.set_state(states[1])
        torch.set_rng_state(states[2])
    return lam, index


def mixed_x(image, image_tf, lam, index):
    x = torch.cat([image, image_tf], dim=0).double()
    return lam * x + (1 - lam) * x[index, :]


def one_hot(labels, C):
    """[N, H, W] labels -> [N, C, H, W] float64; a label outside [0, C) selects no class (an all-zero row)"""
    return torch.stack([(labels == c) for c in range(C)], dim=1).double()


def mixed_y(target, target_tf, lam, index, C):
    """targets [B, 1, H, W] or [B, H, W] -> the blended one-hot maps [2B, C, H, W]"""
    y = torch.cat([target.reshape(target.shape[0], *target.shape[-2:]),
                   target_tf.reshape(target_tf.shape[0], *target_tf.shape[-2:])], dim=0)
    y = one_hot(y, C)
    return lam * y + (1 - lam) * y[index, :]


def mixup_loss(logits64, target, target_tf, lam, index, eps=1e-16):
    """``KL_div()(mixed_pred.softmax(1), mixed_target)`` (mixup.py:75)"""
    return O.kl_div(logits64.softmax(1), mixed_y(target, target_tf, lam, index, logits64.shape[1]), eps)
