"""Float64 CPU restatement of the pseudo-labelling criterion (csrc/pseudo_label.hip: FixMatch's masked cross-entropy and
FreeMatch's self-adaptive thresholds), for its tests.  Flags follow spcl_flip_batch: bit 0 flips H, bit 1 flips W.  All maps
are logical [N, C, H, W]; the teacher map is read through the flips."""
import torch

from tests._iic_oracle import flip


def argmax_lowest(t):
    """arg-max over dim 1 with the lowest class on a tie, stated without relying on ``torch.argmax``'s tie rule"""
    C = t.shape[1]
    idx = torch.arange(C).view(1, C, 1, 1).expand_as(t)
    return torch.where(t == t.max(1, keepdim=True).values, idx, torch.full_like(idx, C)).min(1).values


def conf_and_label(teacher, flags):
    """(float64 confidence [N, H, W] = max softmax(flip(teacher)), label [N, H, W] = arg-max of the flipped f32 LOGITS)"""
    t = flip(teacher, flags)
    return t.double().softmax(1).max(1).values, argmax_lowest(t)


def loss(student64, label, keep, weight=1.0):
    """``weight * mean over ALL pixels of keep * cross_entropy(student, label)``; ``student64`` may require grad, ``keep`` is a
    given [N, H, W] map (the oracle's own or the kernel's)"""
    ce = torch.nn.functional.cross_entropy(student64, label, reduction="none")
    return weight * (ce * keep.double()).mean()


def stats(teacher, flags):
    """float64 [1 + C]: (sum of the confidence, sum of softmax(flip(teacher))_c) over all pixels"""
    q = flip(teacher, flags).double().softmax(1)
    return torch.cat([q.max(1).values.sum().reshape(1), q.sum((0, 2, 3))])


def update(state, stats, M, momentum):
    """FreeMatch's moving averages from one batch's ``stats``: ``state = (tau_g, ptilde[0 .. C))`` float64 ->
    ``(state', tau')``, ``tau'[c] = ptilde'[c] / max ptilde' * tau_g'`` in float64"""
    state, stats = state.double(), stats.double()
    new = momentum * state + (1.0 - momentum) * (stats / float(M))
    return new, new[1:] / new[1:].max() * new[0]
