"""Float64 CPU restatement of the cross-pseudo-supervision criterion (csrc/cross_pseudo.hip), for its tests.  All maps are
logical [N, C, H, W]; both networks saw the same images, so there are no flips."""
import torch

from tests._pseudo_label_oracle import argmax_lowest


def conf_and_label(x):
    """(float64 confidence [N, H, W] = max softmax(x), label [N, H, W] = arg-max of the f32 LOGITS, lowest class on a tie)"""
    return x.double().softmax(1).max(1).values, argmax_lowest(x)


def parts(a64, b64, yA, yB, keepA, keepB, weight=1.0):
    """the two directions, each ``weight * mean over ALL pixels``: (a <- b: keepB * cross_entropy(a, yB), b <- a: keepA *
    cross_entropy(b, yA)); ``a64`` / ``b64`` may require grad, the keep maps are given [N, H, W] maps"""
    ce_a = torch.nn.functional.cross_entropy(a64, yB, reduction="none")
    ce_b = torch.nn.functional.cross_entropy(b64, yA, reduction="none")
    return weight * (ce_a * keepB.double()).mean(), weight * (ce_b * keepA.double()).mean()


def loss(a64, b64, yA, yB, keepA, keepB, weight=1.0):
    """the sum of the two directions; differentiable in both maps (the labels carry no gradient)"""
    pa, pb = parts(a64, b64, yA, yB, keepA, keepB, weight)
    return pa + pb


def hist(yA, yB, keepA, keepB, C):
    """int64 [4 C + 1]: pixels per yA, pixels per yB, kept pixels per yA, kept pixels per yB, pixels with yA == yB"""
    def count(y):
        return torch.bincount(y.flatten(), minlength=C)

    return torch.cat([count(yA), count(yB), count(yA[keepA]), count(yB[keepB]), (yA == yB).sum().reshape(1)])
