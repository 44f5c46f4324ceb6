"""Boundary loss (Kervadec et al., MIDL 2019 / MedIA 2021; not in the reference): ``BoundaryLoss`` = a region criterion
(``DiceKLLoss`` or a subclass) + ``alpha`` * L_B, where L_B is the mean, over samples, listed classes and pixels, of the softmax
probability times the signed Euclidean distance to the ground-truth boundary.  The arithmetic is csrc/boundary.hip
(``functional.signed_distance_maps``, ``functional.boundary_loss``).

The distance maps are formed on the device from the label batch of the step (the labelled batch is rotated, cropped and
flipped there; a rotated distance map is not the distance map of the rotated labels).  For sample n and class c in S, with
m = (labels[n] == c) and d2(x) the smallest integer squared distance from x to a pixel of the same slice whose membership in
m differs from x's:

    phi[n, c, x] = +sqrt(d2) outside m,  -(sqrt(d2) - 1) inside m,  0 on a slice where c is absent or fills it
    L_B  = 1 / (N |S| H W) sum_{n, c in S, x} softmax(logits)[n, c, x] * phi[n, c, x]
    loss = L_region + alpha * L_B

Unit pixel spacing only.  ``alpha`` follows the paper's schedule: ``set_epoch(e)`` sets min(alpha_max, alpha + alpha_step *
(e - 1)), a pure function of the epoch (a resumed run needs no saved state), and writes it into a device scalar the kernels
read: a captured step replays with the new weight."""
import math

import torch
from torch import nn

from ... import functional as F_hip
from ... import native as _n
from .dice import MAX_CLASSES, MAX_SAMPLES, DiceKLLoss
from .iic_loss import _as_logits

MAX_SIDE = 1024  # (uint16 column distances: csrc/boundary.hip)


class BoundaryLoss(nn.Module):
    """``from_logits(logits [N,C,H,W], labels [N,H,W]) -> loss`` and ``forward(prob, onehot, **kwargs)`` with ``KL_div``'s
    signature.  A call leaves ``last_counts`` = the region criterion's Dice counts and ``last_parts`` = a device [3] tensor
    (L_kl, L_dice, L_B).  ``from_logits`` reads nothing back and can be captured in a hipGraph; ``alpha`` (host) is the
    weight of the current epoch."""

    def __init__(self, region=None, alpha=0.01, alpha_step=0.01, alpha_max=1.0, classes=None):
        super().__init__()
        region = DiceKLLoss() if region is None else region
        if not isinstance(region, DiceKLLoss):
            raise ValueError(f"region must be a DiceKLLoss (or a subclass), given {type(region).__name__}")
        alpha, alpha_step, alpha_max = float(alpha), float(alpha_step), float(alpha_max)
        for name, v in (("alpha", alpha), ("alpha_step", alpha_step), ("alpha_max", alpha_max)):
            if not math.isfinite(v) or v < 0:
                raise ValueError(f"{name} must be finite and non-negative, given {v}")
        if classes is not None:
            classes = tuple(int(c) for c in classes)
            if not classes or len(set(classes)) != len(classes):
                raise ValueError(f"classes must be a non-empty list of distinct classes, given {classes}")
            if min(classes) < 0 or max(classes) >= MAX_CLASSES:
                raise ValueError(f"classes must lie in [0, C), C <= {MAX_CLASSES}, given {classes}")
        self.region, self.classes = region, classes
        self._alpha0, self.alpha_step, self.alpha_max = alpha, alpha_step, alpha_max
        self.alpha = min(alpha_max, alpha)
        self.last_counts = self.last_parts = None
        self._alpha_on = {}  # device -> float32 scalar the kernels read

    @property
    def _eps(self):  # (the epochers' graph keys carry it)
        return self.region._eps

    def graph_key(self):
        """what a captured graph of a call bakes in: the region's key and the class list -- not ``alpha``, which the kernels
        read from the device"""
        return (type(self).__name__, self.region.graph_key(), self.classes)

    def set_epoch(self, epoch):
        """alpha of epoch 1, 2, ...: min(alpha_max, alpha + alpha_step * (epoch - 1)) (an epoch below 1 counts as 1)"""
        self.alpha = min(self.alpha_max, self._alpha0 + self.alpha_step * max(int(epoch) - 1, 0))
        for t in self._alpha_on.values():
            t.fill_(self.alpha)
        return self.alpha

    def _alpha_tensor(self, device):
        t = self._alpha_on.get(device)
        if t is None:
            t = self._alpha_on[device] = torch.full((), self.alpha, dtype=torch.float32, device=device)
        return t

    def _classes_for(self, C):
        if self.classes is None:
            if C < 2:
                raise ValueError("the default classes 1 .. C-1 are empty for a one-class map")
            return tuple(range(1, C))
        if max(self.classes) >= C:
            raise ValueError(f"classes {self.classes} are not all in [0, {C})")
        return self.classes

    def from_logits(self, logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        if logits.dim() != 4 or labels.dim() != 3:
            raise ValueError(f"logits [N,C,H,W] and labels [N,H,W], given {tuple(logits.shape)} and {tuple(labels.shape)}")
        N, C, H, W = logits.shape
        if C > MAX_CLASSES or N > MAX_SAMPLES:
            raise ValueError(f"at most {MAX_CLASSES} classes and {MAX_SAMPLES} samples per call, given C = {C}, N = {N}")
        if H > MAX_SIDE or W > MAX_SIDE:
            raise ValueError(f"maps of at most {MAX_SIDE} x {MAX_SIDE}, given {H} x {W}")
        classes = self._classes_for(C)
        _n.require_gpu(logits, labels)
        region_loss = self.region.from_logits(logits, labels)
        with torch.no_grad():
            phi = F_hip.signed_distance_maps(labels, classes)
        b_loss, l_b = F_hip.boundary_loss(logits, phi, classes, self._alpha_tensor(logits.device), with_mean=True)
        self.last_counts = self.region.last_counts
        self.last_parts = torch.cat([self.region.last_parts, l_b.reshape(1)])
        return region_loss + b_loss

    def forward(self, prob: torch.Tensor, target: torch.Tensor, **kwargs) -> torch.Tensor:
        """``prob`` on the simplex, ``target`` its one-hot map: ``from_logits(log(prob), argmax(target))``"""
        if not kwargs.get("disable_assert"):
            assert prob.shape == target.shape
            assert bool(((target == 0) | (target == 1)).all()) and bool((target.sum(1) == 1).all()), "target is not one-hot"
        return self.from_logits(_as_logits(prob), target.argmax(1))
