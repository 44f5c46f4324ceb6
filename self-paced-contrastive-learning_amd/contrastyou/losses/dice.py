"""Soft-Dice and class-weighted supervised criteria (not in the reference): ``DiceKLLoss``, ``SoftDiceLoss``, ``WeightedKL``.
The arithmetic is csrc/sup_dice.hip (``functional.sup_dice_kl_onehot``): two streaming passes over the class map.

With p = softmax of the logits, t = the one-hot of the label map, M = N H W, S = all classes (or 1 .. C-1 with
``include_background=False``), groups g = the whole batch (G = 1) or one per sample (``per_sample=True``, G = N), and
I_gc = sum p t, P_gc = sum p, T_gc = sum t over the pixels of group g:

    L_dice = 1 - 1 / (G |S|) sum_g sum_{c in S} (2 I_gc + smooth) / (P_gc + T_gc + smooth)
    L_kl   = 1 / M sum_i w[l_i] * -log((p_{i,l_i} + eps) / (1 + eps))
    loss   = dice_weight * L_dice + kl_weight * L_kl

With w == 1, L_kl is ``KL_div``'s value on a one-hot target.  The class weights are used as given (no normalisation).  A label
outside [0, C) is an all-zero one-hot row: it contributes no KL term and nothing to I or T; its probabilities count in P.

None of the classes subclasses ``KL_div``: the epochers' ``isinstance(criterion, KL_div)`` tests keep their meaning, and a
criterion with ``from_logits`` is taken by ``semi_seg.epochers.helper.supervised_loss``."""
import math

import torch
from torch import nn

from ... import functional as F_hip
from ... import native as _n
from .iic_loss import _as_logits

MAX_CLASSES, MAX_SAMPLES = 16, 1024  # (the limits of the head kernels)


class DiceKLLoss(nn.Module):
    """``from_logits(logits [N,C,H,W], labels [N,H,W]) -> loss`` and ``forward(prob, onehot, **kwargs)`` with ``KL_div``'s
    signature.  A call leaves ``last_counts`` = (inter, union) [N, C] int64 (the Dice counts of the arg-max map, as
    ``functional.sup_loss_kl_onehot`` returns them) and ``last_parts`` = a device [2] tensor (L_kl, L_dice).  No call reads
    anything back (``forward`` without ``disable_assert=True`` does, for its one-hot assertion): both entries can be captured
    in a hipGraph."""

    def __init__(self, dice_weight=1.0, kl_weight=1.0, class_weight=None, include_background=True, per_sample=False,
                 smooth=1e-5, eps=1e-16):
        super().__init__()
        dice_weight, kl_weight, smooth, eps = float(dice_weight), float(kl_weight), float(smooth), float(eps)
        if not (math.isfinite(smooth) and smooth > 0):
            raise ValueError(f"smooth must be positive, given {smooth}")
        if dice_weight == 0 and kl_weight == 0:
            raise ValueError("dice_weight and kl_weight are both zero: nothing to optimise")
        if class_weight is not None:
            class_weight = tuple(float(w) for w in (class_weight.tolist() if torch.is_tensor(class_weight) else class_weight))
            if any(not math.isfinite(w) or w < 0 for w in class_weight):
                raise ValueError(f"class weights must be finite and non-negative, given {class_weight}")
        self.dice_weight, self.kl_weight, self.class_weight = dice_weight, kl_weight, class_weight
        self.include_background, self.per_sample = bool(include_background), bool(per_sample)
        self.smooth, self._eps = smooth, eps
        self.last_counts = self.last_parts = None
        self._weights = {}  # (device, C) -> float32 weight vector

    def graph_key(self):
        """every scalar and the weight tuple: what a captured graph of a call bakes in"""
        return (type(self).__name__, self.dice_weight, self.kl_weight, self.class_weight, self.include_background,
                self.per_sample, self.smooth, self._eps)

    def _check_shape(self, N, C):
        if self.class_weight is not None and len(self.class_weight) != C:
            raise ValueError(f"{len(self.class_weight)} class weights for {C} classes")
        if not self.include_background and C < 2:
            raise ValueError("include_background=False leaves no class of a one-class map")
        if C > MAX_CLASSES or N > MAX_SAMPLES:
            raise ValueError(f"at most {MAX_CLASSES} classes and {MAX_SAMPLES} samples per call, given C = {C}, N = {N}")

    def _weight_on(self, device, C):
        w = self._weights.get((device, C))
        if w is None:
            w = torch.tensor(self.class_weight if self.class_weight is not None else [1.0] * C, dtype=torch.float32,
                             device=device)
            self._weights[(device, C)] = w
        return w

    def from_logits(self, logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        if logits.dim() != 4 or labels.dim() != 3:
            raise ValueError(f"logits [N,C,H,W] and labels [N,H,W], given {tuple(logits.shape)} and {tuple(labels.shape)}")
        self._check_shape(logits.shape[0], logits.shape[1])
        _n.require_gpu(logits, labels)
        loss, self.last_counts, self.last_parts = F_hip.sup_dice_kl_onehot(
            logits, labels, self._weight_on(logits.device, logits.shape[1]), dice_weight=self.dice_weight,
            kl_weight=self.kl_weight, include_background=self.include_background, per_sample=self.per_sample,
            smooth=self.smooth, eps=self._eps)
        return loss

    def forward(self, prob: torch.Tensor, target: torch.Tensor, **kwargs) -> torch.Tensor:
        """``prob`` on the simplex, ``target`` its one-hot map: ``from_logits(log(prob), argmax(target))`` (softmax(log p) = p)"""
        if not kwargs.get("disable_assert"):
            assert prob.shape == target.shape
            assert bool(((target == 0) | (target == 1)).all()) and bool((target.sum(1) == 1).all()), "target is not one-hot"
        return self.from_logits(_as_logits(prob), target.argmax(1))


class SoftDiceLoss(DiceKLLoss):
    """``DiceKLLoss`` with ``kl_weight=0``"""

    def __init__(self, class_weight=None, include_background=True, per_sample=False, smooth=1e-5, eps=1e-16):
        super().__init__(dice_weight=1.0, kl_weight=0.0, class_weight=class_weight, include_background=include_background,
                         per_sample=per_sample, smooth=smooth, eps=eps)


class WeightedKL(DiceKLLoss):
    """``DiceKLLoss`` with ``dice_weight=0``: ``KL_div`` on one-hot targets with per-class weights"""

    def __init__(self, class_weight=None, eps=1e-16):
        super().__init__(dice_weight=0.0, kl_weight=1.0, class_weight=class_weight, eps=eps)


SUP_CRITERIA = ("kl", "dice", "dice_kl", "weighted_kl", "boundary")
_DICE_KL_KEYS = ("dice_weight", "kl_weight", "class_weight", "include_background", "per_sample", "smooth")
_BOUNDARY_KEYS = ("alpha", "alpha_step", "alpha_max", "classes")


def build_sup_criterion(config=None):
    """the supervised criterion of a run from the optional config section ``SupCriterion: {name: kl | dice | dice_kl |
    weighted_kl | boundary, dice_weight, kl_weight, class_weight, include_background, per_sample, smooth}``; ``boundary``
    (contrastyou/losses/boundary.py) also takes ``alpha, alpha_step, alpha_max, classes`` and hands ``dice_kl``'s keys to its
    region term; without the section: ``KL_div(verbose=False)``, the reference's"""
    from .kl import KL_div
    section = dict((config or {}).get("SupCriterion") or {})
    name = section.pop("name", "kl")
    if name not in SUP_CRITERIA:
        raise ValueError(f"SupCriterion.name must be one of {SUP_CRITERIA}, given {name!r}")
    allowed = {"kl": (), "dice": ("class_weight", "include_background", "per_sample", "smooth"),
               "dice_kl": _DICE_KL_KEYS, "weighted_kl": ("class_weight",), "boundary": _BOUNDARY_KEYS + _DICE_KL_KEYS}[name]
    unknown = sorted(set(section) - set(allowed))
    if unknown:
        raise ValueError(f"SupCriterion {name!r} does not take {unknown} (it takes {list(allowed)})")
    if name == "kl":
        return KL_div(verbose=False)
    if name == "boundary":
        from .boundary import BoundaryLoss
        own = {k: section.pop(k) for k in _BOUNDARY_KEYS if k in section}
        return BoundaryLoss(region=DiceKLLoss(**section), **own)
    return {"dice": SoftDiceLoss, "dice_kl": DiceKLLoss, "weighted_kl": WeightedKL}[name](**section)
