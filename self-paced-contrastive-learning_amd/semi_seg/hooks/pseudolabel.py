"""Self-training with confidence-thresholded pseudo-labels: the FixMatch family (Sohn et al., NeurIPS 2020) with, optionally,
the self-adaptive per-class thresholds of FreeMatch (Wang et al., ICLR 2023).  Not in the reference; off unless a config
carries ``PseudoLabelParameters``.

Each call is ONE launch (functional.pseudo_label_ce): the teacher's class map is flipped by the batch's flags, soft-maxed,
its arg-max becomes the pseudo-label and its largest probability the confidence; the student's second view
(``unlabeled_tf_logits``) is trained with cross-entropy towards the labels whose confidence reaches the threshold of their
class, averaged over ALL pixels.  The teacher gets no gradient.

``teacher="self"`` (FixMatch): the teacher map is the detached ``unlabeled_logits`` -- the student's own prediction on the
first view -- read through ``flip_flags``; no extra forward.  ``teacher="ema"``: a mean teacher as in ``mt.py`` (this class
subclasses its trainer hook, like ``ucmt.py``): the teacher copy runs on ``unlabeled_image`` without autograd, and the
one-launch moving average (``ema_step``) runs after the criterion, before the optimizer step.

``threshold``: one float or a list of C floats in (0, 1].  With ``adaptive=True`` its value is ignored (its length is not):
the thresholds start at 1 / C and the criterion's own launch moves them by the batch's statistics with ``momentum`` (see
INTEGRATION.md: a call compares against the thresholds as they stood BEFORE it, one step behind FreeMatch's Algorithm 1).

``tau`` (f32 [C]) and ``state`` (f64 [1 + C]: the global confidence level and the per-class shares; adaptive mode only) are
buffers of the trainer hook: they move with ``.to()``, are broadcast with the hooks, and are saved and restored with
``__hooks__``.  They are built from ``model.num_classes`` when a model is given, otherwise by the first call (or by a
``load_state_dict`` that comes before it).

Meters, all formed on the device (no synchronisation per step): ``loss``, ``mask_ratio`` (kept pixels / all pixels), ``tau``
(the global level ``tau_g`` after the call when adaptive, else the mean fixed threshold) and ``kept_fg`` (of the pixels whose
pseudo-label is not class 0, the share that was kept)."""
import torch
from torch import nn

from ... import functional as F_hip
from ...contrastyou.hooks.base import TrainerHook
from ...contrastyou.meters import AverageValueMeter
from ..epochers.helper import FixRandomSeed
from .mt import MeanTeacherTrainerHook, _MeanTeacherEpocherHook
from .utils import meter_focus

TEACHERS = ("self", "ema")


class PseudoLabelTrainerHook(MeanTeacherTrainerHook):

    def __init__(self, name: str, weight: float, model: nn.Module = None, threshold=0.95, adaptive: bool = False,
                 momentum: float = 0.999, teacher: str = "self", alpha: float = 0.999, weight_decay: float = 1e-5):
        if teacher not in TEACHERS:
            raise ValueError(f"PseudoLabelTrainerHook: teacher {teacher!r} is none of {TEACHERS}")
        if teacher == "ema" and model is None:
            raise ValueError("PseudoLabelTrainerHook: teacher='ema' needs the model (the teacher is a copy of it)")
        values = [float(v) for v in threshold] if isinstance(threshold, (list, tuple)) else None
        for v in (values if values is not None else [float(threshold)]):
            if not 0.0 < v <= 1.0:
                raise ValueError(f"PseudoLabelTrainerHook: threshold {v} outside (0, 1]")
        classes = int(model.num_classes) if model is not None and hasattr(model, "num_classes") else None
        if values is not None and classes is not None and len(values) != classes:
            raise ValueError(f"PseudoLabelTrainerHook: {len(values)} thresholds for {classes} classes")
        if not 0.0 <= float(momentum) < 1.0:
            raise ValueError(f"PseudoLabelTrainerHook: momentum {momentum} outside [0, 1)")
        if teacher == "ema":
            super().__init__(name, weight, model, alpha=alpha, weight_decay=weight_decay, teacher_softmax=True)
        else:  # no teacher copy, no updater: the student's first view is the teacher
            TrainerHook.__init__(self, name)
            self._weight = weight
            self._teacher_model, self._updater, self._flat = None, None, None
        self._teacher = teacher
        self._adaptive, self._momentum = bool(adaptive), float(momentum)
        self._threshold = values if values is not None else float(threshold)
        self.register_buffer("tau", None)
        self.register_buffer("state", None)
        if classes is not None:
            self._build(classes, torch.device("cpu"))
        elif values is not None:
            self._build(len(values), torch.device("cpu"))

    def _build(self, C, device):
        if isinstance(self._threshold, list) and len(self._threshold) != C:
            raise ValueError(f"PseudoLabelTrainerHook: {len(self._threshold)} thresholds for {C} classes")
        if self._adaptive:
            self.tau, self.state = F_hip.pseudo_label_state(C, device)
        else:
            fixed = self._threshold if isinstance(self._threshold, list) else [self._threshold] * C
            self.tau = torch.tensor(fixed, dtype=torch.float32, device=device)

    def thresholds(self, C, device):
        """``(tau, state)`` for maps of C classes on ``device``: built on the first call, moved when the hook was not"""
        if self.tau is None:
            self._build(C, device)
        if self.tau.numel() != C:
            raise ValueError(f"PseudoLabelTrainerHook: thresholds of {self.tau.numel()} classes, class maps of {C}")
        if self.tau.device != device:
            self.tau = self.tau.to(device)
            if self.state is not None:
                self.state = self.state.to(device)
        return self.tau, self.state

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        for key in ("tau", "state"):  # a checkpoint loaded before the first call brings the buffers' shapes with it
            saved = state_dict.get(prefix + key)
            if saved is not None and getattr(self, key) is None:
                setattr(self, key, torch.empty_like(saved))
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def __call__(self):
        return _PseudoLabelEpocherHook(name=self._hook_name, weight=self._weight, owner=self)


class _PseudoLabelEpocherHook(_MeanTeacherEpocherHook):
    def __init__(self, name: str, weight: float, owner: PseudoLabelTrainerHook) -> None:
        super().__init__(name, weight, None, owner._teacher_model, owner._updater, owner)

    @meter_focus
    def configure_meters(self, meters):
        for key in ("loss", "mask_ratio", "tau", "kept_fg"):
            self.meters.register_meter(key, AverageValueMeter())

    def graph_key(self):
        owner = self._owner
        if owner._teacher != "self":  # the moving average's alpha_t is a host value that changes with every step
            return None
        return (type(self).__name__, float(self._weight), owner._momentum, "adaptive" if owner._adaptive else "fixed")

    def _teacher_map(self, unlabeled_image, unlabeled_logits, unlabeled_logits_tf, flip_flags, seed, affine_transformer,
                     device):
        owner = self._owner
        if owner._teacher == "ema":
            with torch.no_grad():
                teacher = owner.teacher_model(unlabeled_image)
            if flip_flags is None:
                with FixRandomSeed(seed):
                    dec = affine_transformer.decisions(len(unlabeled_image))
                flip_flags = torch.tensor([int(d[0]) | (int(d[1]) << 1) for d in dec], dtype=torch.uint8, device=device)
            return teacher, flip_flags
        if unlabeled_logits is not None and flip_flags is not None:
            return unlabeled_logits.detach(), flip_flags
        return unlabeled_logits_tf.detach(), None  # (already in the student's frame)

    @meter_focus
    def __call__(self, *, unlabeled_tf_logits, unlabeled_logits_tf=None, unlabeled_image=None, seed=None,
                 affine_transformer=None, unlabeled_logits=None, flip_flags=None, **kwargs):
        owner = self._owner
        student = self.epocher._model if owner._teacher == "ema" else None
        if student is not None:
            self._match_compute_dtype(student)
        teacher, flags = self._teacher_map(unlabeled_image, unlabeled_logits, unlabeled_logits_tf, flip_flags, seed,
                                           affine_transformer, unlabeled_tf_logits.device)
        N, C, H, W = unlabeled_tf_logits.shape
        tau, state = owner.thresholds(C, unlabeled_tf_logits.device)
        out = []
        loss = F_hip.pseudo_label_ce(teacher, unlabeled_tf_logits, tau, 1.0, flags, state=state, momentum=owner._momentum,
                                     out=out)
        _, hist, _ = out
        counts = hist.to(torch.float32)
        self.meters["loss"].add(loss.detach())
        self.meters["mask_ratio"].add(counts[C:].sum() / float(N * H * W))
        self.meters["tau"].add(state[0].to(torch.float32) if state is not None else tau.mean())
        self.meters["kept_fg"].add(counts[C + 1:].sum() / counts[1:C].sum().clamp_min(1.0))
        if student is not None:
            owner.ema_step(student)
        return self._weight * loss
