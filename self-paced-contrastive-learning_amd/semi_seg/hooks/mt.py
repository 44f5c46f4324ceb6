"""Mirror of ``semi_seg/hooks/mt.py`` (:13-55), the mean-teacher baseline: the teacher is a detached deep copy of the
model; each call runs it on the unlabelled images without autograd, takes ``weight * MSELoss(flip(teacher output),
softmax(unlabeled_tf_logits))`` in one launch (functional.mt_softmax_mse: the flip by the batch's flags, the softmax, a
fixed-order mean and the gradient of the student's logits) and then moves the teacher towards the student by the
exponential moving average of ``EMAUpdater`` -- before the optimizer step, as mt.py:54 does.  Meter ``loss``.

The teacher's output enters the criterion as it is: mt.py:49-52 names it ``prob`` but applies no softmax, and parity with
the reference is what this project is measured by.  ``teacher_softmax=True`` soft-maxes it first (the older
``_mixins.py:147``).

The teacher's parameters live in one flat buffer owned by the hook (they are views of it, as ``ddp.FlatParams`` makes the
student's; ``state_dict`` is unaffected).  When the student's parameters are consecutive views of one storage in the same
order -- they are under ``SemiTrainer``, whose ``FlatParams`` puts the model's parameters first -- the moving average is
ONE ``spcl_ema_update`` launch over the two slices; otherwise one launch per parameter tensor.  The teacher's parameters
do not require gradients, so ``SemiTrainer.init`` keeps them out of the optimizer's flat parameter.

``EMAUpdater.step`` is not checkpointed (as in the reference): see its docstring for what a resumed run does."""
from copy import deepcopy

import torch
from torch import nn

from ... import functional as F_hip
from ...contrastyou.ema import EMAUpdater
from ...contrastyou.hooks.base import EpocherHook, TrainerHook
from ...contrastyou.meters import AverageValueMeter
from ..epochers.helper import FixRandomSeed
from .utils import meter_focus

# per-instance caches a model may carry in its ``__dict__`` that must not travel into the copy (captured evaluation graphs
# hold device buffers and the addresses of the source's weights)
_NOT_COPIED_PREFIXES = ("_spcl_",)


def _copy_model(model: nn.Module) -> nn.Module:
    held = {k: model.__dict__.pop(k) for k in list(model.__dict__) if k.startswith(_NOT_COPIED_PREFIXES)}
    try:
        return deepcopy(model)
    finally:
        model.__dict__.update(held)


def _dense_run(tensors):
    """the flat f32 view that covers ``tensors`` when they are contiguous, consecutive pieces of one storage in this
    order; else None"""
    first = tensors[0]
    if first.dtype != torch.float32:
        return None
    storage = first.untyped_storage().data_ptr()
    expect = first.data_ptr()
    for t in tensors:
        if (t.dtype != torch.float32 or not t.is_contiguous() or t.untyped_storage().data_ptr() != storage
                or t.data_ptr() != expect):
            return None
        expect += t.numel() * 4
    total = (expect - first.data_ptr()) // 4
    return first.as_strided((total,), (1,))


def compute_dtype_pairs(student: nn.Module, other: nn.Module):
    """the (student module, other module) pairs that carry a compute dtype, for two networks of one class"""
    return [(s, t) for s, t in zip(student.modules(), other.modules())
            if "_compute_dtype" in s.__dict__ or hasattr(type(s), "_compute_dtype")]


def match_compute_dtype(pairs):
    """give the second network of every pair the compute dtype its student has now (also used by cps.py for its peer)"""
    for s, t in pairs:
        if t._compute_dtype != s._compute_dtype:
            t._compute_dtype = s._compute_dtype


class MeanTeacherTrainerHook(TrainerHook):

    def __init__(self, name: str, weight: float, model: nn.Module, alpha: float = 0.999, weight_decay: float = 1e-5,
                 teacher_softmax: bool = False):
        super().__init__(name)
        self._weight = weight
        self._criterion = nn.MSELoss()
        self._updater = EMAUpdater(alpha=alpha, justify_alpha=True, weight_decay=weight_decay)
        self._teacher_softmax = bool(teacher_softmax)
        self._teacher_model = _copy_model(model)  # keeps the mode (train / eval) the model had: the reference never sets it
        for p in self._teacher_model.parameters():
            p.detach_()
            p.requires_grad_(False)
        self._flat = None

    def __call__(self):
        return _MeanTeacherEpocherHook(name=self._hook_name, weight=self._weight, criterion=self._criterion,
                                       teacher_model=self._teacher_model, updater=self._updater, owner=self)

    @property
    def teacher_model(self):
        return self._teacher_model

    # ---- the teacher's parameters as views of one buffer
    def teacher_flat(self):
        """the flat buffer behind the teacher's parameters; (re)built when they are not its views (first call, or after a
        ``.to(device)`` gave them storages of their own)"""
        params = [p for p in self._teacher_model.parameters()]
        flat = self._flat
        if (flat is not None and params[0].data_ptr() == flat.data_ptr()
                and params[-1].data_ptr() + params[-1].numel() * 4 == flat.data_ptr() + flat.numel() * 4
                and params[0].device == flat.device):
            return flat
        if any(p.dtype != torch.float32 for p in params):
            raise TypeError("MeanTeacherTrainerHook: the teacher's parameters must be float32 (as the model's are)")
        flat = torch.empty(sum(p.numel() for p in params), dtype=torch.float32, device=params[0].device)
        off = 0
        with torch.no_grad():
            for p in params:
                v = flat[off:off + p.numel()].view(p.shape)
                v.copy_(p.data)
                p.data = v
                off += p.numel()
        self._flat = flat
        return flat

    def ema_step(self, student: nn.Module):
        flat = self.teacher_flat()
        sp = [p.data for p in student.parameters()]
        run = _dense_run(sp) if len(sp) > 0 else None
        if run is not None and run.numel() == flat.numel() and run.device == flat.device:
            self._updater.update_flat(flat, run)
        else:
            self._updater(self._teacher_model, student)


class _MeanTeacherEpocherHook(EpocherHook):
    def __init__(self, name: str, weight: float, criterion, teacher_model, updater, owner=None) -> None:
        super().__init__(name)
        self._weight = weight
        self._criterion = criterion
        self._teacher_model = teacher_model
        self._updater = updater
        self._owner = owner
        self._dtype_pairs = None

    @meter_focus
    def configure_meters(self, meters):
        self.meters.register_meter("loss", AverageValueMeter())

    def _match_compute_dtype(self, student):
        if self._dtype_pairs is None:
            self._dtype_pairs = compute_dtype_pairs(student, self._teacher_model)
        match_compute_dtype(self._dtype_pairs)

    @meter_focus
    def __call__(self, *, unlabeled_tf_logits, unlabeled_image, seed, affine_transformer, flip_flags=None, **kwargs):
        student = self.epocher._model
        self._match_compute_dtype(student)
        with torch.no_grad():
            teacher_unlabeled = self._teacher_model(unlabeled_image)
        if flip_flags is None:
            with FixRandomSeed(seed):
                dec = affine_transformer.decisions(len(unlabeled_image))
            flip_flags = torch.tensor([int(d[0]) | (int(d[1]) << 1) for d in dec], dtype=torch.uint8,
                                      device=unlabeled_tf_logits.device)
        loss = F_hip.mt_softmax_mse(teacher_unlabeled, unlabeled_tf_logits, 1.0, flip_flags,
                                    teacher_softmax=self._owner._teacher_softmax if self._owner is not None else False)
        self.meters["loss"].add(loss.detach())
        if self._owner is not None:
            self._owner.ema_step(student)
        else:
            self._updater(ema_model=self._teacher_model, student_model=student)
        return self._weight * loss
