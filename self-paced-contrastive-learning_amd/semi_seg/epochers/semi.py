"""Mirror of ``SemiSupervisedEpocher`` (semi_seg/epochers/new_epocher.py:100-238): each step a supervised KL loss on a
labelled batch plus the registered hooks' regularisers on an unlabelled pair, one backward, one optimizer step.

Same control flow, meters (``lr``, ``sup_loss``, ``sup_dice``, ``reg_loss`` + the hooks' own) and the reference's
regularisation keyword set (:176-187), so the InfoNCE hooks run under it as well as the UDA-IIC ones.  Two keywords are
added for the HIP hooks: ``unlabeled_logits`` (before the flip) and ``flip_flags`` (uint8 [n] on the device: bit 0 flips H,
bit 1 flips W -- what ``TensorRandomFlip`` draws under ``FixRandomSeed(seed)``), so the flipped copies are read by
indexing; and two for the hooks that use the labelled batch (semi_seg/hooks/pixelcontrast.py): ``labeled_target`` (the label
maps [n_l, H, W]) and ``label_logits``.  The flipped second view is one ``spcl_flip_batch`` launch -- or, when one hook offers
``strong_view(image_cf, flags)`` (semi_seg/hooks/strongview.py), that hook's strong intensity view of the same flip; the
supervised loss and Dice counts are the fused
launch of ``FineTuneEpocher``; model and hook parameters are one ``FlatParams`` stepped by ``FusedRAdam``, whose
coefficient launch carries the meters' device adds.  No host synchronisation per step; eager launches (no hipGraph)."""
import random
from contextlib import nullcontext
from typing import Iterable, Optional

import torch
from torch import nn

from ... import ddp as _ddp
from ... import functional as F_hip
from ...contrastyou import meters as _meters
from ...contrastyou.meters import AverageValueMeter, UniversalDice
from .finetune import _EpocherBase, unzip_twice_transformed_labeled
from .helper import FixRandomSeed, TensorRandomFlip, begin_epoch, supervised_loss


def _offers_strong_view(hook):
    return callable(getattr(hook, "strong_view", None))


def _nested_strong_view(hook):
    """does a member of a ``CombineEpochHook`` (at any depth) offer ``strong_view``?"""
    members = getattr(hook, "_epocher_hook", ())
    return any(_offers_strong_view(m) or _nested_strong_view(m) for m in members)


class SemiSupervisedEpocher(_EpocherBase):
    meter_focus = "semi"
    _strong_view = None  # the one hook that offers ``strong_view`` (set by ``add_hook``), or None: the plain flip

    def __init__(self, *, model: nn.Module, optimizer, labeled_loader: Iterable, unlabeled_loader: Iterable, sup_criterion,
                 num_batches: int, cur_epoch=0, device="cuda", two_stage: bool = False, disable_bn: bool = False,
                 flat_params: Optional[_ddp.FlatParams] = None, **kwargs):
        self._optimizer = optimizer
        self._labeled_loader, self._unlabeled_loader = labeled_loader, unlabeled_loader
        self._sup_criterion = sup_criterion
        begin_epoch(sup_criterion, cur_epoch)
        self._affine_transformer = TensorRandomFlip(axis=[1, 2], threshold=0.8)
        self._two_stage, self._disable_bn = two_stage, disable_bn
        self._flat_params = flat_params
        from ...optim import is_fused
        if flat_params is not None:
            flat_params.fold_mean = is_fused(optimizer)
        self._hooks = []
        self._unit = None
        super().__init__(model=model, num_batches=num_batches, cur_epoch=cur_epoch, device=device)

    def configure_meters(self, meters):
        C = self.num_classes
        meters.register_meter("lr", AverageValueMeter())
        meters.register_meter("sup_loss", AverageValueMeter())
        meters.register_meter("sup_dice", UniversalDice(C, report_axises=list(range(1, C))))
        meters.register_meter("reg_loss", AverageValueMeter())
        return meters

    # ---- contrastyou/epochers/base.py:47-60
    def add_hook(self, hook):
        if _nested_strong_view(hook):
            raise ValueError(f"{type(self).__name__}: a hook that offers `strong_view` sits inside a combined hook -- it adds no "
                             "loss, which a CombineEpochHook cannot sum; register it with the epocher directly")
        if _offers_strong_view(hook):
            if self._strong_view is not None:
                raise ValueError(f"{type(self).__name__}: a second hook offers `strong_view` -- the unlabelled pair has one "
                                 "second view, made by one hook (drop one of the two StrongViewParameters hooks)")
            self._strong_view = hook
        self._hooks.append(hook)
        hook.set_epocher(self)

    def add_hooks(self, hooks):
        for h in hooks:
            self.add_hook(h)

    def close_hooks(self):
        for h in self._hooks:
            h.close()

    def run(self):
        try:
            return super().run()
        finally:
            self.close_hooks()

    def _run(self):
        self.meters["lr"].add([g["lr"] for g in self._optimizer.param_groups])
        self._model.train()
        for self.cur_batch_num, labeled_data, unlabeled_data in zip(range(self._num_batches), self._labeled_loader,
                                                                     self._unlabeled_loader):
            self.step(labeled_data, unlabeled_data)

    # ---- new_epocher.py:33-50
    def forward_pass(self, **kwargs):
        for h in self._hooks:
            h.before_forward_pass(**kwargs)
        result = self._forward_pass(**kwargs)
        for h in self._hooks:
            h.after_forward_pass(**kwargs, result_dict=result)
        return result

    def regularization(self, **kwargs):
        for h in self._hooks:
            h.before_regularization(**kwargs)
        result = self._regularization(**kwargs)
        for h in self._hooks:
            h.after_regularization(**kwargs, result_dict=result)
        return result

    def _regularization(self, **kwargs):  # new_epocher.py:234-238
        if len(self._hooks) > 0:
            losses = [h(**kwargs) for h in self._hooks]
            # a hook marked ``contributes_loss = False`` (semi_seg/hooks/strongview.py) is called and adds nothing
            losses = [v for h, v in zip(self._hooks, losses) if getattr(h, "contributes_loss", True)]
            if not losses:
                return torch.zeros((), dtype=torch.float, device=self._device)
            total = losses[0]
            for extra in losses[1:]:
                total = total + extra
            return total
        return torch.zeros((), dtype=torch.float, device=self._device)

    def _bn_context(self, model=None):
        """``_disable_tracking_bn_stats`` (new_epocher.py:225-227): batch statistics, running statistics left alone"""
        model = self._model if model is None else model
        return model.set_bn_track(False) if self._disable_bn else nullcontext()

    def _forward_pass(self, labeled_image, unlabeled_image, unlabeled_image_tf, model=None):  # new_epocher.py:205-222
        """``model``: another network to run under the same policy (semi_seg/hooks/cps.py runs its peer); default the model"""
        model = self._model if model is None else model
        n_l, n_unl = len(labeled_image), len(unlabeled_image)
        if not self._two_stage:
            logits = model(torch.cat([labeled_image, unlabeled_image, unlabeled_image_tf], dim=0))
            return torch.split(logits, [n_l, n_unl, n_unl], dim=0)
        label_logits = model(labeled_image)
        with self._bn_context(model):
            unlabeled_logits, unlabeled_tf_logits = torch.split(
                model(torch.cat([unlabeled_image, unlabeled_image_tf], dim=0)), [n_unl, n_unl], dim=0)
        return label_logits, unlabeled_logits, unlabeled_tf_logits

    def _forward_unlabeled(self, image, model=None):
        """one network on ONE unlabelled batch under the policy of ``_forward_pass``'s unlabelled stage: with ``two_stage``
        inside ``_bn_context`` (``disable_bn`` holds for any network), else a plain pass.  For hooks that run forwards of their
        own on images they made (semi_seg/hooks/cps.py runs the model and its peer on the CutMix batch)."""
        model = self._model if model is None else model
        if not self._two_stage:
            return model(image)
        with self._bn_context(model):
            return model(image)

    def flip_flags(self, seed, n):
        """the flag bytes ``TensorRandomFlip`` draws under ``FixRandomSeed(seed)`` for n samples (new_epocher.py:154-155),
        on the device (a pinned host buffer and an asynchronous copy: no synchronisation)"""
        with FixRandomSeed(seed):
            dec = self._affine_transformer.decisions(n)
        host = torch.tensor([int(d[0]) | (int(d[1]) << 1) for d in dec], dtype=torch.uint8)
        if self._device.type != "cuda":
            return host
        return host.pin_memory().to(self._device, non_blocking=True)

    def step(self, labeled_data, unlabeled_data, seed=None):
        """one iteration of ``_run_semi`` (new_epocher.py:145-202); returns (sup_loss, reg_loss) as device scalars"""
        seed = random.randint(0, int(1e7)) if seed is None else seed
        (labeled_image, _), labeled_target, labeled_filename, _, label_group = \
            unzip_twice_transformed_labeled(labeled_data, self._device)
        (unlabeled_image, unlabeled_image_cf), _, unlabeled_filename, unl_partition, unl_group = \
            unzip_twice_transformed_labeled(unlabeled_data, self._device)
        flags = self.flip_flags(seed, len(unlabeled_image))
        if self._strong_view is None:
            unlabeled_image_tf = F_hip.flip_batch(unlabeled_image_cf.contiguous(), flags)
        else:  # the flip with the hook's intensity ops on the way
            unlabeled_image_tf = self._strong_view.strong_view(unlabeled_image_cf, flags)
        label_logits, unlabeled_logits, unlabeled_tf_logits = self.forward_pass(
            labeled_image=labeled_image, unlabeled_image=unlabeled_image, unlabeled_image_tf=unlabeled_image_tf)
        unlabeled_logits_tf = F_hip.flip_batch(unlabeled_logits, flags)
        target = labeled_target.squeeze(1)
        sup_loss, counts = supervised_loss(self._sup_criterion, label_logits, target, self.num_classes)
        reg_loss = self.regularization(
            unlabeled_tf_logits=unlabeled_tf_logits, unlabeled_logits_tf=unlabeled_logits_tf, seed=seed,
            unlabeled_image=unlabeled_image, unlabeled_image_tf=unlabeled_image_tf, label_group=unl_group,
            partition_group=unl_partition, unlabeled_filename=unlabeled_filename, labeled_filename=labeled_filename,
            affine_transformer=self._affine_transformer, unlabeled_logits=unlabeled_logits, flip_flags=flags,
            labeled_target=target, label_logits=label_logits)
        total_loss = sup_loss + reg_loss
        if self._unit is None or self._unit.device != total_loss.device:
            self._unit = F_hip.register_unit_gradient(torch.ones((), dtype=total_loss.dtype, device=total_loss.device))
        if self._flat_params is not None:
            self._flat_params.zero_grad()
            total_loss.backward(gradient=self._unit)
            self._flat_params.gather_grads()
            self._flat_params.allreduce_()
        else:
            self._optimizer.zero_grad(set_to_none=True)
            total_loss.backward(gradient=self._unit)
        self._update(sup_loss, reg_loss)
        if self.on_master():
            inter, union = counts
            dice = self.meters["sup_dice"]
            dice.add_counts(inter, union, dice.group_names_for(inter.shape[0], list(label_group)))
        return sup_loss, reg_loss

    def _update(self, sup_loss, reg_loss):
        from ...optim import is_fused
        if is_fused(self._optimizer) and self._flat_params is not None:
            adds = None
            if self.on_master():  # the meters' device adds ride in the optimizer's coefficient launch
                _meters.begin_batch()
                self.meters["sup_loss"].add(sup_loss.detach())
                self.meters["reg_loss"].add(reg_loss.detach())
                adds = _meters.take_batch()
            self._optimizer.step(scalar_adds=adds, grad_scale=self._flat_params.grad_scale)
            _meters.flush_batch()
        else:
            self._optimizer.step()
            if self.on_master():
                with torch.no_grad():
                    _meters.begin_batch()
                    self.meters["sup_loss"].add(sup_loss.detach())
                    self.meters["reg_loss"].add(reg_loss.detach())
                    _meters.flush_batch()
