"""Mirror of ``AdversarialEpocher`` (semi_seg/epochers/new_comparable.py:89-206): two networks and two optimizer steps per
iteration.  The segmentation update minimises ``sup_loss + reg_weight * BCE(D(softmax(unlabelled logits)), 1)``, then the
discriminator update minimises ``reg_weight * (BCE(D(softmax(labelled logits)), 1) + BCE(D(softmax(unlabelled logits)),
0))`` on the detached logits of the same forward passes; ``dis_consider_image`` stacks the image in front of the class map
(read in place: nothing is concatenated).  The discriminator runs in train mode in all three passes (three running-statistic
updates per step, as in the reference); the first one computes no gradient of its own parameters (the reference throws
them away, :177).  With ``reg_weight == 0`` the unlabelled loader is never advanced, the discriminator is never launched
and both adversarial meters receive 0.

Meters: the parent's without ``reg_loss``, plus ``adv_reg/{dis_loss, gen_loss, reg_weight}``, fed from device scalars.  The
supervised loss and Dice counts are the fused launch of ``FineTuneEpocher``; each network is one ``FlatParams`` stepped by its
own optimizer, whose coefficient launch carries the meters' device adds.  Eager launches (no hipGraph)."""
import torch
from torch import nn

from ... import functional as F_hip
from ...contrastyou import meters as _meters
from ...contrastyou.meters import AverageValueMeter
from .finetune import unzip_twice_transformed_labeled
from .helper import supervised_loss
from .semi import SemiSupervisedEpocher

TRUE_LABEL, FAKE_LABEL = 1, 0


class AdversarialEpocher(SemiSupervisedEpocher):

    def __init__(self, *, model: nn.Module, optimizer, labeled_loader, unlabeled_loader, sup_criterion, num_batches: int,
                 cur_epoch=0, device="cuda", two_stage: bool = False, disable_bn: bool = False, discriminator=None,
                 discr_optimizer=None, reg_weight=None, dis_consider_image: bool, flat_params=None, discr_flat_params=None,
                 **kwargs):
        super().__init__(model=model, optimizer=optimizer, labeled_loader=labeled_loader, unlabeled_loader=unlabeled_loader,
                         sup_criterion=sup_criterion, num_batches=num_batches, cur_epoch=cur_epoch, device=device,
                         two_stage=two_stage, disable_bn=disable_bn, flat_params=flat_params, **kwargs)
        assert isinstance(discriminator, nn.Module), discriminator
        assert isinstance(discr_optimizer, torch.optim.Optimizer), discr_optimizer
        self._discriminator, self._discr_optimizer = discriminator, discr_optimizer
        self._reg_weight = float(reg_weight)
        self._dis_consider_image = dis_consider_image
        self._discr_flat = discr_flat_params
        from ...optim import is_fused
        if discr_flat_params is not None:
            discr_flat_params.fold_mean = is_fused(discr_optimizer)
        self._unlabeled_iter = None
        self._zero = None

    def _assertion(self):  # new_comparable.py:91-92
        pass

    def configure_meters(self, meters):
        meters = super().configure_meters(meters)
        meters.delete_meters(["reg_loss"])
        with meters.focus_on("adv_reg"):
            meters.register_meter("dis_loss", AverageValueMeter())
            meters.register_meter("gen_loss", AverageValueMeter())
            meters.register_meter("reg_weight", AverageValueMeter())
        return meters

    @property
    def unlabeled_iter(self):
        """created at the first use: with ``reg_weight == 0`` the unlabelled loader is not even asked for an iterator
        (new_comparable.py:202-206)"""
        if self._unlabeled_iter is None:
            self._unlabeled_iter = iter(self._unlabeled_loader)
        return self._unlabeled_iter

    def _run(self):
        self.meters["lr"].add([g["lr"] for g in self._optimizer.param_groups])
        self._model.train()
        self._discriminator.train()
        with self.meters.focus_on("adv_reg"):
            self.meters["reg_weight"].add(self._reg_weight)
        for self.cur_batch_num, labeled_data in zip(range(self._num_batches), self._labeled_loader):
            self.step(labeled_data)

    # ---- one network's backward + optimizer step
    def _backward_and_step(self, loss, flat, optimizer, meter_adds):
        """``meter_adds``: [(group or None, name, device scalar)], recorded on the master rank"""
        if self._unit is None or self._unit.device != loss.device:
            self._unit = F_hip.register_unit_gradient(torch.ones((), dtype=loss.dtype, device=loss.device))
        if flat is not None:
            flat.zero_grad()
            loss.backward(gradient=self._unit)
            flat.gather_grads()
            flat.allreduce_()
        else:
            optimizer.zero_grad(set_to_none=True)
            loss.backward(gradient=self._unit)
        from ...optim import is_fused
        fused = is_fused(optimizer) and flat is not None
        adds = None
        if self.on_master():
            _meters.begin_batch()
            self._add_meters(meter_adds)
            if fused:  # the meters' device adds ride in the optimizer's coefficient launch
                adds = _meters.take_batch()
        if fused:
            optimizer.step(scalar_adds=adds, grad_scale=flat.grad_scale)
        else:
            optimizer.step()
        _meters.flush_batch()

    def _add_meters(self, meter_adds):
        for group, name, value in meter_adds:
            if group is None:
                self.meters[name].add(value.detach())
            else:
                with self.meters.focus_on(group):
                    self.meters[name].add(value.detach())

    def step(self, labeled_data, unlabeled_data=None):
        """one iteration of ``_run_adver`` (new_comparable.py:132-200); returns (sup_loss, gen_loss, dis_loss) as device
        scalars.  ``unlabeled_data``: a batch to use instead of the unlabelled loader's next one."""
        (labeled_image, _), labeled_target, labeled_filename, _, label_group = \
            unzip_twice_transformed_labeled(labeled_data, self._device)
        active = self._reg_weight > 0
        unlabeled_image = None
        if active:
            if unlabeled_data is None:
                unlabeled_data = next(self.unlabeled_iter)
            (unlabeled_image, _), _, unlabeled_filename, unl_partition, unl_group = \
                unzip_twice_transformed_labeled(unlabeled_data, self._device)
        D = self._discriminator
        with_image = self._dis_consider_image
        # ---- update segmentation (:148-173)
        labeled_logits = self._model(labeled_image)
        target = labeled_target.squeeze(1)
        sup_loss, counts = supervised_loss(self._sup_criterion, labeled_logits, target, self.num_classes)
        if self._zero is None or self._zero.device != sup_loss.device:
            self._zero = torch.zeros((), dtype=torch.float32, device=sup_loss.device)
        generator_err = disc_loss = self._zero
        unlabeled_logits = None
        if active:
            unlabeled_logits = self._model(unlabeled_image)
            with D.no_weight_grads():
                generator_err = D.bce(F_hip.softmax_classes(unlabeled_logits), TRUE_LABEL,
                                      image=unlabeled_image if with_image else None)
            generator_loss = sup_loss + self._reg_weight * generator_err
        else:
            generator_loss = sup_loss
        self._backward_and_step(generator_loss, self._flat_params, self._optimizer,
                                [(None, "sup_loss", sup_loss), ("adv_reg", "gen_loss", generator_err)])
        if self.on_master():
            inter, union = counts
            dice = self.meters["sup_dice"]
            dice.add_counts(inter, union, dice.group_names_for(inter.shape[0], list(label_group)))
        # ---- update the discriminator on the detached logits (:174-197)
        if active:
            with torch.no_grad():
                prob_l = F_hip.softmax_classes(labeled_logits.detach())
                prob_u = F_hip.softmax_classes(unlabeled_logits.detach())
            err_l = D.bce(prob_l, TRUE_LABEL, image=labeled_image if with_image else None)
            err_u = D.bce(prob_u, FAKE_LABEL, image=unlabeled_image if with_image else None)
            disc_loss = err_l + err_u
            self._backward_and_step(disc_loss * self._reg_weight, self._discr_flat, self._discr_optimizer,
                                    [("adv_reg", "dis_loss", disc_loss)])
        elif self.on_master():
            with torch.no_grad():
                _meters.begin_batch()
                self._add_meters([("adv_reg", "dis_loss", disc_loss)])
                _meters.flush_batch()
        return sup_loss, generator_err, disc_loss
