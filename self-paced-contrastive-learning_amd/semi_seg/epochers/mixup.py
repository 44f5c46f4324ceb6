"""Mirror of ``MixUpEpocher`` (semi_seg/epochers/new_comparable.py:18-86): the labelled loader alone; each step a supervised
KL loss on the labelled images plus the registered hooks' regulariser on the labelled pair (both views and both label maps:
the mix-up hook), one backward, one optimizer step.  The reference's meters (``lr``, ``sup_loss``, ``sup_dice``,
``reg_loss`` + the hooks' own) and regularisation keyword set (:60-66).  The supervised loss and Dice counts are the fused
launch of ``FineTuneEpocher``; the parameters are one ``FlatParams`` stepped by ``FusedRAdam``, whose coefficient launch
carries the meters' device adds.  No host synchronisation per step; eager launches (no hipGraph)."""
import random

import torch

from ... import functional as F_hip
from .helper import supervised_loss
from .semi import SemiSupervisedEpocher


def unzip_twice_transformed_pair(data, device):
    """``MixUpEpocher._unzip_data`` (new_comparable.py:35-39): ((image, image_tf, target, target_tf), filename, (partition,
    group)) -> (image, image_tf), (target, target_tf), filename, partition, group"""
    (image, image_tf, target, target_tf), filename, (partition_list, group_list) = data
    return ((image.to(device, non_blocking=True), image_tf.to(device, non_blocking=True)),
            (target.to(device, non_blocking=True), target_tf.to(device, non_blocking=True)), filename, partition_list,
            group_list)


class MixUpEpocher(SemiSupervisedEpocher):

    def init(self):
        self._assertion()
        super().init()

    def _assertion(self):
        """new_comparable.py:20-28: mix-up blends the two views' label maps, so the second view must be transformed on its own
        (``total_freedom``).  A loader that says how its second view is drawn (``_total_freedom``) must say so; a plain
        sequence of batches has nothing to say."""
        for loader in (self._labeled_loader, self._unlabeled_loader):
            if loader is not None and hasattr(loader, "_total_freedom"):
                assert loader._total_freedom is True, "MixUpEpocher needs loaders built with total_freedom=True"

    def _run(self):
        self.meters["lr"].add([g["lr"] for g in self._optimizer.param_groups])
        self._model.train()
        for self.cur_batch_num, labeled_data in zip(range(self._num_batches), self._labeled_loader):
            self.step(labeled_data)

    def _forward_pass(self, labeled_image, **kwargs):  # new_comparable.py:84-86
        return self._model(labeled_image)

    def step(self, labeled_data, seed=None):
        """one iteration of ``_run_mix_up`` (new_comparable.py:42-79); returns (sup_loss, reg_loss) as device scalars"""
        seed = random.randint(0, int(1e7)) if seed is None else seed
        (labeled_image, labeled_image_tf), (labeled_target, labeled_target_tf), labeled_filename, _, label_group = \
            unzip_twice_transformed_pair(labeled_data, self._device)
        label_logits = self.forward_pass(labeled_image=labeled_image, labeled_image_tf=labeled_image_tf)
        target = labeled_target.squeeze(1)
        sup_loss, counts = supervised_loss(self._sup_criterion, label_logits, target, self.num_classes)
        reg_loss = self.regularization(labeled_image=labeled_image, labeled_image_tf=labeled_image_tf,
                                       labeled_target=labeled_target, labeled_target_tf=labeled_target_tf, seed=seed,
                                       label_logits=label_logits)
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


# the reference's ``new_comparable`` module also holds the adversarial epocher
from .adversarial import AdversarialEpocher  # noqa: E402,F401
