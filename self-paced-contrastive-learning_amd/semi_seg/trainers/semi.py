"""Mirror of ``SemiTrainer`` (semi_seg/trainers/new_trainer.py:17-56): ``FineTuneTrainer``'s epoch loop, evaluation and
best / last checkpoints with the hook registry of the pre-train trainer -- ``register_hooks`` before ``init()``, one flat
parameter over model + hook parameters, ``__hooks__`` in the checkpoint -- and ``SemiSupervisedEpocher`` as the training
epocher (``two_stage`` / ``disable_bn`` from the reference's keyword set).  ``MixUpTrainer`` (:67-72) is the same trainer on
``MixUpEpocher`` (semi_seg/epochers/mixup.py): the labelled loader alone, the mix-up hook as its regulariser.
``AdversarialTrainer`` (:75-120) adds a second network, the DCGAN discriminator, with a flat parameter and an optimizer of
its own, and runs ``AdversarialEpocher`` (semi_seg/epochers/adversarial.py) without hooks."""
import torch
from torch import nn

from ... import ddp as _ddp
from ..epochers.adversarial import AdversarialEpocher
from ..epochers.mixup import MixUpEpocher
from ..epochers.semi import SemiSupervisedEpocher
from .finetune import FineTuneTrainer
from .pretrain import WarmupCosine, build_optimizer


class SemiTrainer(FineTuneTrainer):
    activate_hooks = True

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.__hooks__ = nn.ModuleList()

    # trainer/base.py:49-58
    def register_hook(self, hook):
        from ...contrastyou.hooks.base import TrainerHook
        assert isinstance(hook, TrainerHook), hook
        self.__hooks__.append(hook)

    def register_hooks(self, *hooks):
        if self.__initialized__:
            raise RuntimeError("`register_hook must be called before `init()``")
        for h in hooks:
            self.register_hook(h)

    def init(self):
        self._model.to(self._device)
        self.__hooks__.to(self._device)
        _ddp.broadcast_state(self._model, self.__hooks__)
        params = [p for p in self._model.parameters() if p.requires_grad]
        # (requires_grad: a hook may hold modules that are not trained -- the mean teacher's detached copy of the model --,
        # which travel with ``__hooks__`` (device, broadcast, checkpoint) but are no business of the optimizer)
        hook_params = [p for h in self.__hooks__ for p in h.parameters() if p.requires_grad]
        self._flat = _ddp.FlatParams(params + hook_params)
        self._optimizer = build_optimizer(self._optim_name, self._flat.param, self._optim_cfg)
        self._scheduler = None
        if self._sched_cfg is not None:
            self._scheduler = WarmupCosine(self._optimizer, max_epoch=self._max_epoch, **self._sched_cfg)
        self.__initialized__ = True

    @property
    def train_epocher(self):
        return SemiSupervisedEpocher

    def _create_tra_epoch(self):
        epocher = self.train_epocher(model=self._model, optimizer=self._optimizer, labeled_loader=self._labeled_loader,
                                     unlabeled_loader=self._unlabeled_loader, sup_criterion=self._criterion,
                                     num_batches=self._num_batches, cur_epoch=self._cur_epoch, device=self._device,
                                     two_stage=self._two_stage, disable_bn=self._disable_bn, flat_params=self._flat)
        if self.activate_hooks and len(self.__hooks__) > 0:
            epocher.add_hooks([h() for h in self.__hooks__])
        epocher.init()
        return epocher

    def state_dict(self):
        sd = super().state_dict()
        sd["__hooks__"] = self.__hooks__.state_dict()
        return sd

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        self.__hooks__.load_state_dict(sd["__hooks__"])

    def resume_from_path(self, path):
        self.load_state_dict(torch.load(path, map_location="cpu"))


class MixUpTrainer(SemiTrainer):
    """``MixUpTrainer`` (new_trainer.py:67-72): ``SemiTrainer`` with ``MixUpEpocher`` as its training epocher; the driver
    (main_mixup.py:51-62) registers a ``MixUpHook``"""
    activate_hooks = True

    def __init__(self, **kwargs):
        # no default construction: a trainer is built with ``model=`` and its loaders (every real call is), and
        # tests/test_iic_hooks_host.py::test_main_import_line_resolves_after_install expects ``MixUpTrainer()`` to refuse
        if not kwargs:
            raise NotImplementedError("MixUpTrainer: no default construction (pass model=, the loaders, criterion=, ...)")
        super().__init__(**kwargs)

    @property
    def train_epocher(self):
        return MixUpEpocher


class AdversarialTrainer(SemiTrainer):
    """``AdversarialTrainer`` (new_trainer.py:75-120): ``SemiTrainer`` without hooks on ``AdversarialEpocher``, plus the
    discriminator (``Discriminator(input_dim, hidden_dim=64)`` built under the configured ``RandomSeed``, ``input_dim`` = the
    classes, plus the image channels with ``dis_consider_image``) and its optimizer, built from ``config["Optim"]`` like the
    model's.  That optimizer gets NO scheduler: the discriminator's learning rate stays at ``Optim.lr`` while the model's
    follows the warm-up / cosine schedule (the reference builds ``_dis_optimizer`` by hand, :100-103, outside
    ``_init_scheduler``).  The checkpoint carries both under the names the reference's automatic buffer gives them,
    ``_discriminator`` and ``_dis_optimizer``."""
    activate_hooks = False

    def __init__(self, **kwargs):
        if not kwargs:  # (as MixUpTrainer: no default construction)
            raise NotImplementedError("AdversarialTrainer: no default construction (pass model=, the loaders, criterion=, "
                                      "reg_weight=, ...)")
        if "reg_weight" not in kwargs:
            raise TypeError("AdversarialTrainer.__init__() missing 1 required keyword-only argument: 'reg_weight'")
        reg_weight = kwargs.pop("reg_weight")
        dis_consider_image = bool(kwargs.pop("dis_consider_image", False))
        super().__init__(**kwargs)
        from ...val import fix_all_seed_within_context
        from ..arch.discr import Discriminator
        input_dim = self._model.num_classes + (self._model._input_dim if dis_consider_image else 0)
        self._dis_consider_image = dis_consider_image
        seed = (self._config or {}).get("RandomSeed", 10)
        with fix_all_seed_within_context(seed):
            self._discriminator = Discriminator(input_dim=input_dim, hidden_dim=64)
        self._reg_weight = float(reg_weight)
        self._dis_optimizer = self._dis_flat = None

    def init(self):
        super().init()
        self._discriminator.to(self._device)
        _ddp.broadcast_state(self._discriminator)
        self._dis_flat = _ddp.FlatParams([p for p in self._discriminator.parameters() if p.requires_grad])
        self._dis_optimizer = build_optimizer(self._optim_name, self._dis_flat.param, self._optim_cfg)  # (no scheduler)

    @property
    def train_epocher(self):
        return AdversarialEpocher

    def _create_tra_epoch(self):
        epocher = self.train_epocher(model=self._model, optimizer=self._optimizer, labeled_loader=self._labeled_loader,
                                     unlabeled_loader=self._unlabeled_loader, sup_criterion=self._criterion,
                                     num_batches=self._num_batches, cur_epoch=self._cur_epoch, device=self._device,
                                     two_stage=self._two_stage, disable_bn=self._disable_bn, flat_params=self._flat,
                                     discriminator=self._discriminator, discr_optimizer=self._dis_optimizer,
                                     reg_weight=self._reg_weight, dis_consider_image=self._dis_consider_image,
                                     discr_flat_params=self._dis_flat)
        epocher.init()
        return epocher

    def state_dict(self):
        sd = super().state_dict()
        sd["_discriminator"] = self._discriminator.state_dict()
        sd["_dis_optimizer"] = self._dis_optimizer.state_dict()
        return sd

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        self._discriminator.load_state_dict(sd["_discriminator"])
        self._dis_optimizer.load_state_dict(sd["_dis_optimizer"])
