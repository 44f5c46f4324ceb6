"""Minimum trainer for the encoder pre-train path: ``Trainer`` (contrastyou/trainer/base.py:23-155: hook registry,
optimizer + warm-up/cosine schedule, epoch loop), ``_PretrainTrainerMixin`` (semi_seg/trainers/new_pretrain.py:18-104)
and the checkpoint layout of ``contrastyou/trainer/_io.py:49-71`` (``_model``/``_optimizer``/``_scheduler``/
``__hooks__`` sub-dicts, so ``extract_model_state_dict`` style reuse of ``["_model"]`` interchanges).

The reference's RAdam / GradualWarmupScheduler come from the un-vendored ``deepclustering2``; restated by contract with
``torch.optim.RAdam`` (as the fused HIP kernel ``optim.FusedRAdam``) and a linear warm-up to ``multiplier`` x lr over ``warmup_max`` epochs followed by
CosineAnnealingLR(T_max=max_epoch-warmup_max, eta_min=1e-7)."""
import math
import os
import warnings
from typing import Iterable, Optional

import torch
from torch import nn

from ... import ddp as _ddp
from ...optim import FusedAdam, FusedAdamW, FusedRAdam, FusedSGD
from ..epochers import dense_monitor as _dense
from ..epochers.monitor import (LOWER_IS_BETTER, EmbeddingMonitor, expected_keys, monitor_store, parse_monitor,
                                 resolve_select_by)
from ..epochers.pretrain import PretrainDecoderEpocher, PretrainEncoderEpocher
from ..hooks.creator import feature_until_from_hooks


class WarmupCosine:
    def __init__(self, optimizer, *, max_epoch, warmup_max=10, multiplier=300, eta_min=1e-7):
        self.opt = optimizer
        self.base = [g["lr"] for g in optimizer.param_groups]
        self.max_epoch, self.warmup_max, self.multiplier, self.eta_min = max_epoch, warmup_max, multiplier, eta_min
        self.epoch = 0
        self._apply()

    def _lr(self, base):
        e = self.epoch
        if e <= self.warmup_max:
            return base * ((self.multiplier - 1.0) * e / max(1, self.warmup_max) + 1.0)
        top, t_max = base * self.multiplier, max(1, self.max_epoch - self.warmup_max)
        return self.eta_min + (top - self.eta_min) * (1 + math.cos(math.pi * (e - self.warmup_max) / t_max)) / 2

    def _apply(self):
        for g, b in zip(self.opt.param_groups, self.base):
            g["lr"] = self._lr(b)

    def step(self):
        self.epoch += 1
        self._apply()

    def state_dict(self):
        return {"epoch": self.epoch}

    def load_state_dict(self, sd):
        self.epoch = sd["epoch"]
        self._apply()


def read_optim_sched(config, *, lr=None, weight_decay=None, warmup_max=None, multiplier=None, default_lr=1e-7,
                     default_multiplier=400):
    """``Trainer._init_optimizer`` / ``_init_scheduler`` (contrastyou/trainer/base.py:60-83) as data: the optimizer's name
    and keyword set from ``config["Optim"]`` (every key but ``name`` / ``pre_lr`` / ``ft_lr`` reaches the optimizer, :64),
    the scheduler's from ``config["Scheduler"]`` (``None`` when the section is absent: no scheduler, :72-73).  The mirror's
    own keywords (``lr=`` ...) only override when given; the defaults only fill a section-less (``config=None``) call."""
    optim_cfg = dict((config or {}).get("Optim", {}))
    name = optim_cfg.pop("name", "RAdam")
    for k in ("pre_lr", "ft_lr"):
        optim_cfg.pop(k, None)
    if lr is not None:
        optim_cfg["lr"] = lr
    if weight_decay is not None:
        optim_cfg["weight_decay"] = weight_decay
    optim_cfg.setdefault("lr", default_lr)
    optim_cfg.setdefault("weight_decay", 1e-5)
    sched = (config or {}).get("Scheduler", None)
    if config is None or sched is not None or warmup_max is not None or multiplier is not None:
        sched = dict(sched or {})
        if warmup_max is not None:
            sched["warmup_max"] = warmup_max
        if multiplier is not None:
            sched["multiplier"] = multiplier
        sched.setdefault("warmup_max", 10)
        sched.setdefault("multiplier", default_multiplier)
    return name, optim_cfg, sched


_FUSED = {"Adam": FusedAdam, "AdamW": FusedAdamW, "SGD": FusedSGD}
_TORCH_ONLY_KEYS = ("amsgrad", "maximize", "foreach", "capturable", "differentiable", "fused")  # not implemented by the fused steps


def build_optimizer(name, flat_param, optim_cfg):
    """``optim.__dict__[name](...)`` of contrastyou/trainer/base.py:60-69 on the flat parameter.  RAdam, and Adam / AdamW / SGD
    on a CUDA parameter, are the fused HIP steps (torch.optim semantics; the epochers capture the step, fold the data-parallel
    mean and carry the meters only with these).  Any other name, a CPU parameter, or a section that switches on a torch
    feature the fused steps do not implement (``_TORCH_ONLY_KEYS``) gets the ``torch.optim`` class."""
    if name == "RAdam":
        return FusedRAdam([flat_param], **optim_cfg)  # torch.optim.RAdam semantics, HIP kernel
    if name in _FUSED and flat_param.is_cuda and not any(optim_cfg.get(k) for k in _TORCH_ONLY_KEYS):
        return _FUSED[name]([flat_param], **{k: v for k, v in optim_cfg.items() if k not in _TORCH_ONLY_KEYS})
    if hasattr(torch.optim, name):
        return getattr(torch.optim, name)([flat_param], **optim_cfg)
    raise KeyError(name)


class PretrainEncoderTrainer:
    """``PretrainEncoderTrainer`` as ``main_pretrain_encoder.py:54-72`` drives it.

    Accepts the reference's constructor call unchanged --
    ``PretrainEncoderTrainer(model=, labeled_loader=, unlabeled_loader=, val_loader=, test_loader=, criterion=,
    config=, save_dir=, **config["Trainer"])`` (``SemiTrainer.__init__`` ``semi_seg/trainers/new_trainer.py:20-35`` +
    ``_PretrainTrainerMixin.__init__`` ``new_pretrain.py:36-45``): optimiser and schedule are read from
    ``config["Optim"]`` / ``config["Scheduler"]`` in ``init()`` (``contrastyou/trainer/base.py:60-83``), the contrastive
    loader is built from ``unlabeled_loader`` and ``config["ContrastiveLoaderParams"]`` (a missing section raises
    ``RuntimeError`` as the reference does) -- or the mirror's own short form ``chain_dataloader=`` with keyword
    hyper-parameters.  Epoch bookkeeping follows ``new_pretrain.py:69-85``: ``range(max(_cur_epoch + 1, _start_epoch),
    max_epoch)``, i.e. a fresh trainer runs epochs 1 .. max_epoch - 1 and a resumed one continues after the saved epoch.

    ``monitor=`` (NOT in the reference; a dict of ``every``, ``k``, ``max_slices``, ``space``, ``select_by``, or the config's
    ``Monitor`` section): after every ``every``-th epoch the master rank scores the representation on a fixed slice set
    (``semi_seg/epochers/monitor.py``), keeps the dict under ``history[-1]["monitor"]``, updates ``_best_score`` and writes
    ``best.pth`` on an improvement.  Absent, the trainer does what it did.

    ``dense_monitor=`` (NOT in the reference; a dict of ``every``, ``k``, ``max_slices``, ``space``, ``exclude``, ``select_by``,
    or the config's ``DenseMonitor`` section): the same for the contrastive hooks on DECODER features, which ``monitor=`` only
    names in ``skipped`` -- leave-one-scan-out k-NN classification of the pooled cells against the store's label maps
    (``semi_seg/epochers/dense_monitor.py``) into ``history[-1]["dense_monitor"]``, ``_best_score`` and ``best.pth``.  One run
    selects by one key: a run in which both monitors resolve a selection key is refused in ``init()``
    (``DenseMonitor.select_by: false`` records without selecting)."""
    RUN_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))),
                            "runs2")

    def __init__(self, *, model: nn.Module, chain_dataloader: Optional[Iterable] = None, labeled_loader=None,
                 unlabeled_loader=None, val_loader=None, test_loader=None, criterion=None, config: Optional[dict] = None,
                 save_dir: Optional[str] = None, max_epoch: int = 80, num_batches: int = 200, device="cuda",
                 lr=None, weight_decay=None, warmup_max=None, multiplier=None, two_stage: bool = False,
                 disable_bn: bool = False, monitor=None, dense_monitor=None, **kwargs):
        self._model = model
        self._labeled_loader, self._unlabeled_loader = labeled_loader, unlabeled_loader
        self._val_loader, self._test_loader = val_loader, test_loader
        self._criterion = self._sup_criterion = criterion
        self._two_stage, self._disable_bn = two_stage, disable_bn
        self._config = config
        self._save_dir = save_dir
        self._max_epoch, self._num_batches, self._device = max_epoch, num_batches, device
        self._optim_name, self._optim_cfg, self._sched_cfg = read_optim_sched(
            config, lr=lr, weight_decay=weight_decay, warmup_max=warmup_max, multiplier=multiplier, default_lr=5e-7)
        if chain_dataloader is None:
            if config is None or "ContrastiveLoaderParams" not in config:  # new_pretrain.py:38-40
                raise RuntimeError("`ContrastiveLoaderParams` should be found in config, given \n`" +
                                   ", ".join((config or {}).keys()) + "`")
            from ..data import get_contrastive_dataloader  # row N2
            chain_dataloader, self._monitor_loader = get_contrastive_dataloader(
                unlabeled_loader, config["ContrastiveLoaderParams"], device=device)
        self._chain_dataloader = self._contrastive_loader = chain_dataloader
        self.__hooks__ = nn.ModuleList()
        self._inference_until = None
        self._cur_epoch, self._start_epoch, self._best_score = 0, 0, 0
        self._best_epoch = None  # the epoch of `_best_score` (only the monitor writes either)
        self._optimizer = self._scheduler = self._flat = None
        # the pre-training monitor (NOT in the reference; semi_seg/epochers/monitor.py): off unless `monitor=` or the config's
        # `Monitor` section asks for it -- without it nothing below differs from a trainer that has never heard of it
        self._monitor_cfg = parse_monitor(monitor if monitor is not None else (config or {}).get("Monitor"))
        self._monitor = self._monitor_indices = self._monitor_key = None
        # the dense monitor (semi_seg/epochers/dense_monitor.py): off unless `dense_monitor=` or the `DenseMonitor` section
        self._dense_cfg = _dense.parse_dense_monitor(
            dense_monitor if dense_monitor is not None else (config or {}).get("DenseMonitor"))
        self._dense_monitor = self._dense_indices = self._dense_key = None
        self.__initialized__ = False
        self.history = []
        if save_dir and config is not None and _ddp.on_master():  # trainer/base.py:40-41 (dump_config)
            os.makedirs(save_dir, exist_ok=True)
            import yaml
            with open(os.path.join(save_dir, "config.yaml"), "w") as f:
                yaml.safe_dump(config, f)

    @property
    def save_dir(self):
        return str(self._save_dir)

    @staticmethod
    def on_master():
        return _ddp.on_master()

    # new_pretrain.py:47-62
    @property
    def forward_until(self):
        if self._inference_until is None:
            return list(type(self._model).decoder_names)[-1]
        return self._inference_until

    @forward_until.setter
    def forward_until(self, forward_until):
        if isinstance(forward_until, str):
            if forward_until == "all":
                self._inference_until = None
                return
            assert forward_until in type(self._model).arch_elements, forward_until
        self._inference_until = forward_until

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

    # trainer/base.py:44-47,60-83
    def init(self):
        if self._monitor_cfg is not None:
            self._resolve_monitor_key()  # (host only, every rank: a `select_by` the hooks cannot produce is refused HERE)
        if self._dense_cfg is not None:
            self._resolve_dense_key()  # (host only, every rank; after the monitor's: one run selects by one key)
        self._model.to(self._device)
        self.__hooks__.to(self._device)
        _ddp.broadcast_state(self._model, self.__hooks__)
        # call inside ``model.set_grad(False, start=until, include_start=False)`` (main_pretrain_encoder.py:69): only
        # parameters that require grad join the flat parameter, exactly the reference's optimiser membership
        params = [p for p in self._model.parameters() if p.requires_grad]
        hook_params = [p for h in self.__hooks__ for p in h.parameters()]
        # the reference gives model and hook parameters two groups with identical hyper-parameters
        # (trainer/base.py:62-68): one flat parameter is the same optimisation problem
        self._flat = _ddp.FlatParams(params + hook_params)
        self._optimizer = build_optimizer(self._optim_name, self._flat.param, self._optim_cfg)
        self._scheduler = None
        if self._sched_cfg is not None:
            self._scheduler = WarmupCosine(self._optimizer, max_epoch=self._max_epoch, **self._sched_cfg)
        if self._monitor_cfg is not None and _ddp.on_master():
            self._build_monitor(self._monitor_indices)
        if self._dense_cfg is not None and _ddp.on_master():
            self._build_dense_monitor(self._dense_indices)
        self.__initialized__ = True

    def _resolve_monitor_key(self):
        """which key selects best.pth, decided from the registered hooks before anything runs: `select_by` when the monitor
        can report it (`ValueError` otherwise), by default the first hook's `projection/knn_patient`; `None` when no hook taps
        an encoder feature (decoder pre-training with dense hooks only) -- the monitor then records `skipped` in the history
        and leaves `_best_score` and best.pth alone, which a warning says once"""
        store = monitor_store(self._chain_dataloader)
        keys = expected_keys(self._model, self.__hooks__, getattr(store, "data_name", "acdc"), self._monitor_cfg["space"])
        self._monitor_key = resolve_select_by(keys, self._monitor_cfg["select_by"])
        if self._monitor_key is None:
            warnings.warn(f"{type(self).__name__}(monitor=...): no contrastive hook taps an encoder feature, so the monitor has "
                          "nothing to score: it records the skipped hooks and selects no best.pth")

    def _build_monitor(self, indices=None):
        cfg = self._monitor_cfg
        self._monitor = EmbeddingMonitor(self._chain_dataloader, max_slices=cfg["max_slices"], k=cfg["k"], space=cfg["space"],
                                         indices=indices)
        self._monitor_indices = list(self._monitor.indices)

    def _run_monitor(self):
        """one evaluation of the fixed slice set: the dict goes into the epoch's history entry, `_best_score` follows
        `select_by` (the first evaluation always counts), an improvement writes best.pth after last.pth"""
        result = self._monitor.run(self._model, self.__hooks__)
        self.history[-1]["monitor"] = result
        key = self._monitor_key
        if key is None or key not in result:  # nothing to select by (decided in `init()`; a run never adds to that)
            return False
        score = -float(result[key]) if key.rsplit("/", 1)[1] in LOWER_IS_BETTER else float(result[key])
        improved = self._best_epoch is None or score > self._best_score
        if improved:
            self._best_score, self._best_epoch = score, self._cur_epoch
        return improved

    def _resolve_dense_key(self):
        """the dense monitor's part of `init()`, host only: no contrastive hook on a decoder feature, a store without label
        maps, a `select_by` the hooks cannot produce, and a second selector beside the monitor's are each a `ValueError`"""
        name = type(self).__name__
        if not _dense.dense_targets(self.__hooks__):
            raise ValueError(f"{name}(dense_monitor=...): no contrastive hook taps a decoder feature, the dense monitor has "
                             "nothing to score (hooks on encoder features are the business of `monitor=`)")
        if getattr(monitor_store(self._chain_dataloader), "targets", None) is None:
            raise ValueError(f"{name}(dense_monitor=...): the pre-training store has no label maps (`targets`), and the dense "
                             "monitor votes on the classes of its `val` views")
        keys = _dense.expected_keys(self._model, self.__hooks__, self._dense_cfg["space"])
        self._dense_key = _dense.resolve_select_by(keys, self._dense_cfg["select_by"])
        if self._dense_key is not None and self._monitor_key is not None:
            raise ValueError(f"{name}: two selectors for one best.pth -- Monitor selects by {self._monitor_key!r} and DenseMonitor "
                             f"by {self._dense_key!r}; one run selects by one key (`DenseMonitor.select_by: false` records "
                             "without selecting, or leave `Monitor` out)")

    def _build_dense_monitor(self, indices=None):
        cfg = self._dense_cfg
        self._dense_monitor = _dense.DenseEmbeddingMonitor(
            self._chain_dataloader, self.__hooks__, max_slices=cfg["max_slices"], k=cfg["k"], space=cfg["space"],
            exclude=cfg["exclude"], indices=indices)
        self._dense_indices = list(self._dense_monitor.indices)

    def _run_dense_monitor(self):
        """as `_run_monitor`, into `history[-1]["dense_monitor"]`"""
        result = self._dense_monitor.run(self._model, self.__hooks__)
        self.history[-1]["dense_monitor"] = result
        key = self._dense_key
        if key is None or key not in result:
            return False
        score = -float(result[key]) if key.rsplit("/", 1)[1] in _dense.DENSE_LOWER_IS_BETTER else float(result[key])
        improved = self._best_epoch is None or score > self._best_score
        if improved:
            self._best_score, self._best_epoch = score, self._cur_epoch
        return improved

    train_epocher = PretrainEncoderEpocher

    def _create_tra_epoch(self):
        epocher = self.train_epocher(model=self._model, optimizer=self._optimizer,
                                         chain_dataloader=self._chain_dataloader, num_batches=self._num_batches,
                                         cur_epoch=self._cur_epoch, device=self._device,
                                         inference_until=self._inference_until, flat_params=self._flat)
        epocher.add_hooks([h() for h in self.__hooks__])
        epocher.init()
        self._last_epocher = epocher
        return epocher

    def run_tra_epoch(self):
        return self._create_tra_epoch().run()

    # trainer/base.py:85-92, trainers/new_pretrain.py:69-85
    def start_training(self):
        if not self.__initialized__:
            raise RuntimeError(f"{self.__class__.__name__} should call `init()` first")
        from ... import stepgraph as _sg
        try:
            for self._cur_epoch in range(max(self._cur_epoch + 1, self._start_epoch), self._max_epoch):
                stats = self.run_tra_epoch()
                self.history.append(stats)
                if self._scheduler is not None:
                    self._scheduler.step()
                improved = False
                try:
                    if self._monitor is not None and self._cur_epoch % self._monitor_cfg["every"] == 0:
                        improved = self._run_monitor()
                    if self._dense_monitor is not None and self._cur_epoch % self._dense_cfg["every"] == 0:
                        improved = self._run_dense_monitor() or improved
                finally:  # (whatever the monitor does, the epoch that was just trained is saved)
                    if self._save_dir and _ddp.on_master():
                        self.save_to("last.pth")
                if improved and self._save_dir and _ddp.on_master():
                    self.save_to("best.pth")
        finally:
            _sg.gc_release()  # (the epochers' captures keep the collector's heap frozen from one epoch to the next)
        return self.history

    # trainer/_io.py:49-71,120-134
    def state_dict(self):
        return {"_model": self._model.state_dict(), "_optimizer": self._optimizer.state_dict(),
                "_scheduler": self._scheduler.state_dict() if self._scheduler is not None else None,
                "__hooks__": self.__hooks__.state_dict(),
                "_hook_schedulers": [getattr(s, "_scheduler").state_dict() if hasattr(s, "_scheduler") else None
                                     for h in self.__hooks__ for s in getattr(h, "_hooks", [h])],
                "_buffers": dict({"_cur_epoch": self._cur_epoch, "_start_epoch": self._start_epoch,
                                  "_best_score": self._best_score},
                                 **({"_best_epoch": self._best_epoch, "_monitor_indices": list(self._monitor_indices)}
                                    if self._monitor is not None else {}),
                                 **({"_dense_monitor_indices": list(self._dense_indices)}
                                    if self._dense_monitor is not None else {}),
                                 **({"_best_epoch": self._best_epoch}
                                    if self._dense_monitor is not None and self._monitor is None else {}))}

    def load_state_dict(self, sd):
        self._model.load_state_dict(sd["_model"])
        self._optimizer.load_state_dict(sd["_optimizer"])
        if self._scheduler is not None and sd.get("_scheduler") is not None:
            self._scheduler.load_state_dict(sd["_scheduler"])
        self.__hooks__.load_state_dict(sd["__hooks__"])
        subs = [s for h in self.__hooks__ for s in getattr(h, "_hooks", [h])]
        for s, ssd in zip(subs, sd.get("_hook_schedulers", [])):
            if ssd is not None and hasattr(s, "_scheduler"):
                s._scheduler.load_state_dict(ssd)
        self._cur_epoch = sd["_buffers"]["_cur_epoch"]
        self._start_epoch = sd["_buffers"]["_start_epoch"]
        self._best_score = sd["_buffers"].get("_best_score", 0)
        if self._monitor_cfg is not None:
            self._best_epoch = sd["_buffers"].get("_best_epoch")
            saved = sd["_buffers"].get("_monitor_indices")
            if saved is not None and list(saved) != self._monitor_indices:
                self._monitor_indices = list(saved)  # the slice set the saved score was measured on
                if self._monitor is not None:
                    self._build_monitor(self._monitor_indices)
        if self._dense_cfg is not None:
            self._best_epoch = sd["_buffers"].get("_best_epoch")
            saved = sd["_buffers"].get("_dense_monitor_indices")
            if saved is not None and list(saved) != self._dense_indices:
                self._dense_indices = list(saved)  # the slice set the saved score was measured on
                if self._dense_monitor is not None:
                    self._build_dense_monitor(self._dense_indices)

    def save_to(self, save_name=None, name=None):
        name = save_name or name
        os.makedirs(self._save_dir, exist_ok=True)
        tmp = os.path.join(self._save_dir, name + ".tmp")
        torch.save(self.state_dict(), tmp)
        os.replace(tmp, os.path.join(self._save_dir, name))

    def resume_from_path(self, path):
        self.load_state_dict(torch.load(path, map_location="cpu"))


class PretrainDecoderTrainer(PretrainEncoderTrainer):
    """``PretrainDecoderTrainer`` (new_pretrain.py:107-110), driven by ``main_pretrain_decoder.py:53-71`` with
    ``forward_until`` = a decoder feature and ``model.set_grad(True, start="Conv5", end=until, include_start=False)``
    inside ``model.set_grad(False)`` (row N3)."""
    train_epocher = PretrainDecoderEpocher
