"""Cross pseudo supervision (CPS; Chen et al., CVPR 2021).  Not in the reference; off unless a config carries
``CrossPseudoParameters``.

Two segmentation networks with different initialisations see the same batches; each is trained with cross-entropy towards
the other's hard arg-max prediction, and both get the ordinary supervised loss.  Every other teacher of this package is the
student itself or a moving average of it, so its errors stay correlated with the student's; the peer's do not.

The trainer hook owns the PEER: a second network of the model's class built from the model's own constructor values under
``fix_all_seed_within_context(peer_seed)`` (or the ``peer`` it is given).  ``learnable_modules`` returns it, so
``SemiTrainer.init()`` puts its parameters into the one flat parameter behind the model's, ``__hooks__`` checkpoints it and
``broadcast_state`` sends it -- the trainer itself knows nothing of it.

Each call runs the peer on the step's three image batches under the epocher's own forward policy (one concatenated pass, or
``two_stage`` with ``disable_bn``: ``SemiSupervisedEpocher._forward_pass(..., model=peer)``), takes the peer's own supervised
loss (the epocher's criterion, unweighted) and ONE launch per class map named in ``on`` (functional.cross_pseudo_ce: both
soft-maxes, both arg-maxes, both directions' cross-entropy and both gradients).  A map of n_seg of the n_total slices enters
with weight n_seg / n_total: the sum is the mean over all pixels of all listed maps.  The hook returns ``peer_sup + weight *
cross``.

``threshold``: one float or a list of C floats in [0, 1]: a network teaches a pixel only where its confidence reaches the
threshold of the class it predicts.  The default 0 is plain CPS (no threshold vector is passed).  The thresholds are the
buffer ``tau`` of the trainer hook.

Meters, all formed on the device (no synchronisation per step): ``loss`` (the cross term), ``peer_sup_loss``, ``agree`` (the
share of pixels on which the two arg-maxes agree) and ``kept`` (kept pixels of both directions / (2 * pixels)).

``val()`` and ``inference()`` use the model alone; the trained peer is in ``__hooks__`` of every checkpoint."""
import torch
from torch import nn

from ... import functional as F_hip
from ...contrastyou.hooks.base import EpocherHook, TrainerHook
from ...contrastyou.meters import AverageValueMeter
from ..epochers.helper import supervised_loss
from .mt import compute_dtype_pairs, match_compute_dtype
from .utils import meter_focus

MAPS = ("labeled", "unlabeled", "unlabeled_tf")


def _build_peer(model: nn.Module, peer_seed: int) -> nn.Module:
    from ...val import fix_all_seed_within_context
    momentum = next((m.momentum for m in model.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)), 0.1)
    with fix_all_seed_within_context(int(peer_seed)):
        return type(model)(input_dim=model._input_dim, num_classes=model.num_classes, max_channel=model._max_channel,
                           momentum=momentum)


def _same_parameters(a: nn.Module, b: nn.Module) -> bool:
    pa, pb = list(a.parameters()), list(b.parameters())
    if len(pa) != len(pb):
        return False
    return all(x.shape == y.shape and torch.equal(x.detach().cpu(), y.detach().cpu()) for x, y in zip(pa, pb))


class CrossPseudoTrainerHook(TrainerHook):

    def __init__(self, name: str, weight: float, model: nn.Module, threshold=0.0, peer_seed: int = 1, on=MAPS,
                 peer: nn.Module = None):
        on = (on,) if isinstance(on, str) else tuple(on)
        if len(on) == 0:
            raise ValueError(f"CrossPseudoTrainerHook: `on` is empty (some of {MAPS})")
        for m in on:
            if m not in MAPS:
                raise ValueError(f"CrossPseudoTrainerHook: `on` names {m!r}, which is none of {MAPS}")
        if len(set(on)) != len(on):
            raise ValueError(f"CrossPseudoTrainerHook: `on` names a map twice: {on}")
        values = [float(v) for v in threshold] if isinstance(threshold, (list, tuple)) else None
        for v in (values if values is not None else [float(threshold)]):
            if not 0.0 <= v <= 1.0:
                raise ValueError(f"CrossPseudoTrainerHook: threshold {v} outside [0, 1]")
        classes = int(model.num_classes)
        if values is not None and len(values) != classes:
            raise ValueError(f"CrossPseudoTrainerHook: {len(values)} thresholds for {classes} classes")
        super().__init__(name)
        self._weight = weight
        self._on = on
        self._peer_seed = int(peer_seed)
        self._peer = peer if peer is not None else _build_peer(model, peer_seed)
        if _same_parameters(self._peer, model):
            raise ValueError("CrossPseudoTrainerHook: the peer's parameters all equal the model's -- two identical networks "
                             "give cross pseudo supervision no signal (another `peer_seed`, or another `peer`)")
        fixed = values if values is not None else [float(threshold)] * classes
        self._plain = all(v == 0.0 for v in fixed)  # plain CPS: no threshold vector is passed
        self.register_buffer("tau", torch.tensor(fixed, dtype=torch.float32))

    @property
    def learnable_modules(self):
        return [self._peer]

    @property
    def peer(self) -> nn.Module:
        return self._peer

    def thresholds(self, device):
        """the threshold vector for maps on ``device`` (moved when the hook was not), or None for plain CPS"""
        if self._plain:
            return None
        if self.tau.device != device:
            self.tau = self.tau.to(device)
        return self.tau

    def __call__(self):
        return _CrossPseudoEpocherHook(name=self._hook_name, weight=self._weight, owner=self)


class _CrossPseudoEpocherHook(EpocherHook):
    def __init__(self, name: str, weight: float, owner: CrossPseudoTrainerHook) -> None:
        super().__init__(name)
        self._weight = weight
        self._owner = owner
        self._images = None
        self._dtype_pairs = None

    @meter_focus
    def configure_meters(self, meters):
        for key in ("loss", "peer_sup_loss", "agree", "kept"):
            self.meters.register_meter(key, AverageValueMeter())

    def graph_key(self):
        owner = self._owner
        return (type(self).__name__, float(self._weight), owner._on, "plain" if owner._plain else "tau")

    def before_forward_pass(self, **kwargs):
        # references, not copies: the same three batches the model is about to see
        if all(k in kwargs for k in ("labeled_image", "unlabeled_image", "unlabeled_image_tf")):
            self._images = (kwargs["labeled_image"], kwargs["unlabeled_image"], kwargs["unlabeled_image_tf"])
        else:
            self._images = None

    @meter_focus
    def __call__(self, *, unlabeled_tf_logits=None, unlabeled_logits=None, label_logits=None, labeled_target=None, **kwargs):
        images, self._images = self._images, None
        if images is None or any(v is None for v in (unlabeled_tf_logits, unlabeled_logits, label_logits, labeled_target)):
            raise RuntimeError(
                f"{type(self._owner).__name__}: the epocher ({self.epocher.__class__.__name__}) did not hand over the labelled "
                "and the two unlabelled image batches with their logits -- cross pseudo supervision runs under "
                "SemiSupervisedEpocher's keyword set, not under an epocher with another one (such as MixUpEpocher)")
        owner, epocher = self._owner, self.epocher
        peer = owner.peer
        if not peer.training:
            peer.train()
        if self._dtype_pairs is None:
            self._dtype_pairs = compute_dtype_pairs(epocher._model, peer)
        match_compute_dtype(self._dtype_pairs)
        labeled_image, unlabeled_image, unlabeled_image_tf = images
        peer_logits = epocher._forward_pass(labeled_image=labeled_image, unlabeled_image=unlabeled_image,
                                            unlabeled_image_tf=unlabeled_image_tf, model=peer)
        peer_sup, _ = supervised_loss(epocher._sup_criterion, peer_logits[0], labeled_target, epocher.num_classes)
        student = dict(zip(MAPS, (label_logits, unlabeled_logits, unlabeled_tf_logits)))
        theirs = dict(zip(MAPS, peer_logits))
        n_total = sum(len(student[m]) for m in owner._on)
        tau = owner.thresholds(unlabeled_tf_logits.device)
        C = unlabeled_tf_logits.shape[1]
        cross, agree, kept, pixels = None, None, None, 0
        for m in owner._on:
            s, p = student[m], theirs[m]
            out = []
            term = F_hip.cross_pseudo_ce(s, p, tau, len(s) / n_total, out=out)
            hist = out[1]
            a, k = hist[4 * C], hist[2 * C:4 * C].sum()
            cross = term if cross is None else cross + term
            agree = a if agree is None else agree + a
            kept = k if kept is None else kept + k
            pixels += s.shape[0] * s.shape[2] * s.shape[3]
        self.meters["loss"].add(cross.detach())
        self.meters["peer_sup_loss"].add(peer_sup.detach())
        self.meters["agree"].add(agree.to(torch.float32) / float(pixels))
        self.meters["kept"].add(kept.to(torch.float32) / float(2 * pixels))
        return peer_sup + self._weight * cross
