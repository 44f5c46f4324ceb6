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

CutMix (``"cutmix"`` in ``on``; off by default; French et al., BMVC 2020, the CPS paper's headline row): the strong perturbation
of this package.  A call draws one box per unlabelled slice on the device (functional.cutmix_boxes from the seed word ``draw``),
mixes ``unlabeled_image`` with itself rolled by one (functional.cutmix_images), runs the model and the peer on the mixed batch
WITH gradient (``SemiSupervisedEpocher._forward_unlabeled``: under ``two_stage`` inside the epocher's ``disable_bn`` context, for
both networks) and takes ONE launch of functional.cross_pseudo_ce_mixed: the teachers are the two networks' logits on the
UNMIXED ``unlabeled_image`` -- the pass the step has already made --, read through the boxes; no mixed teacher map is built.
The term enters like any other map, n_unl of the n_total slices.  ``on: [cutmix]`` alone is the official CPS + CutMix: the
supervised losses plus the mixed term.  ``cutmix = {"prop_range": [0.25, 0.5], "seed": 0}``: the range of a box's share of the
image area and the first seed word; ``draw`` is a registered int32 buffer, advanced by one per call and checkpointed, so a
resumed run draws the boxes the uninterrupted one would.  A batch of fewer than two unlabelled slices has nothing to mix with:
a RuntimeError.

``threshold``: one float or a list of C floats in [0, 1]: a network teaches a pixel only where its confidence reaches the
threshold of the class it predicts.  The default 0 is plain CPS (no threshold vector is passed).  The thresholds are the
buffer ``tau`` of the trainer hook.

Meters, all formed on the device (no synchronisation per step): ``loss`` (the cross term), ``peer_sup_loss``, ``agree`` (the
share of pixels on which the two arg-maxes agree) and ``kept`` (kept pixels of both directions / (2 * pixels)); with CutMix on,
``mixed`` as well (the share of the mixed batch's pixels that lie inside a box).

``val()`` and ``inference()`` use the model alone; the trained peer is in ``__hooks__`` of every checkpoint."""
import torch
from torch import nn

from ... import functional as F_hip
from ...contrastyou.hooks.base import EpocherHook, TrainerHook
from ...contrastyou.meters import AverageValueMeter
from ..epochers.helper import supervised_loss
from .mt import compute_dtype_pairs, match_compute_dtype
from .utils import meter_focus

MAPS = ("labeled", "unlabeled", "unlabeled_tf", "cutmix")
DEFAULT_ON = MAPS[:3]  # "cutmix" is never on unless it is named
CUTMIX_DEFAULTS = {"prop_range": (0.25, 0.5), "seed": 0}


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

    def __init__(self, name: str, weight: float, model: nn.Module, threshold=0.0, peer_seed: int = 1, on=DEFAULT_ON,
                 peer: nn.Module = None, cutmix=None):
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
        prop_range, draw = None, None
        if cutmix is not None and "cutmix" not in on:
            raise ValueError(f"CrossPseudoTrainerHook: a `cutmix` section is given but `on` = {on} does not name \"cutmix\" -- "
                             "add it to `on`, or drop the section")
        if "cutmix" in on:
            section = dict(CUTMIX_DEFAULTS, **(dict(cutmix) if cutmix is not None else {}))
            unknown = sorted(set(section) - set(CUTMIX_DEFAULTS))
            if unknown:
                raise ValueError(f"CrossPseudoTrainerHook: `cutmix` has no key {unknown} (some of {sorted(CUTMIX_DEFAULTS)})")
            try:
                prop_range = tuple(float(v) for v in section["prop_range"])
            except (TypeError, ValueError):
                prop_range = ()
            if len(prop_range) != 2 or not 0.0 < prop_range[0] <= prop_range[1] <= 1.0:
                raise ValueError(f"CrossPseudoTrainerHook: cutmix prop_range {section['prop_range']!r} must be a pair with "
                                 "0 < lo <= hi <= 1")
            draw = section["seed"]
            if isinstance(draw, bool) or not isinstance(draw, int) or not 0 <= draw < 2 ** 31:
                raise ValueError(f"CrossPseudoTrainerHook: cutmix seed must be an integer in [0, 2^31), given {draw!r}")
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
        self._prop_range = prop_range  # None: no CutMix, and neither the buffer nor the meter below exists
        if prop_range is not None:
            self.register_buffer("draw", torch.tensor([draw], dtype=torch.int32))

    @property
    def cutmix(self) -> bool:
        return self._prop_range is not None

    def seed_word(self, device):
        """the box sampler's seed word on ``device`` (moved once when the hook itself was not)"""
        if self.draw.device != device:
            self.draw = self.draw.to(device)
        return self.draw

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
        for key in ("loss", "peer_sup_loss", "agree", "kept") + (("mixed",) if self._owner.cutmix else ()):
            self.meters.register_meter(key, AverageValueMeter())

    def graph_key(self):
        owner = self._owner
        key = (type(self).__name__, float(self._weight), owner._on, "plain" if owner._plain else "tau")
        return key + (owner._prop_range,) if owner.cutmix else key

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
        if owner.cutmix and len(unlabeled_image) < 2:
            raise RuntimeError(f"{type(owner).__name__}: CutMix mixes every unlabelled slice with the next one of its batch; "
                               f"this batch holds {len(unlabeled_image)} unlabelled slice(s), fewer than two")
        peer_logits = epocher._forward_pass(labeled_image=labeled_image, unlabeled_image=unlabeled_image,
                                            unlabeled_image_tf=unlabeled_image_tf, model=peer)
        peer_sup, _ = supervised_loss(epocher._sup_criterion, peer_logits[0], labeled_target, epocher.num_classes)
        student = dict(zip(DEFAULT_ON, (label_logits, unlabeled_logits, unlabeled_tf_logits)))
        theirs = dict(zip(DEFAULT_ON, peer_logits))
        n_unl = len(unlabeled_image)
        n_total = sum(n_unl if m == "cutmix" else len(student[m]) for m in owner._on)
        tau = owner.thresholds(unlabeled_tf_logits.device)
        C = unlabeled_tf_logits.shape[1]
        cross, agree, kept, pixels = None, None, None, 0
        for m in owner._on:
            out = []
            if m == "cutmix":
                s = unlabeled_logits
                term = self._cutmix_term(unlabeled_image, unlabeled_logits, theirs["unlabeled"], tau, n_unl / n_total, out)
                inside = out[1][4 * C + 1]
                self.meters["mixed"].add(inside.to(torch.float32) / float(s.shape[0] * s.shape[2] * s.shape[3]))
            else:
                s, p = student[m], theirs[m]
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

    def _cutmix_term(self, unlabeled_image, unlabeled_logits, peer_unlabeled, tau, share, out):
        """boxes from the seed word, the mixed batch, both networks on it, the criterion read through the boxes"""
        owner, epocher = self._owner, self.epocher
        n_unl, _, H, W = unlabeled_image.shape
        if tuple(unlabeled_logits.shape[2:]) != (H, W) or tuple(peer_unlabeled.shape[2:]) != (H, W):
            raise RuntimeError(f"{type(owner).__name__}: CutMix draws its boxes for the {H} x {W} images and reads the class maps "
                               f"through the same boxes, but the networks return {tuple(unlabeled_logits.shape[2:])} / "
                               f"{tuple(peer_unlabeled.shape[2:])} maps -- it needs a network whose output has its input's size")
        draw = owner.seed_word(unlabeled_image.device)
        boxes = F_hip.cutmix_boxes(draw, n_unl, H, W, owner._prop_range)
        draw.add_(1)
        mixed = F_hip.cutmix_images(unlabeled_image, boxes, 1)
        model_mixed = epocher._forward_unlabeled(mixed)
        peer_mixed = epocher._forward_unlabeled(mixed, model=owner.peer)
        return F_hip.cross_pseudo_ce_mixed(model_mixed, peer_mixed, unlabeled_logits.detach(), peer_unlabeled.detach(), boxes, 1,
                                           tau, share, out=out)
