"""Label-guided pixel contrast: the common core of the supervised local contrastive loss of Hu et al. (MICCAI 2021), Alonso et
al. (ICCV 2021), ReCo (ICLR 2022) and the cross-image pixel contrast of Wang et al. (ICCV 2021) -- sample a class-balanced set
of pixel embeddings from a decoder feature, pull same-class pixels together, push the others apart.  Not in the reference; off
unless a config carries ``PixelContrastParameters``.

Per call, on the tapped feature ``[B, Cf, h, w]`` of the step's forward passes:

* the labelled rows (the first ``n_l``) get their cell labels from ``labeled_target`` (``functional.pixel_contrast_labels``: a
  cell counts for a class only when every label of its pooling window is that class).  With ``unlabeled_threshold`` the
  first-view unlabelled rows join them: their label map is the arg-max of the detached ``unlabeled_logits`` where its largest
  soft-max probability reaches the threshold and 255 (ignore) elsewhere, through the same rule;
* ``functional.pixel_sample`` chooses up to ``samples_per_class`` cells per class on the device by the hash of their index and
  the seed word ``draw``; ``functional.gather_rows`` reads their feature rows in place; the pixel-wise MLP head
  (``functional.pixelwise_mlp``) and ``functional.l2norm_rows`` run on those ``C * samples_per_class`` rows ONLY;
  ``functional.pixel_supcon`` is the criterion.  The hook returns ``weight * L``;
* a batch whose sample holds ONE class only has positives and no negatives: the criterion's L would only pull that class
  together, so the hook returns an exact 0 (and a zero gradient) for it -- a device-side select on ``count``, as the methods
  above skip a batch without a second class.

``draw`` is a registered int32 buffer, initialised to ``seed``, handed to the sampler as its seed word and advanced by an
in-place ``add_(1)`` after each call: no host value changes from step to step, the buffer is saved and restored with
``__hooks__``.  The head's parameters are ``learnable_modules`` and join the trainer's flat parameter.

Meters, all formed on the device (no synchronisation per step): ``loss``, ``anchors`` (|I| / M: the share of slots that are
valid rows with a positive), ``filled`` (sum of the counts / M) and ``fg_filled`` (the same over the classes >= 1)."""
from typing import List

import torch
from torch import nn

from ... import functional as F_hip
from ...contrastyou.hooks.base import EpocherHook, TrainerHook
from ...contrastyou.meters import AverageValueMeter
from ...contrastyou.projectors.heads import get_contrastive_dense_projector
from ..arch.hook import SingleFeatureExtractor
from .infonce import decoder_names, encoder_names
from .utils import meter_focus


class PixelContrastTrainerHook(TrainerHook):

    def __init__(self, *, name: str, model: nn.Module, feature_name: str = "Up_conv3", weight: float,
                 samples_per_class: int = 256, temperature: float = 0.1, hidden_dim: int = 128, output_dim: int = 64,
                 head_type: str = "mlp", unlabeled_threshold=None, seed: int = 0) -> None:
        super().__init__(hook_name=name)
        if feature_name not in encoder_names + decoder_names:
            raise ValueError(f"PixelContrastTrainerHook: feature {feature_name!r} is none of {encoder_names + decoder_names}")
        if head_type not in ("mlp", "linear"):
            raise ValueError(f"PixelContrastTrainerHook: head_type {head_type!r} is neither 'mlp' nor 'linear'")
        classes = int(model.num_classes)
        F_hip._pixel_contrast_ck("PixelContrastTrainerHook", classes, samples_per_class)
        input_dim = model.get_channel_dim(feature_name)
        for what, v in (("the feature's channels", input_dim), ("hidden_dim", hidden_dim), ("output_dim", output_dim)):
            if int(v) % 4 != 0:
                raise ValueError(f"PixelContrastTrainerHook: {what} = {v} is not a multiple of 4")
        if not 4 <= int(output_dim) <= F_hip.PIXEL_CONTRAST_MAX_D:
            raise ValueError(f"PixelContrastTrainerHook: output_dim = {output_dim} (4 .. {F_hip.PIXEL_CONTRAST_MAX_D})")
        if not float(temperature) > 0.0:
            raise ValueError(f"PixelContrastTrainerHook: temperature {temperature} (> 0)")
        if unlabeled_threshold is not None and not 0.0 < float(unlabeled_threshold) <= 1.0:
            raise ValueError(f"PixelContrastTrainerHook: unlabeled_threshold {unlabeled_threshold} outside (0, 1]")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 31:
            raise ValueError(f"PixelContrastTrainerHook: seed must be an integer in [0, 2^31), given {seed!r}")
        self._feature_name = feature_name
        self._weight = weight
        self._classes, self._samples = classes, int(samples_per_class)
        self._temperature = float(temperature)
        self._head_type = head_type
        self._threshold = None if unlabeled_threshold is None else float(unlabeled_threshold)
        self._extractor = SingleFeatureExtractor(model, feature_name=feature_name)
        self._projector = get_contrastive_dense_projector(head_type=head_type, input_dim=input_dim, hidden_dim=hidden_dim,
                                                          output_dim=output_dim)
        self.register_buffer("draw", torch.tensor([seed], dtype=torch.int32))

    @property
    def learnable_modules(self) -> List[nn.Module]:
        return [self._projector, ]

    def seed_word(self, device):
        """the sampler's seed word on ``device`` (moved once when the hook itself was not)"""
        if self.draw.device != device:
            self.draw = self.draw.to(device)
        return self.draw

    def __call__(self):
        return _PixelContrastEpocherHook(name=self._hook_name, weight=self._weight, owner=self)


class _PixelContrastEpocherHook(EpocherHook):

    def __init__(self, *, name: str, weight: float, owner: PixelContrastTrainerHook) -> None:
        super().__init__(name)
        self._weight = weight
        self._owner = owner
        self._extractor = owner._extractor
        self._extractor.bind()

    @meter_focus
    def configure_meters(self, meters):
        for key in ("loss", "anchors", "filled", "fg_filled"):
            meters.register_meter(key, AverageValueMeter())

    def graph_key(self):
        o = self._owner
        return (type(self).__name__, float(self._weight), o._feature_name, o._classes, o._samples, o._temperature,
                o._head_type, o._threshold)

    def before_forward_pass(self, **kwargs):
        self._extractor.clear()
        self._extractor.set_enable(True)

    def after_forward_pass(self, **kwargs):
        self._extractor.set_enable(False)

    def _label_maps(self, labeled_target, unlabeled_logits):
        """uint8 [n, H, W]: the ground truth of the labelled slices and, with a threshold, the confident arg-max of the first
        unlabelled view (255 elsewhere)"""
        target = labeled_target[:, 0] if labeled_target.dim() == 4 else labeled_target
        if target.dtype != torch.uint8:
            target = target.to(torch.uint8)
        threshold = self._owner._threshold
        if threshold is None:
            return target
        if unlabeled_logits is None:
            raise ValueError("PixelContrastTrainerHook with unlabeled_threshold needs the epocher's `unlabeled_logits` keyword")
        conf, arg = unlabeled_logits.detach().float().softmax(1).max(1)
        pseudo = torch.where(conf >= threshold, arg.to(torch.uint8), 255)
        return torch.cat([target, pseudo], dim=0)

    @meter_focus
    def __call__(self, *, labeled_target=None, unlabeled_logits=None, **kwargs):
        if labeled_target is None:
            raise ValueError("PixelContrastTrainerHook needs the labelled batch's label maps: the epocher's call of "
                             "regularization(...) lacks the `labeled_target` keyword")
        owner = self._owner
        C, K = owner._classes, owner._samples
        labels = self._label_maps(labeled_target, unlabeled_logits)
        feature = self._extractor.feature()[:len(labels)]
        cell_label = F_hip.pixel_contrast_labels(labels, C, tuple(feature.shape[2:]))
        draw = owner.seed_word(feature.device)
        idx, count = F_hip.pixel_sample(cell_label, C, K, draw)
        draw.add_(1)
        loss = self.criterion_of(feature, idx, count)
        loss = loss * ((count > 0).sum() >= 2).to(loss.dtype)  # (no second class, nothing to contrast: 1.0 or 0.0, on the device)
        with torch.no_grad():
            M = float(C * K)
            cnt = count.to(torch.float32)
            self.meters["loss"].add(loss.detach())
            self.meters["anchors"].add(torch.where(count >= 2, cnt, 0.0).sum() / M)
            self.meters["filled"].add(cnt.sum() / M)
            self.meters["fg_filled"].add(cnt[1:].sum() / float((C - 1) * K))
        return self._weight * loss

    def criterion_of(self, feature, idx, count):
        """gather -> head -> unit rows -> criterion, on the ``C * samples_per_class`` chosen rows only"""
        owner = self._owner
        p = owner._projector
        rows = F_hip.gather_rows(feature, idx)
        as_map = rows.view(rows.shape[0], 1, 1, rows.shape[1]).permute(0, 3, 1, 2)  # [M, Cf, 1, 1], read in place
        if owner._head_type == "mlp":
            out = F_hip.pixelwise_mlp(as_map, p[0].weight, p[0].bias, p[2].weight, p[2].bias)
        else:
            out = F_hip.pixelwise_mlp(as_map, p[0].weight, p[0].bias)
        z = F_hip.l2norm_rows(out.reshape(rows.shape[0], -1))
        return F_hip.pixel_supcon(z, count, owner._samples, owner._temperature)

    def close(self):
        self._extractor.remove()
