"""HIP-backed mirror of the reference module ``contrastyou/losses/contrast_loss.py``: ``SupConLoss2`` (in / out mode),
``SupConLoss3`` (real-valued ``pos_weight``) and ``SupConLoss4`` (block weights).

Same public names and call contract (reference line numbers cited per symbol).  The three classes are ONE criterion over
pair weights P and a denominator switch E (csrc/supcon_weighted.hip); what differs is where P and E are read from.  No
[2n, 2n] matrix is built unless a tap (``sim_exp``, ``sim_logits``, ``pos_mask``, ``neg_mask``, ``pos_weight``,
``enable_mask``) is read.  Host synchronisation, ``sync_checks``, ``check`` / ``check_lagged`` / ``flush_check``: as in
``contrast_loss3`` (one readback of the result block per call, or none).

The NaN guard follows the reference's arithmetic: a row without positive weight gives 0 / 0 in out mode and the call raises
``RuntimeError(loss)`` (:102-103,179-180,268-269); in in mode the same row gives log(0) / 0 = -inf, which the reference does
not raise for either.  Out of scope: the TensorBoard figures of ``register_writer``."""
from __future__ import annotations

from contextlib import contextmanager

import torch
from torch import Tensor

from ... import functional as F_hip
from .contrast_loss3 import _SupConBase, _capturing, exp_sim_temperature, is_normalized

__all__ = ["SupConLoss2", "SupConLoss3", "SupConLoss4", "is_normalized", "exp_sim_temperature"]


def _block(w, batch_size: int, dev):
    """an [n, n] weight block as the kernel reads it (contiguous float32 on the features' device); the shape is the
    reference's assertion (:63,150) -- or its slice assignment's refusal (:228-235)"""
    assert w.shape == torch.Size([batch_size, batch_size]), (w.shape, batch_size)
    return w.detach().to(device=dev, dtype=torch.float32).contiguous()


_SIMCLR_LABELS = {}


def _simclr_labels(batch_size: int, dev):
    """SimCLR (:76-80): the only positives of a row are its own two views -- every row its own class"""
    key = (batch_size, str(dev))
    lab = _SIMCLR_LABELS.get(key)
    if lab is None:
        lab = torch.arange(batch_size, dtype=torch.float32, device=dev)
        if not _capturing():  # (memory allocated during a capture belongs to that graph: not kept)
            _SIMCLR_LABELS[key] = lab
    return lab


class SupConLoss2(_SupConBase):
    """contrast_loss.py:34-127."""

    def __init__(self, temperature=0.07, out_mode=True, sync_checks=True):
        super().__init__(temperature, sync_checks)
        self._out_mode = out_mode

    def _launch(self, proj_feat1, proj_feat2, **pairs):
        self._state = F_hip.SupConWeightedState()
        self._taps_cache = None
        self._host_out = None
        stacked = F_hip.stacked_halves(proj_feat1, proj_feat2)
        if stacked is not None:  # the two views are torch.chunk halves of one projection: skip the chunk / cat copies
            proj_feat1, proj_feat2 = stacked, None
        loss = F_hip.supcon_weighted_loss(proj_feat1, proj_feat2, in_mode=not self._out_mode, t=self._t, state=self._state,
                                          **pairs)
        if self.sync_checks and not _capturing():
            self.check()  # unit-norm assertion (:49,144,220) and NaN guard of this call, one readback
        return loss

    def forward(self, proj_feat1, proj_feat2, target=None, mask: Tensor = None):
        assert proj_feat1.shape == proj_feat2.shape, (proj_feat1.shape, proj_feat2.shape)  # :50
        if (target is not None) and (mask is not None):  # :52-53
            raise RuntimeError("`target` and `mask` should not be provided in the same time")
        batch_size = len(proj_feat1)
        dev = proj_feat2.device
        if mask is not None:  # :62-66: == 1 positive, == 0 negative, anything else in neither sum
            m = _block(mask, batch_size, dev)
            return self._launch(proj_feat1, proj_feat2, w11=m, w22=m, w12=m, mask_semantics=True)
        if target is not None:  # :68-75
            if isinstance(target, Tensor):
                labels = target.detach().to(device=dev, dtype=torch.float32).contiguous()
            else:
                labels = torch.tensor(list(target), dtype=torch.float32, device=dev)
            assert labels.numel() == batch_size, (labels.shape, batch_size)
            return self._launch(proj_feat1, proj_feat2, labels=labels.reshape(batch_size))
        return self._launch(proj_feat1, proj_feat2, labels=_simclr_labels(batch_size, dev))  # :76-80

    # ---- hook taps, with the values the reference stores before it removes the diagonal (:83-86,159-161,247-250) ----
    def _tap(self, name):
        if self._state is None:
            raise AttributeError(name)
        if self._taps_cache is None:
            taps = F_hip.supcon_weighted_materialize(self._state)
            taps["pos_mask"] = taps["pos_weight"]
            taps["neg_mask"] = taps["enable_mask"] - taps["pos_weight"]
            self._taps_cache = taps
        return self._taps_cache[name]

    @contextmanager
    def register_writer(self, writer=None, epoch=0, extra_tag=None):  # :106-127 (the figures: out of scope)
        yield


class SupConLoss3(SupConLoss2):
    """contrast_loss.py:130-204: softened supervised contrastive loss."""

    def forward(self, proj_feat1, proj_feat2, pos_weight: Tensor = None, **kwargs):
        assert proj_feat1.shape == proj_feat2.shape, (proj_feat1.shape, proj_feat2.shape)  # :145
        assert pos_weight is not None  # :147
        w = _block(pos_weight, len(proj_feat1), proj_feat2.device)  # :150; .repeat(2, 2) (:152) is done by indexing
        return self._launch(proj_feat1, proj_feat2, w11=w, w22=w, w12=w)

    pos_weight = property(lambda self: self._tap("pos_weight"))


class SupConLoss4(SupConLoss2):
    """contrast_loss.py:207-299: one weight matrix per block of the [2n, 2n] pair matrix."""

    def forward(self, *, proj_feat1, proj_feat2, one2one_weight: Tensor = None, two2two_weight: Tensor,  # noqa
                one2two_weight=None, **kwargs):  # noqa
        assert proj_feat1.shape == proj_feat2.shape, (proj_feat1.shape, proj_feat2.shape)  # :221
        assert one2one_weight is not None or one2two_weight is not None or two2two_weight is not None  # :222
        batch_size = len(proj_feat1)
        dev = proj_feat2.device
        w11 = w22 = w12 = None
        if one2two_weight is not None:  # :227-229 -- block (1,1) is installed only beside one2two_weight
            if one2one_weight is None:
                raise TypeError("can't assign a NoneType to a torch.FloatTensor")  # (what :228 raises)
            w11 = _block(one2one_weight, batch_size, dev)
            w12 = _block(one2two_weight, batch_size, dev)  # :233-237: blocks (1,2) AND (2,1), not transposed
        if two2two_weight is not None:  # :230-232
            w22 = _block(two2two_weight, batch_size, dev)
        return self._launch(proj_feat1, proj_feat2, w11=w11, w22=w22, w12=w12)

    pos_weight = property(lambda self: self._tap("pos_weight"))
    enable_mask = property(lambda self: self._tap("enable_mask"))
