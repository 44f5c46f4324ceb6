#!/usr/bin/env python3
"""Write tests/golden/g15_iic_estimator.npz from the REFERENCE's ``ClusterHead`` / ``DenseClusterHead``
(contrastyou/projectors/heads.py), ``IIDLoss`` / ``IIDSegmentationSmallPathLoss`` (contrastyou/losses/iic_loss.py) and
``IICEstimator.forward`` (semi_seg/mi_estimator/discrete_mi_estimator.py).

    python tools/gen_golden_iic_estimator.py --reference <checkout of the reference>

The three files are loaded by path.  What they import beyond torch is stubbed: ``loguru.logger``, ``termcolor.colored``,
``deepclustering2.utils.simplex``, ``deepclustering2.configparser._utils.get_config``, ``torch._six.container_abcs``,
``contrastyou.utils.average_iter`` / ``_pair``, and, around the estimator, ``.base`` (``SingleEstimator`` / ``EstimatorList``
as bare ``nn.Module``s), ``..arch.unet.get_channel_dim`` (the channel count of the case) and ``..utils`` (the ``IIDLoss``
wrapper of semi_seg/utils.py:210-213, which returns the first element, restated in four lines; the names the file imports
and does not use here are placeholders).  The class bodies -- plain torch -- are what runs.

Only data is written.  Heads: per case the seeded feature, the state dict with its key list, the S probability maps, and for
an upstream gradient on the maps the gradient of the feature (the parameters' gradients are recorded with the estimator cases:
with them for every head case the file would pass the size limit for a committed file).  Estimator: per case the two features
(``forward(feat_tf, flip(feat))`` of semi_seg/epochers/_mixins.py:86, the flip applied here), the flags, the state dict, the
float32 loss and its gradients.  ``SoftmaxWithT`` divides in place, so every call gets clones.  No test reads the reference;
they read this file."""
import argparse
import collections.abc
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import _iic_estimator_oracle as E  # noqa: E402
from tests import _iic_oracle as R  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "g15_iic_estimator.npz")
S, K, C = 3, 5, 16
CHANNELS = {}


def _module(name, **attrs):
    m = sys.modules.get(name) or types.ModuleType(name)
    m.__dict__.update(attrs)
    if not hasattr(m, "__path__"):
        m.__path__ = []
    sys.modules[name] = m
    return m


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference(root):
    class _Logger:
        def __getattr__(self, _):
            return lambda *a, **k: None

    def simplex(t, axis=1):
        s = t.sum(axis)
        return bool(torch.allclose(s, torch.ones_like(s), atol=1e-4))

    def average_iter(a_list):
        return sum(a_list) / float(len(a_list))

    _module("loguru", logger=_Logger())
    _module("termcolor", colored=lambda s, *a, **k: s)
    _module("deepclustering2")
    _module("deepclustering2.utils", simplex=simplex)
    _module("deepclustering2.configparser")
    _module("deepclustering2.configparser._utils", get_config=lambda scope="base": {"Arch": {}})
    if "torch._six" not in sys.modules:
        _module("torch._six", container_abcs=collections.abc)
    _module("contrastyou")
    _module("contrastyou.utils", average_iter=average_iter)
    _module("contrastyou.utils.utils", _pair=nn.modules.utils._pair)
    _module("contrastyou.projectors")
    _load("contrastyou.projectors.nn", os.path.join(root, "contrastyou", "projectors", "nn.py"))
    heads = _load("contrastyou.projectors.heads", os.path.join(root, "contrastyou", "projectors", "heads.py"))
    _module("contrastyou.losses")
    losses = _load("contrastyou.losses.iic_loss", os.path.join(root, "contrastyou", "losses", "iic_loss.py"))

    class SingleEstimator(nn.Module):
        pass

    class EstimatorList(nn.Module):
        def __init__(self):
            super().__init__()
            self._estimator_dictionary = nn.ModuleDict()

    class IIDLoss(losses.IIDLoss):  # semi_seg/utils.py:210-213
        def forward(self, x_out, x_tf_out):
            return super().forward(x_out, x_tf_out)[0]

    _module("_ref_semi_seg")
    _module("_ref_semi_seg.mi_estimator")
    _module("_ref_semi_seg.mi_estimator.base", SingleEstimator=SingleEstimator, EstimatorList=EstimatorList,
            encoder_names=["Conv1", "Conv2", "Conv3", "Conv4", "Conv5"])
    _module("_ref_semi_seg.arch")
    _module("_ref_semi_seg.arch.unet", get_channel_dim=lambda name, max_channel=None: CHANNELS[name])
    _module("_ref_semi_seg.utils", IIDLoss=IIDLoss, IIDSegmentationSmallPathLoss=losses.IIDSegmentationSmallPathLoss,
            _nlist=None, _filter_encodernames=None, _filter_decodernames=None)
    est = _load("_ref_semi_seg.mi_estimator.discrete_mi_estimator",
                os.path.join(root, "semi_seg", "mi_estimator", "discrete_mi_estimator.py"))
    return heads, est


def head_cases():
    return [(dense, ht, nz, T) for dense in (False, True) for ht in ("linear", "mlp") for nz in (False, True) for T in (1.0, 0.5)]


def head_key(dense, ht, nz, T):
    return f"head/{'dense' if dense else 'encoder'}_{ht}_n{int(nz)}_t{T}"


def estimator_cases():
    return [(layer, shape, ht, nz, T) for layer, shape in (("Conv5", (3, 16, 4, 4)), ("Up_conv3", (3, 8, 12, 10)))
            for ht in ("linear", "mlp") for nz, T in ((False, 1.0), (True, 0.5))]


def estimator_key(layer, shape, ht, nz, T):
    return f"estimator/{layer}_{ht}_n{int(nz)}_t{T}"


FLAGS = [1, 2, 3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    heads, est_mod = load_reference(args.reference)
    out, worst = {}, 0.0
    for idx, case in enumerate(head_cases()):
        dense, ht, nz, T = case
        key = head_key(*case)
        torch.manual_seed(300 + idx)
        cls = heads.DenseClusterHead if dense else heads.ClusterHead
        head = cls(input_dim=C, num_clusters=K, num_subheads=S, head_type=ht, T=T, normalize=nz)
        g = torch.Generator().manual_seed(400 + idx)
        feat = torch.randn(4, C, 6, 5, generator=g)
        x = feat.clone().requires_grad_(True)
        probs = torch.stack([p.clone() for p in head(x)], 0)
        up = torch.randn(probs.shape, generator=g)
        (probs * up).sum().backward()
        out[key + "/feat"], out[key + "/up"] = feat.numpy(), up.numpy()
        out[key + "/probs"], out[key + "/dfeat"] = probs.detach().numpy(), x.grad.numpy()
        out[key + "/keys"] = np.array(list(head.state_dict()))
        for k, v in head.state_dict().items():
            out[key + "/init/" + k] = v.detach().clone().numpy()
        oracle = E.dense_cluster_head_logits if dense else E.cluster_head_logits
        lg = oracle(feat.double(), {k: v.double() for k, v in head.state_dict().items()}, S, ht, nz, T)
        want = torch.stack([lg[:, s * K:(s + 1) * K].softmax(1) for s in range(S)], 0).reshape(probs.shape)
        err = float((want - probs.detach().double()).abs().max())
        worst = max(worst, err)
        print(f"{key}: probabilities {tuple(probs.shape)}, restatement (float64) vs reference (float32): max abs {err:.2e}")
    for idx, case in enumerate(estimator_cases()):
        layer, shape, ht, nz, T = case
        key = estimator_key(*case)
        CHANNELS[layer] = shape[1]
        torch.manual_seed(500 + idx)
        est = est_mod.IICEstimator()
        est.init_projector(layer_name=layer, head_type=ht, num_subhead=S, num_cluster=K, normalize=nz, temperature=T)
        est.init_criterion(padding=1, patch_size=8)
        g = torch.Generator().manual_seed(600 + idx)
        feat, feat_tf = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
        a, b = feat.clone().requires_grad_(True), feat_tf.clone().requires_grad_(True)
        loss = est(b, R.flip(a, FLAGS))
        loss.backward()
        out[key + "/feat"], out[key + "/feat_tf"] = feat.numpy(), feat_tf.numpy()
        out[key + "/flags"] = np.array(FLAGS, dtype=np.uint8)
        out[key + "/loss"] = loss.detach().numpy()
        out[key + "/dfeat"], out[key + "/dfeat_tf"] = a.grad.numpy(), b.grad.numpy()
        out[key + "/keys"] = np.array(list(est.state_dict()))
        for k, v in est.state_dict().items():
            out[key + "/init/" + k] = v.detach().clone().numpy()
        for k, p in est.named_parameters():
            out[key + "/grad/" + k] = p.grad.numpy()
        print(f"{key}: loss {float(loss.detach()):.9g}")
    out["head_cases"] = np.array([head_key(*c) for c in head_cases()])
    out["estimator_cases"] = np.array([estimator_key(*c) for c in estimator_cases()])
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(head_cases())} + {len(estimator_cases())} cases, {os.path.getsize(OUT)} bytes; worst head gap {worst:.2e}")


if __name__ == "__main__":
    main()
