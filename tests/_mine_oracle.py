"""Restatement of the MINE estimator (semi_seg/mi_estimator/mineestimator.py:19-36 behind the call of
semi_seg/epochers/_mixins.py:79-86) in torch.nn.functional on the CPU, in any floating dtype (float64: the reference of the GPU
tests; float32: the yardstick of their tolerance).  A state is a dict with the keys of the reference's ``_projector``
(``0.weight`` ... ``8.bias``); ``estimator_loss`` updates its running statistics in place, as the module would."""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

MOMENTUM, EPS = 0.1, 1e-5
SHAPES = [(1, 16, 5, 7), (3, 16, 5, 7), (3, 8, 9, 6)]  # (n, C, H, W) of tests/golden/g12_mine.npz
FLOOR_CONV, FLOOR_HEAD = 2e-5, 1e-6  # the f32 bars of tests/test_gpu_decoder.py: through convolutions / for the head alone


def rel_l2(a, ref):
    a, ref = a.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float((a - ref).norm() / ref.norm().clamp_min(1e-300))


def bound(f32_value, ref64, floor=FLOOR_CONV):
    """the tolerance of a comparison that goes through products and long sums: 4 x the relative L2 error torch's own float32
    CPU evaluation of the same expression makes on the same inputs (the margin covers another summation order), at least the
    f32 bar ``floor``"""
    return max(4.0 * rel_l2(f32_value, ref64), floor)


def projector(C, dtype=torch.float32):
    """the reference's ``_projector`` (mineestimator.py:19-30), stock modules in the reference's order"""
    return nn.Sequential(
        nn.Conv2d(2 * C, C, 3, 1, 1), nn.BatchNorm2d(C), nn.ReLU(inplace=True),
        nn.Conv2d(C, C // 2, 3, 1, 1), nn.BatchNorm2d(C // 2), nn.ReLU(inplace=True),
        nn.AdaptiveMaxPool2d((1, 1)), nn.Flatten(), nn.Linear(C // 2, 1)).to(dtype)


def init_state(C, seed):
    """the initial state one seed draws (construction order = the reference's)"""
    torch.manual_seed(seed)
    sd = {k: v.clone() for k, v in projector(C).state_dict().items()}
    g = torch.Generator().manual_seed(seed + 1)  # BatchNorm affine and running statistics away from their trivial defaults
    for i in ("1", "4"):
        c = sd[i + ".weight"].numel()
        sd[i + ".weight"] = 1.0 + 0.2 * torch.randn(c, generator=g)
        sd[i + ".bias"] = 0.2 * torch.randn(c, generator=g)
        sd[i + ".running_mean"] = 0.1 * torch.randn(c, generator=g)
        sd[i + ".running_var"] = 1.0 + 0.5 * torch.rand(c, generator=g)
    return sd


def make_inputs(n, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(2 * n, C, H, W, generator=g)
    flags = [(seed + 3 * i) % 4 for i in range(n)]
    return feat, flags


def cast(sd, dtype, requires_grad=False):
    out = {}
    for k, v in sd.items():
        if v.is_floating_point():
            v = v.detach().clone().to(dtype)
            if requires_grad and "running" not in k:
                v.requires_grad_(True)
        else:
            v = v.clone()
        out[k] = v
    return out


def flip(x, flags):
    """per-sample flips: bit 0 flips H, bit 1 flips W"""
    rows = []
    for xi, f in zip(x, flags):
        dims = [d for d, bit in ((1, 1), (2, 2)) if int(f) & bit]
        rows.append(torch.flip(xi, dims) if dims else xi)
    return torch.stack(rows, 0)


def activation(x, sd, training=True):
    """the second layer's ReLU output [n, C/2, H, W] (what the pooling reads)"""
    for conv, bn in (("0", "1"), ("3", "4")):
        x = F.conv2d(x, sd[conv + ".weight"], sd[conv + ".bias"], padding=1)
        x = F.relu(F.batch_norm(x, sd[bn + ".running_mean"], sd[bn + ".running_var"], sd[bn + ".weight"], sd[bn + ".bias"],
                                training, MOMENTUM, EPS))
        if training and (bn + ".num_batches_tracked") in sd:
            sd[bn + ".num_batches_tracked"] += 1
    return x


def head(act, sd):
    """AdaptiveMaxPool2d((1, 1)) -> Flatten -> Linear: the logits [n]"""
    return F.linear(F.adaptive_max_pool2d(act, 1).flatten(1), sd["8.weight"], sd["8.bias"]).reshape(-1)


def pairs(feat, flags):
    """the two inputs of the statistics network from the extracted feature [2n, C, H, W]"""
    n = feat.shape[0] // 2
    feat1, feat2 = feat[n:], flip(feat[:n], flags)
    feat2_prime = torch.cat([feat2[1:], feat2[0:1]], dim=0)
    return torch.cat([feat1, feat2], dim=1), torch.cat([feat1, feat2_prime], dim=1)


def estimator_loss(feat, flags, sd, training=True, taps=None):
    """``Em - Ej`` (mineestimator.py:32-36), joint pass first; ``taps``: a dict that receives the two activations"""
    joint, marg = pairs(feat, flags)
    aj = activation(joint, sd, training)
    am = activation(marg, sd, training)
    if taps is not None:
        taps.update(act_joint=aj, act_marg=am)
    ej = -F.softplus(head(aj, sd)).mean()
    em = F.softplus(head(am, sd)).mean()
    return em - ej


def top2_gap(act):
    """the smallest gap between the two largest POSITIVE activations of any (sample, channel): while it exceeds the rounding
    error of the activation no argmax can differ between two evaluations (a channel with fewer than two positive values has
    its gap measured against 0, the ReLU's floor)"""
    v = act.detach().double().flatten(2)
    if v.shape[2] == 1:
        top = torch.cat([v, torch.zeros_like(v)], 2)
    else:
        top = v.topk(2, dim=2).values
    live = top[..., 0] > 0
    gaps = (top[..., 0] - top[..., 1])[live]
    return float(gaps.min()) if gaps.numel() else float("inf")


def run(feat, flags, sd0, dtype, training=True):
    """one call with backward in ``dtype`` -> dict(loss, dfeat, grads {key: tensor}, state after the call, taps)"""
    sd = cast(sd0, dtype, requires_grad=True)
    x = feat.detach().clone().to(dtype).requires_grad_(True)
    taps = {}
    loss = estimator_loss(x, flags, sd, training, taps)
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sd.items() if v.requires_grad}
    return {"loss": loss.detach(), "dfeat": x.grad, "grads": grads,
            "state": {k: v.detach() for k, v in sd.items()}, "taps": {k: v.detach() for k, v in taps.items()}}


def load_golden(path):
    """-> (case keys, {array name: tensor})"""
    z = np.load(path)
    return [str(c) for c in z["cases"]], {k: torch.from_numpy(z[k]) for k in z.files if k != "cases"}


def composed_on_device(est, feature, flags):
    """``Em - Ej`` of the HIP estimator ``est`` composed from the ops the package had before csrc/mine.hip: ``flip_batch`` and
    torch's ``roll`` / ``cat`` for the inputs, ``conv_bn_relu`` for the layers, ``adaptive_pool2d(., "max")`` and torch's
    ``linear`` / ``softplus`` / ``mean`` for the tail.  Same convolution kernels, same stored activations; what the fused
    path is measured and (in bf16) checked against."""
    from spcl_amd import config
    from spcl_amd import functional as F_hip
    dtype = config.get_compute_dtype()
    n = feature.shape[0] // 2
    feat1 = feature[n:]
    feat2 = F_hip.flip_batch(feature[:n], flags) if flags is not None else feature[:n]
    feat2_prime = torch.roll(feat2, -1, 0)
    layers = (est._layer(0, 1), est._layer(3, 4))
    lin = est._projector[8]
    terms = []
    for second in (feat2, feat2_prime):
        x = torch.cat([feat1, second], dim=1)
        for w, b, gamma, beta, bn in layers:
            x = F_hip._mine_layer(x, w, b, gamma, beta, bn, dtype)
        pooled = F_hip.adaptive_pool2d(x, (1, 1), "max").flatten(1)
        terms.append(F.softplus(F.linear(pooled, lin.weight, lin.bias)).mean())
    return terms[1] + terms[0]
