"""TEST INFRASTRUCTURE: the eval-mode UNet in float64, stage by stage, on weights whose running statistics are REAL.

``O.init_unet_state`` leaves ``running_mean = 0`` and ``running_var = 1`` with every gamma in [0.9, 1.1]: on such a state a
wrong ``shift``, a wrong ``invstd`` under a small variance or a sign mistake under a negative gamma moves an eval-mode
output by less than any tolerance.  ``eval_state`` makes the statistics those of the weights themselves (one train-mode
oracle pass with momentum 1 over a calibration batch), spreads gamma over +-[0.5, 1.5], and plants the two cases where one
term decides alone: ``running_var = 0`` (``eps`` is all there is under the root) and ``running_mean = 50``.

``stage_oracle`` is ``O.unet_forward(train=False)`` cut into its ten stages, so that one stage can be computed from GIVEN
inputs -- the device's own outputs of the stages before it (teacher forcing: the only usable bar in bf16, where one value
rounded the other way cascades through everything behind it)."""
from functools import lru_cache

import torch
import torch.nn.functional as F

from oracle import spcl_oracle as O

STAGES = O.ENCODER_NAMES + O.DECODER_BLOCKS + ("Deconv_1x1",)
_SKIP = {"Up_conv5": "Conv4", "Up_conv4": "Conv3", "Up_conv3": "Conv2", "Up_conv2": "Conv1"}
MARGIN = 2e-4        # a pixel whose float64 top-2 margin is below MARGIN * max|logits| may flip its arg-max in float32
MARGIN_SHARE = 0.01  # ... and at most this share of the pixels may be such


def until_of(stage):
    """what ``UNet.forward(until=)`` takes for this stage (``None``: the logits)"""
    return None if stage == "Deconv_1x1" else stage


def _bn_prefixes(sd):
    return [k[:-len(".running_mean")] for k in sd if k.endswith(".running_mean")]


def eval_state(max_channel, seed, input_dim=1, hw=(32, 32), num_classes=4, encoder_only=False):
    """-> state dict in float64 whose every value is float32-representable (the device and the oracle hold the same numbers).
    ``hw``: the size of the 4-image calibration batch, the size the test then runs at.  ``encoder_only``: the five encoder
    blocks alone (sizes whose odd halves the decoder could not concatenate)."""
    g = torch.Generator().manual_seed(100003 * seed + 17)
    sd = O.init_unet_state(input_dim, num_classes, max_channel, seed=seed, encoder_only=encoder_only, dtype=torch.float64)
    for p in _bn_prefixes(sd):
        w = sd[p + ".weight"]
        w *= 0.5 + torch.rand(w.shape, generator=g, dtype=torch.float64)
        w[::5] *= -1.0
        sd[p + ".bias"] = 0.3 * torch.randn(w.shape, generator=g, dtype=torch.float64)
    calib = torch.rand(4, input_dim, *hw, generator=g, dtype=torch.float64)
    with torch.no_grad():
        # running statistics := this batch's statistics
        O.unet_forward(calib, sd, "Conv5" if encoder_only else None, train=True, momentum=1.0)
    eps = 1e-5
    for p in ("_Conv3.conv.1",) if encoder_only else ("_Conv3.conv.1", "_Up3.up.2"):
        # eps alone decides: invstd = 1 / sqrt(eps) = 316.  gamma shrinks by what invstd grew, so that the channel's scale stays
        # what it was: left at 316 x, this one channel would be max|.| of every later stage and every figure relative to that
        # maximum (the error bars, the arg-max margin) would speak about it alone
        sd[p + ".weight"][1] *= (eps / (sd[p + ".running_var"][1] + eps)).sqrt()
        sd[p + ".running_var"][1] = 0.0
        sd[p + ".running_mean"][2] = 50.0   # shift = beta - 50 scale: the mean term alone decides (gamma > 0: a dead channel)
    return {k: (v.float().double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}


def stage_inputs(stage, x, outs):
    """the tensors ``stage`` reads, from the image and the outputs of the stages before it"""
    i = STAGES.index(stage)
    if i == 0:
        return (x,)
    if stage in _SKIP:
        return (outs[STAGES[i - 1]], outs[_SKIP[stage]])
    return (outs[STAGES[i - 1]],)


def stage_oracle(name, inputs, sd, q=None):
    """one stage of ``O.unet_forward(train=False)`` from ``inputs`` (``stage_inputs``): an encoder stage is an optional
    max_pool2d then ``_conv_block``; a decoder stage ``_up_conv`` -> cat((skip, up)) -> ``_conv_block``; then the 1x1 head.
    ``q = O.BF16Emulation``: the bf16 mode's storage roundings."""
    if name in O.ENCODER_NAMES:
        (e,) = inputs
        if name == "Conv1":
            e = q.input(e) if q else e
        else:
            e = F.max_pool2d(e, 2, 2)
        return O._conv_block(e, sd, f"_{name}", False, 0.1, q=q)
    if name in O.DECODER_BLOCKS:
        d, skip = inputs
        lvl = name[-1]
        d = O._up_conv(d, sd, f"_Up{lvl}", False, 0.1, q=q)
        return O._conv_block(torch.cat((skip, d), 1), sd, f"_Up_conv{lvl}", False, 0.1, q=q)
    assert name == "Deconv_1x1", name
    (d,) = inputs
    return F.conv2d(d, sd["_Deconv_1x1.weight"], sd["_Deconv_1x1.bias"])


def chain(x, sd, q=None, stages=STAGES):
    """every stage from ``x`` on, each fed by the oracle's own outputs -> {stage: output}"""
    outs = {}
    with torch.no_grad():
        for s in stages:
            outs[s] = stage_oracle(s, stage_inputs(s, x, outs), sd, q=q)
    return outs


def as_dtype(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in sd.items()}


def relmax(a, b):
    """max|a - b| / max|b| in float64"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def low_margin(logits64):
    """[N, H, W] bool: the pixels whose float64 top-2 logit margin is below MARGIN * max|logits|"""
    top = logits64.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) < MARGIN * logits64.abs().max()


def case_seed(N, H, W, max_channel, input_dim=1):
    return 7 * H + 3 * W + N + max_channel + 1000 * input_dim


@lru_cache(maxsize=None)
def case(N, H, W, max_channel, input_dim=1, encoder_only=False, variant=0):
    """the shared reference of one shape, computed once and never modified: image (float32 values in float64), state, the
    float64 oracle's stage outputs and, per stage, the float32 oracle's max-error against them (the yardstick of the
    float32 device pass: what float32 arithmetic in another summation order costs on these very numbers)."""
    seed = case_seed(N, H, W, max_channel, input_dim) + 10007 * variant
    sd = eval_state(max_channel, seed, input_dim, (H, W), encoder_only=encoder_only)
    x = torch.rand(N, input_dim, H, W, generator=torch.Generator().manual_seed(seed + 1)).double()
    stages = O.ENCODER_NAMES if encoder_only else STAGES
    f64 = chain(x, sd, stages=stages)
    f32 = chain(x.float(), as_dtype(sd, torch.float32), stages=stages)
    return {"x": x, "sd": sd, "f64": f64, "f32": f32, "f32_err": {s: relmax(f32[s], f64[s]) for s in stages}}


def _plain_bn(x, sd, p, eps=1e-5):
    """eval-mode BatchNorm written out: every operation, autograd's sums for dgamma / dbeta included, in the tensors' own
    dtype.  (``F.batch_norm`` on the CPU accumulates those sums in double even for float32 tensors: a float32 run through it
    says nothing about what float32 SUMS cost.)"""
    scale = sd[p + ".weight"] / torch.sqrt(sd[p + ".running_var"] + eps)
    return (x - sd[p + ".running_mean"].view(1, -1, 1, 1)) * scale.view(1, -1, 1, 1) + sd[p + ".bias"].view(1, -1, 1, 1)


def _forward_plain(x, sd):
    """``O.unet_forward(x, sd, None, train=False)`` with ``_plain_bn``"""
    def block(e, p):
        for ci, bi in ((0, 1), (3, 4)):
            e = F.relu(_plain_bn(F.conv2d(e, sd[f"{p}.conv.{ci}.weight"], None, 1, 1), sd, f"{p}.conv.{bi}"))
        return e

    feats, e = {}, x
    for k, name in enumerate(O.ENCODER_NAMES):
        e = block(F.max_pool2d(e, 2, 2) if k else e, f"_{name}")
        feats[name] = e
    for lvl, skip in ((5, "Conv4"), (4, "Conv3"), (3, "Conv2"), (2, "Conv1")):
        up = F.conv2d(F.interpolate(e, scale_factor=2, mode="nearest"), sd[f"_Up{lvl}.up.1.weight"], None, 1, 1)
        up = F.relu(_plain_bn(up, sd, f"_Up{lvl}.up.2"))
        e = block(torch.cat((feats[skip], up), 1), f"_Up_conv{lvl}")
    return F.conv2d(e, sd["_Deconv_1x1.weight"], sd["_Deconv_1x1.bias"])


def _oracle_grads(c, labels, dtype, plain=False):
    sd = as_dtype({k: v.clone() for k, v in c["sd"].items()}, dtype)  # (copies: the shared case stays as it is)
    for k, v in sd.items():
        if v.is_floating_point() and "running" not in k:
            v.requires_grad_(True)
    x = c["x"].clone().to(dtype)
    logits = _forward_plain(x, sd) if plain else O.unet_forward(x, sd, None, train=False)
    loss = O.finetune_loss(logits, labels)
    loss.backward()
    return float(loss.detach()), {k: v.grad.double() for k, v in sd.items() if v.requires_grad}


GRAD_F32_BAR = 2e-4  # a gradient case is one on which float32 arithmetic takes every ReLU gate the way float64 does: see below
# the variant of each gradient shape and the number of probes it was clean under where it was chosen (``grad_variant_is_clean``;
# float32 convolutions differ between CPUs, so this is a choice made once, not a property every machine reproduces).
# (3, 48, 32): the first of 2, 5, 7, 8 that are clean under 6 probes.  (2, 64, 64) at max_channel 256: NO variant below 40 is
# clean under 6 probes -- 256-channel sums over 4 x 4 maps always leave some pre-activation inside float32 noise -- so this
# is the first one clean under both float32 oracles alone.  If that case ever fails with ~1e-3 on every tensor in front of
# one layer while the small shape passes, a gate went the other way: compare the two f32 product modes before suspecting a
# kernel (on an MI355X the default split-product mode takes every gate of it, the exact-f32 mode flips one).
GRAD_VARIANT = {(3, 48, 32, 128): (2, 6), (2, 64, 64, 256): (4, 0)}


def _grad_inputs(N, H, W, max_channel, variant):
    c = case(N, H, W, max_channel, variant=variant)
    seed = case_seed(N, H, W, max_channel) + 10007 * variant + 2
    return c, torch.randint(0, 4, (N, H, W), generator=torch.Generator().manual_seed(seed))


def grad_variant_is_clean(N, H, W, max_channel, variant, probes=3):
    """A frozen-statistics network is piecewise linear: a pre-activation within rounding noise of 0 takes its ReLU gate either
    way, and ONE gate taken the other way in a 4 x 4 map moves the weight gradients by 1e-3 .. 1e-2 of their maximum in
    float32 arithmetic that is otherwise right (either float32 oracle does it on most draws of (2, 64, 64), max_channel 256).
    Such a draw says nothing about a kernel.  A variant is clean when float32 arithmetic keeps every tensor within
    GRAD_F32_BAR of float64 in ``2 + probes`` forms: the two float32 oracles of ``grad_case``, and the second one on the
    image moved by 2e-7 of itself (``probes`` draws: other roundings everywhere, the same gradient to 1e-6).  A property of
    the inputs, decided without the device."""
    c, labels = _grad_inputs(N, H, W, max_channel, variant)
    grads = _oracle_grads(c, labels, torch.float64)[1]
    g = torch.Generator().manual_seed(variant + 5)
    for k in range(2 + probes):
        moved = c if k < 2 else dict(c, x=(c["x"] * (1 + 2e-7 * torch.randn(c["x"].shape, generator=g, dtype=torch.float64))))
        got = _oracle_grads(moved, labels, torch.float32, plain=k > 0)[1]
        if max(relmax(got[n], grads[n]) for n in grads) > GRAD_F32_BAR:
            return False
    return True


@lru_cache(maxsize=None)
def grad_case(N, H, W, max_channel):
    """``case`` under grad (variant GRAD_VARIANT[shape]): labels, the fine-tune loss of the eval-mode pass (train=False: frozen
    statistics), its gradient w.r.t. every parameter in float64, and per parameter the float32 oracle's own error
    max|diff| / max|ref| -- the larger of two float32 runs of the oracle: through ``F.batch_norm`` (which sums dgamma / dbeta
    in double) and with the BatchNorm written out (``_plain_bn``: float32 sums).  The second matters where a sum cancels:
    the gamma gradient of the running_var = 0 channel is 9e-5 off in plain float32 and 3e-6 with double accumulators."""
    variant = GRAD_VARIANT[(N, H, W, max_channel)][0]
    c, labels = _grad_inputs(N, H, W, max_channel, variant)
    loss, grads = _oracle_grads(c, labels, torch.float64)
    runs = [_oracle_grads(c, labels, torch.float32, plain)[1] for plain in (False, True)]
    return {"case": c, "variant": variant, "labels": labels, "loss": loss, "grads": grads,
            "f32_err": {k: max(relmax(r[k], grads[k]) for r in runs) for k in grads}}


def load_unet(sd, max_channel, dtype, input_dim=1, num_classes=4):
    """the HIP UNet holding ``sd`` (exactly: its values are float32; an encoder-only state leaves the decoder as constructed),
    in eval mode on the GPU"""
    import spcl_amd  # noqa: F401
    from spcl_amd.semi_seg.arch import UNet
    m = UNet(input_dim=input_dim, num_classes=num_classes, max_channel=max_channel)
    missing = m.load_state_dict(as_dtype(sd, torch.float32), strict="_Deconv_1x1.weight" in sd)
    assert not missing.unexpected_keys and all(not k.startswith("_Conv") for k in missing.missing_keys)
    m.cuda().eval()
    m.set_compute_dtype(dtype)
    return m
