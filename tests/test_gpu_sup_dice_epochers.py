"""GPU: the soft-Dice / class-weighted criteria through the epochers (``semi_seg.epochers.helper.supervised_loss``).

``KL_div`` keeps the fused launch and its bits; a ``FineTuneEpocher`` step with ``DiceKLLoss`` replays from its hipGraph to the
bits of the eager step and its loss is the float64 oracle's on the model's own logits (1e-5 relative, the kernel tests' bar);
the semi-supervised, mix-up and adversarial epochers run a step with it; ``EvalEpocher`` and ``InferenceEpocher(tta="flips")``
report finite losses through the generic ``(prob, onehot)`` call; two criteria that differ in one class weight never share a
captured graph."""
import itertools
import math

import pytest
import torch

from tests import _sup_dice_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WEIGHTS = (0.3, 1.0, 2.0, 1.5)
_names = itertools.count()


def _unet(seed=4, cmax=128):
    from spcl_amd.semi_seg.arch import UNet
    torch.manual_seed(seed)
    net = UNet(input_dim=1, num_classes=4, max_channel=cmax).to(DEV)
    net.set_compute_dtype(torch.float32)
    return net.train()


def _batch(n, size, seed):
    g = torch.Generator().manual_seed(seed)
    img, img_tf = torch.rand(n, 1, size, size, generator=g), torch.rand(n, 1, size, size, generator=g)
    tgt = torch.randint(0, 4, (n, 1, size, size), generator=g)
    names = [f"patient{k:03d}_00_{k}" for k in range(n)]
    return (img.to(DEV), img_tf.to(DEV), tgt.to(DEV), tgt.clone().to(DEV)), names, (["0"] * n, names)


def _criterion(**kw):
    from spcl_amd.contrastyou.losses import DiceKLLoss
    args = dict(dice_weight=0.7, kl_weight=1.3, class_weight=WEIGHTS, include_background=False, per_sample=True)
    args.update(kw)
    return DiceKLLoss(**args)


def test_helper_with_kl_div_is_the_fused_launch():
    from spcl_amd import functional as F_hip
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.semi_seg.epochers.helper import supervised_loss
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(3, 4, 19, 23, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    labels = torch.randint(0, 4, (3, 19, 23), generator=g).to(DEV)
    out = []
    for fn in (lambda x: supervised_loss(KL_div(), x, labels, 4), lambda x: F_hip.sup_loss_kl_onehot(x, labels, 1e-16)):
        x = logits.clone().requires_grad_(True)
        loss, (inter, union) = fn(x)
        loss.backward()
        out.append((loss.detach(), x.grad, inter, union))
    assert all(torch.equal(a, b) for a, b in zip(*out))
    # a criterion with from_logits takes its own kernels, anything else the composed path: same value, same counts
    crit = _criterion()
    loss, counts = supervised_loss(crit, logits, labels, 4)
    assert counts is crit.last_counts and torch.equal(counts[0], out[0][2]) and torch.equal(counts[1], out[0][3])

    class Composed(torch.nn.Module):  # (no from_logits: softmax, one-hot, criterion, arg-max, Dice counts)
        def forward(self, prob, onehot, **kw):
            return crit(prob, onehot, **kw)
    loss_c, counts_c = supervised_loss(Composed(), logits, labels, 4)
    assert abs(float(loss_c) - float(loss)) <= 1e-6 * abs(float(loss))
    assert torch.equal(counts_c[0], counts[0]) and torch.equal(counts_c[1], counts[1])


def test_finetune_step_replays_bit_for_bit_and_matches_the_oracle():
    from spcl_amd import ddp
    from spcl_amd.optim import FusedRAdam
    from spcl_amd.semi_seg.epochers import FineTuneEpocher

    class Spy(FineTuneEpocher):
        seen = None

        def _forward_pass(self, image):
            out = super()._forward_pass(image)
            if self.seen is not None:
                self.seen.append(out.detach().clone())
            return out

    steps, bs, size = 4, 3, 32
    batches = [_batch(bs, size, 20 + k) for k in range(steps)]
    res = {}
    for graph in (False, True):
        net = _unet()
        flat = ddp.FlatParams([p for p in net.parameters() if p.requires_grad])
        opt = FusedRAdam([flat.param], lr=1e-3, weight_decay=1e-5)
        ep = Spy(model=net, optimizer=opt, labeled_loader=iter([]), sup_criterion=_criterion(), num_batches=steps,
                 device="cuda", flat_params=flat, graph=graph)
        if not graph:
            ep.seen = []
        curve = []
        with ep.meters.focus_on(ep.meter_focus):
            for b in batches:
                curve.append(float(ep.step(b).detach()))
        if graph:
            assert ep._step_graph.captured and not ep._step_graph.failed and ep._step_graph.replays == steps - 2
        else:
            for loss, logits, b in zip(curve, ep.seen, batches):
                ref, _, _ = O.dice_kl(logits.float().cpu(), b[0][2].squeeze(1).cpu(), dice_weight=0.7, kl_weight=1.3,
                                      class_weight=WEIGHTS, include_background=False, per_sample=True)
                assert abs(loss - float(ref)) <= 1e-5 * abs(float(ref)), (loss, float(ref))
        res[graph] = (curve, flat.data.clone(), ep.meters.statistics()["semi"])
    assert res[False][0] == res[True][0] and len(set(res[False][0])) == steps
    assert torch.equal(res[False][1], res[True][1])
    assert res[False][2]["sup_dice"] == res[True][2]["sup_dice"]


def test_graph_keys_tell_two_class_weights_apart():
    from spcl_amd import ddp
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.optim import FusedRAdam
    from spcl_amd.semi_seg.epochers import FineTuneEpocher
    net = _unet()
    flat = ddp.FlatParams([p for p in net.parameters() if p.requires_grad])
    opt = FusedRAdam([flat.param], lr=1e-3)
    (img, _, tgt, _), _, _ = _batch(2, 16, 1)
    keys = []
    for crit in (_criterion(), _criterion(class_weight=(0.3, 1.0, 2.0, 1.25)), _criterion(), KL_div()):
        ep = FineTuneEpocher(model=net, optimizer=opt, labeled_loader=iter([]), sup_criterion=crit, num_batches=1,
                             device="cuda", flat_params=flat, graph=True)
        keys.append(ep._graph_key(img, tgt))
    assert None not in keys and keys[0] != keys[1] and keys[0] == keys[2] and keys[3] != keys[0]
    assert len(keys[3]) == len(keys[0]) - 1  # (KL_div's key is what it was)


def test_semi_mixup_and_adversarial_epochers_step_with_it():
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.arch.discr import Discriminator
    from spcl_amd.semi_seg.epochers.adversarial import AdversarialEpocher
    from spcl_amd.semi_seg.epochers.mixup import MixUpEpocher
    from spcl_amd.semi_seg.epochers.semi import SemiSupervisedEpocher
    from spcl_amd.semi_seg.hooks.mixup import MixUpHook
    lab, unl = _batch(2, 32, 1), _batch(2, 32, 2)

    def check(ep, crit, sup):
        stats = ep.meters.statistics()[ep.meter_focus]
        assert sup.requires_grad
        sup = sup.detach()
        assert math.isfinite(float(sup)) and float(sup) > 0
        assert abs(stats["sup_loss"]["mean"] - float(sup)) <= 1e-6 * float(sup)
        l_kl, l_dice = (float(v) for v in crit.last_parts)
        assert abs(0.7 * l_dice + 1.3 * l_kl - float(sup)) <= 1e-6 * float(sup) and 0 < l_dice < 1
        assert tuple(crit.last_counts[0].shape) == (2, 4) and "sup_dice" in stats

    net, crit = _unet(), _criterion()
    (hook,) = create_hook_from_config(net, {"Data": {"name": "acdc"}, "Trainer": {"max_epoch": 2},
                                            "EntropyMinParameters": {"weight": 0.3}})
    ep = SemiSupervisedEpocher(model=net, optimizer=torch.optim.SGD(net.parameters(), lr=0.0), labeled_loader=[],
                               unlabeled_loader=[], sup_criterion=crit, num_batches=1, device=DEV)
    ep.add_hooks([hook.to(DEV)()])
    with ep.meters.focus_on(ep.meter_focus):
        sup, _ = ep.step(lab, unl, seed=7)
    check(ep, crit, sup)

    net, crit = _unet(), _criterion()
    ep = MixUpEpocher(model=net, optimizer=torch.optim.SGD(net.parameters(), lr=0.0), labeled_loader=[], unlabeled_loader=None,
                      sup_criterion=crit, num_batches=1, device=DEV)
    ep.add_hooks([MixUpHook(hook_name=f"sup_dice_mx_{next(_names)}", weight=0.1)()])
    ep.init()
    with ep.meters.focus_on(ep.meter_focus):
        sup, _ = ep.step(lab, seed=7)
    check(ep, crit, sup)

    lab, unl = _batch(2, 64, 3), _batch(2, 64, 4)  # (the discriminator's four stride-2 stages need 64 x 64 for its 4 x 4 head)
    net, crit = _unet(), _criterion()
    D = Discriminator(4, 16).to(DEV).train()
    ep = AdversarialEpocher(model=net, optimizer=torch.optim.SGD(net.parameters(), lr=0.0), labeled_loader=[],
                            unlabeled_loader=(), sup_criterion=crit, num_batches=1, device=DEV, discriminator=D,
                            discr_optimizer=torch.optim.SGD(D.parameters(), lr=0.0), reg_weight=0.5, dis_consider_image=False)
    with ep.meters.focus_on(ep.meter_focus):
        sup, _, _ = ep.step(lab, unl)
    check(ep, crit, sup)


class _Loader:
    def __init__(self, items):
        self.items = items

    def __len__(self):
        return len(self.items)

    def __iter__(self):
        return iter(self.items)


def test_eval_and_tta_inference_report_finite_losses(tmp_path):
    from spcl_amd.semi_seg.epochers import EvalEpocher, InferenceEpocher
    items = []
    for i in range(3):
        (img, _, tgt, _), _, _ = _batch(2, 32, 50 + i)
        items.append(((img, tgt), [f"scan{i:02d}_{k:02d}" for k in range(2)], ([0] * 2, [f"scan{i:02d}"] * 2)))
    net, crit = _unet().eval(), _criterion()
    for graph in (False, True):
        stats = EvalEpocher(model=net, loader=_Loader(items), sup_criterion=crit, device="cuda", graph=graph).run()["eval"]
        assert math.isfinite(stats["loss"]["mean"]) and stats["loss"]["mean"] > 0
    # the eval loss is the criterion on the model's logits
    with torch.no_grad():
        want = sum(float(crit.from_logits(net(img), tgt.squeeze(1))) for (img, tgt), _, _ in items) / len(items)
    assert abs(stats["loss"]["mean"] - want) <= 1e-5 * want
    ep = InferenceEpocher(model=net, loader=_Loader(items), sup_criterion=crit, device="cuda", tta="flips")
    ep.init(save_dir=str(tmp_path))
    stats = ep.run()["eval"]
    for name in ("loss", "loss_tta"):
        assert math.isfinite(stats[name]["mean"]) and stats[name]["mean"] > 0, name
