"""GPU: the boundary criterion through the epochers (``semi_seg.epochers.helper.supervised_loss`` / ``begin_epoch``).

A ``FineTuneEpocher`` step (eager and replayed from its hipGraph, the same bits), a semi-supervised step and an ``EvalEpocher``
pass run with ``SupCriterion: {name: boundary}`` and report a finite loss and Dice; the epocher's ``cur_epoch`` has reached
the criterion's device scalar; the fine-tune loss is the float64 oracle's on the model's own logits.  With ``KL_div`` the
epochers give the bits they give when ``begin_epoch`` does nothing, and never look ``set_epoch`` up on the criterion."""
import math

import pytest
import torch

from tests import _boundary_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONFIG = {"SupCriterion": {"name": "boundary", "alpha": 0.02, "alpha_step": 0.03, "alpha_max": 0.5, "dice_weight": 0.7,
                           "kl_weight": 1.3, "include_background": False, "per_sample": True}}
EPOCH = 6
ALPHA = 0.02 + 0.03 * (EPOCH - 1)


def _unet(seed=4, cmax=128):
    from spcl_amd.semi_seg.arch import UNet
    torch.manual_seed(seed)
    net = UNet(input_dim=1, num_classes=4, max_channel=cmax).to(DEV)
    net.set_compute_dtype(torch.float32)
    return net.train()


def _batch(n, size, seed):
    g = torch.Generator().manual_seed(seed)
    img, img_tf = torch.rand(n, 1, size, size, generator=g), torch.rand(n, 1, size, size, generator=g)
    tgt = torch.zeros(n, 1, size, size, dtype=torch.long)
    for k in range(n):  # rectangles of the foreground classes: distances of several pixels
        for c in (1, 2, 3):
            y, x = torch.randint(0, size - 8, (2,), generator=g).tolist()
            tgt[k, 0, y:y + 4 + 2 * c, x:x + 9 - 2 * c] = c
    names = [f"patient{k:03d}_00_{k}" for k in range(n)]
    return (img.to(DEV), img_tf.to(DEV), tgt.to(DEV), tgt.clone().to(DEV)), names, (["0"] * n, names)


def _criterion():
    from spcl_amd.contrastyou.losses import build_sup_criterion
    return build_sup_criterion(CONFIG)


def _alpha_on_device(crit):
    (t,) = crit._alpha_on.values()
    return float(t)


def test_finetune_step_replays_bit_for_bit_and_matches_the_oracle():
    from spcl_amd import ddp
    from spcl_amd.contrastyou.losses import BoundaryLoss
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
        net, crit = _unet(), _criterion()
        assert type(crit) is BoundaryLoss and crit.alpha == 0.02
        flat = ddp.FlatParams([p for p in net.parameters() if p.requires_grad])
        opt = FusedRAdam([flat.param], lr=1e-3, weight_decay=1e-5)
        ep = Spy(model=net, optimizer=opt, labeled_loader=iter([]), sup_criterion=crit, num_batches=steps, cur_epoch=EPOCH,
                 device="cuda", flat_params=flat, graph=graph)
        assert abs(crit.alpha - ALPHA) < 1e-12  # (the epocher told the criterion its epoch)
        if not graph:
            ep.seen = []
        curve = []
        with ep.meters.focus_on(ep.meter_focus):
            for b in batches:
                curve.append(float(ep.step(b).detach()))
        assert _alpha_on_device(crit) == float(torch.tensor(ALPHA, dtype=torch.float32))
        stats = ep.meters.statistics()["semi"]
        assert all(math.isfinite(v) for v in curve) and math.isfinite(stats["sup_loss"]["mean"]) and "sup_dice" in stats
        assert all(math.isfinite(v) for v in stats["sup_dice"].values())
        if graph:
            assert ep._step_graph.captured and not ep._step_graph.failed and ep._step_graph.replays == steps - 2
        else:
            for loss, logits, b in zip(curve, ep.seen, batches):
                ref, l_region, _, a = O.boundary_loss(logits.float().cpu(), b[0][2].squeeze(1).cpu(), alpha=ALPHA,
                                                      dice_weight=0.7, kl_weight=1.3, include_background=False,
                                                      per_sample=True)
                assert abs(loss - float(ref)) <= 1e-5 * (abs(float(l_region)) + ALPHA * float(a)), (loss, float(ref))
        res[graph] = (curve, flat.data.clone(), stats)
    assert res[False][0] == res[True][0] and len(set(res[False][0])) == steps
    assert torch.equal(res[False][1], res[True][1])
    assert res[False][2]["sup_dice"] == res[True][2]["sup_dice"]


def test_semi_supervised_step_runs_with_it():
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.epochers.semi import SemiSupervisedEpocher
    lab, unl = _batch(2, 32, 1), _batch(2, 32, 2)
    net, crit = _unet(), _criterion()
    (hook,) = create_hook_from_config(net, {"Data": {"name": "acdc"}, "Trainer": {"max_epoch": 2},
                                            "EntropyMinParameters": {"weight": 0.3}})
    ep = SemiSupervisedEpocher(model=net, optimizer=torch.optim.SGD(net.parameters(), lr=0.0), labeled_loader=[],
                               unlabeled_loader=[], sup_criterion=crit, num_batches=1, cur_epoch=EPOCH, device=DEV)
    ep.add_hooks([hook.to(DEV)()])
    with ep.meters.focus_on(ep.meter_focus):
        sup, _ = ep.step(lab, unl, seed=7)
    stats = ep.meters.statistics()[ep.meter_focus]
    assert sup.requires_grad and math.isfinite(float(sup))
    assert abs(stats["sup_loss"]["mean"] - float(sup)) <= 1e-6 * abs(float(sup))
    assert abs(crit.alpha - ALPHA) < 1e-12 and _alpha_on_device(crit) == float(torch.tensor(ALPHA, dtype=torch.float32))
    l_kl, l_dice, l_b = (float(v) for v in crit.last_parts)
    assert abs(0.7 * l_dice + 1.3 * l_kl + ALPHA * l_b - float(sup)) <= 1e-5 * (abs(float(sup)) + ALPHA * abs(l_b))
    assert l_b != 0.0 and tuple(crit.last_counts[0].shape) == (2, 4) and "sup_dice" in stats
    assert all(math.isfinite(v) for v in stats["sup_dice"].values())


class _Loader:
    def __init__(self, items):
        self.items = items

    def __len__(self):
        return len(self.items)

    def __iter__(self):
        return iter(self.items)


def test_eval_pass_reports_a_finite_loss_and_dice():
    from spcl_amd.semi_seg.epochers import EvalEpocher
    items = []
    for i in range(3):
        (img, _, tgt, _), _, _ = _batch(2, 32, 50 + i)
        items.append(((img, tgt), [f"scan{i:02d}_{k:02d}" for k in range(2)], ([0] * 2, [f"scan{i:02d}"] * 2)))
    net, crit = _unet().eval(), _criterion()
    crit.set_epoch(EPOCH)
    for graph in (False, True):
        stats = EvalEpocher(model=net, loader=_Loader(items), sup_criterion=crit, cur_epoch=EPOCH, device="cuda",
                            graph=graph).run()["eval"]
        assert math.isfinite(stats["loss"]["mean"])
        assert all(math.isfinite(v) for v in stats["dice"].values())
    with torch.no_grad():
        want = sum(float(crit.from_logits(net(img), tgt.squeeze(1))) for (img, tgt), _, _ in items) / len(items)
    assert abs(stats["loss"]["mean"] - want) <= 1e-5 * abs(want)
    assert abs(crit.alpha - ALPHA) < 1e-12  # (an evaluation changes no schedule)


def test_kl_div_keeps_its_bits_and_is_never_asked_for_set_epoch(monkeypatch):
    from spcl_amd import ddp
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.optim import FusedRAdam
    from spcl_amd.semi_seg.epochers import FineTuneEpocher
    from spcl_amd.semi_seg.epochers import finetune as ft_mod
    from spcl_amd.semi_seg.epochers import semi as semi_mod
    from spcl_amd.semi_seg.epochers.semi import SemiSupervisedEpocher
    from spcl_amd.hook_creator import create_hook_from_config

    class Recording(KL_div):
        def __init__(self):
            super().__init__(verbose=False)
            object.__setattr__(self, "asked", [])

        def __getattr__(self, name):  # (reached only for names the normal lookup does not find)
            self.asked.append(name)
            return super().__getattr__(name)

    batches = [_batch(3, 32, 30 + k) for k in range(3)]
    lab, unl = _batch(2, 32, 1), _batch(2, 32, 2)

    def run(crit):
        net = _unet()
        flat = ddp.FlatParams([p for p in net.parameters() if p.requires_grad])
        opt = FusedRAdam([flat.param], lr=1e-3, weight_decay=1e-5)
        ep = FineTuneEpocher(model=net, optimizer=opt, labeled_loader=iter([]), sup_criterion=crit, num_batches=3,
                             cur_epoch=EPOCH, device="cuda", flat_params=flat, graph=False)
        with ep.meters.focus_on(ep.meter_focus):
            curve = [float(ep.step(b).detach()) for b in batches]
        net2 = _unet(seed=5)
        (hook,) = create_hook_from_config(net2, {"Data": {"name": "acdc"}, "Trainer": {"max_epoch": 2},
                                                 "EntropyMinParameters": {"weight": 0.3}})
        sp = SemiSupervisedEpocher(model=net2, optimizer=torch.optim.SGD(net2.parameters(), lr=0.1), labeled_loader=[],
                                   unlabeled_loader=[], sup_criterion=crit, num_batches=1, cur_epoch=EPOCH, device=DEV)
        sp.add_hooks([hook.to(DEV)()])
        with sp.meters.focus_on(sp.meter_focus):
            sup, _ = sp.step(lab, unl, seed=7)
        return curve, flat.data.clone(), sup.detach().clone(), torch.cat([p.detach().flatten() for p in net2.parameters()])

    rec = Recording()
    here = run(rec)
    assert "set_epoch" not in rec.asked, rec.asked
    assert not hasattr(type(rec), "set_epoch")
    monkeypatch.setattr(ft_mod, "begin_epoch", lambda criterion, cur_epoch: None)
    monkeypatch.setattr(semi_mod, "begin_epoch", lambda criterion, cur_epoch: None)
    without = run(KL_div(verbose=False))
    assert here[0] == without[0] and torch.equal(here[1], without[1])
    assert torch.equal(here[2], without[2]) and torch.equal(here[3], without[3])
