"""GPU: the MIDL baseline's hook (semi_seg/hooks/midl.py behind ``create_midl_hook``).

One ``SemiSupervisedEpocher.step`` on the small UNet and synthetic batches of tests/test_gpu_semi_reg_hooks.py (64 x 64 maps,
``patch_size`` 40: starts 0, 20, 24 on both axes, 3 x 3 overlapping patches with an irregular last start): ``reg_loss``
against ``consistency_weight * consistency + iic_weight * patch-wise IIC`` in float64 on the step's own logits (a second,
identically initialised model), every parameter's gradient against the pull-back of the float64 d(logits), meter ``iic_mi``
= the unweighted criterion.  Two steps from the same seed and state give the same bits.  The hook called with the reference's
plain keywords (the flipped copy, no flags) gives the loss it gives with the epocher's ``unlabeled_logits`` / ``flip_flags``.
A ``SemiTrainer`` built from ``MIDLPaperParameters`` trains one epoch of two batches, checkpoints and resumes."""
import pytest
import torch

from oracle import spcl_oracle as O
from tests import _iic_oracle as R
from tests import _midl_oracle as M
from tests.test_gpu_semi_reg_hooks import _check_step_grads, _reference_grads, _setup
from tests.test_gpu_semi_step import _batch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MIDL = {"iic_weight": 0.1, "padding": 1, "patch_size": 40, "consistency_weight": 5.0, "name": "mse"}


def _drive(th):
    """the combined epocher hook with one meter interface of its own, handed to each member"""
    from spcl_amd.contrastyou.meters import MeterInterface
    eh = th()
    meters = MeterInterface(default_focus="semi")
    for member in eh._epocher_hook:
        member.meters = meters
        member.configure_meters(meters)
    return eh


def _step(seed=1234):
    sd, model, hook, ep, flat = _setup("MIDLPaperParameters", MIDL)
    lab, unl = _batch(2, 64, 1), _batch(2, 64, 2)
    with ep.meters.focus_on(ep.meter_focus):
        sup, reg = ep.step(lab, unl, seed=seed)
    torch.cuda.synchronize()
    return sd, model, hook, ep, flat, lab, unl, sup, reg


def test_semi_step_with_the_midl_hook_vs_float64():
    from spcl_amd.contrastyou.hooks.base import CombineTrainerHook
    seed = 1234
    sd, model, hook, ep, flat, lab, unl, sup, reg = _step(seed)
    assert isinstance(hook, CombineTrainerHook)
    flags = [int(d[0]) | (int(d[1]) << 1) for d in O.random_flip_decisions(seed, 2)]
    holder = {}

    def dlogits(ul, utl):
        u64 = utl.clone().requires_grad_(True)
        uda = R.consistency(ul, u64, 1.0, flags)
        iic, per_patch = M.loss(u64, ul.detach(), MIDL["padding"], MIDL["patch_size"], flags)
        assert len(per_patch) == 9
        loss = MIDL["consistency_weight"] * uda + MIDL["iic_weight"] * iic
        loss.backward()
        holder.update(reg=float(loss), iic=float(iic), uda=float(uda))
        return 1, u64.grad

    osup, ref_grads = _reference_grads(sd, lab, unl, flags, dlogits)
    print(f"reg_loss {float(reg):.9g} vs {holder['reg']:.9g} (consistency {holder['uda']:.6g}, iic {holder['iic']:.6g})")
    assert abs(float(sup) - osup) <= 1e-4 * abs(osup), (float(sup), osup)
    assert abs(float(reg) - holder["reg"]) <= 1e-4 * abs(holder["reg"]), (float(reg), holder["reg"])
    _check_step_grads(model, flat, ref_grads)
    stats = ep.meters.statistics()
    assert stats["midl"]["iic_mi"]["mean"] == pytest.approx(holder["iic"], rel=1e-4)
    assert stats["consistency"]["loss"]["mean"] == pytest.approx(holder["uda"], rel=1e-4)
    ep.close_hooks()  # (flushes the lagged NaN check: nothing to report)


def test_two_steps_from_the_same_state_give_the_same_bits():
    a, b = _step(), _step()
    assert torch.equal(a[7], b[7]) and torch.equal(a[8], b[8])
    assert torch.equal(a[4].param.detach(), b[4].param.detach())
    for va, vb in zip(a[4].views, b[4].views):
        assert torch.equal(va, vb)


def test_plain_reference_keywords_give_the_same_loss():
    from spcl_amd import functional as F_hip
    from spcl_amd.semi_seg.hooks import create_midl_hook
    hook = create_midl_hook(consistency_weight=5.0, iic_weight=0.1, padding=1, patch_size=8)
    g = torch.Generator().manual_seed(3)
    utl = torch.randn(3, 4, 21, 27, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    ul = torch.randn(3, 4, 21, 27, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    flags = [3, 0, 1]
    fl = torch.tensor(flags, dtype=torch.uint8, device=DEV)
    losses, grads = [], []
    for extra in ({"unlabeled_logits": ul, "flip_flags": fl}, {}):
        eh = _drive(hook)
        x = utl.clone().requires_grad_(True)
        loss = eh(unlabeled_tf_logits=x, unlabeled_logits_tf=F_hip.flip_batch(ul, fl), seed=0, affine_transformer=None, **extra)
        loss.backward()
        losses.append(float(loss))
        grads.append(x.grad.clone())
        eh.close()
    ref = 5.0 * R.consistency(ul.double().cpu(), utl.double().cpu(), 1.0, flags) + \
        0.1 * M.loss(utl.double().cpu(), ul.double().cpu(), 1, 8, flags)[0]
    print(f"with the epocher's keywords {losses[0]:.9g}, with the reference's {losses[1]:.9g}, float64 {float(ref):.9g}")
    assert abs(losses[0] - losses[1]) <= 1e-6 * abs(losses[0]), losses
    assert abs(losses[0] - float(ref)) <= 1e-5 * abs(float(ref)), (losses[0], float(ref))
    assert float((grads[0] - grads[1]).norm() / grads[0].norm()) <= 1e-6


def test_semi_trainer_with_the_midl_hook_checkpoints_and_resumes(tmp_path):
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.trainers.semi import SemiTrainer as ST
    torch.manual_seed(3)
    model = UNet(input_dim=1, num_classes=4, max_channel=128)
    lab = [_batch(2, 64, 30 + k) for k in range(2)]
    unl = [_batch(2, 64, 40 + k) for k in range(2)]
    val = [((b[0][0], b[0][2]), b[1], b[2]) for b in lab]
    cfg = {"Optim": {"name": "RAdam", "lr": 1e-5, "weight_decay": 1e-5}, "Data": {"name": "acdc"},
           "Trainer": {"max_epoch": 1}, "MIDLPaperParameters": MIDL}
    tr = ST(model=model, labeled_loader=lab, unlabeled_loader=unl, val_loader=val, test_loader=None, criterion=KL_div(),
            save_dir=str(tmp_path), max_epoch=1, num_batches=2, device=DEV, two_stage=True, disable_bn=True, config=cfg)
    tr.register_hooks(*create_hook_from_config(model, cfg))
    tr.init()
    hist = tr.start_training()
    assert len(hist) == 1
    text = str(hist[-1]["tra"])
    for name in ("sup_loss", "reg_loss", "midl", "iic_mi", "consistency"):
        assert name in text, (name, text)
    assert "__hooks__" in torch.load(tmp_path / "last.pth", map_location="cpu")
    saved_hooks = {k: v.clone() for k, v in tr.__hooks__.state_dict().items()}
    saved_model = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    model2 = UNet(input_dim=1, num_classes=4, max_channel=128)
    tr2 = ST(model=model2, labeled_loader=lab, unlabeled_loader=unl, val_loader=val, test_loader=None, criterion=KL_div(),
             save_dir=None, max_epoch=1, num_batches=2, device=DEV, two_stage=True, disable_bn=True, config=cfg)
    tr2.register_hooks(*create_hook_from_config(model2, cfg))
    tr2.init()
    tr2.resume_from_path(str(tmp_path / "last.pth"))
    got = tr2.__hooks__.state_dict()
    assert sorted(got) == sorted(saved_hooks)
    for k, v in got.items():
        assert torch.equal(v.cpu(), saved_hooks[k].cpu()), k
    for k, v in model2.state_dict().items():
        assert torch.equal(v.detach().cpu(), saved_model[k]), k
