"""GPU: the mix-up hook, epocher and trainer.

The hook on a small UNet under a given seed against the float64 oracle (``O.unet_forward`` on the restated ``mixed_x``,
``kl_div`` on ``mixed_y``): returned loss, the gradient reaching every parameter, the meter; with ``enable_bn=False`` the
running statistics stay as they were, bit for bit.  One ``MixUpEpocher.step`` (B = 2, 64 x 64, f32, hook weight 1.0):
``sup`` / ``reg`` within 1e-4 relative and every parameter's gradient within 5e-3 relative L2 of the oracle -- the bars
tests/test_gpu_semi_step.py holds an f32 step to; the hook test runs the same network arithmetic on a smaller input and is
held to the same two.  The step test asserts on the oracle alone that the regulariser carries at least a quarter of every
parameter's gradient norm, so that a wrong mix-up gradient cannot hide below the 5e-3 bar (at the configuration's weight of
0.01 its share is 0.004: that weight would test nothing).  Further steps issue no synchronising call.  A ``MixUpTrainer``
built as main_mixup.py builds it trains two epochs, writes best / last checkpoints, and a trainer resumed from the first
epoch's checkpoint reaches the same parameters bit for bit."""
import itertools
import random
import shutil

import pytest
import torch

from oracle import spcl_oracle as O
from tests import _mixup_oracle as M
from tests.test_gpu_semi_reg_hooks import _drive, _unet
from tests.test_gpu_semi_step import _batch, _rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_names = itertools.count()


def _hook(**params):
    """hook names are claimed once per process (contrastyou/hooks/base.py): every construction takes a fresh one"""
    from spcl_amd.semi_seg.hooks.mixup import MixUpHook
    return MixUpHook(hook_name=f"mx_hook_{next(_names)}", **params)


def _params64(sd):
    return {k: ((v.double().requires_grad_(True) if "running" not in k else v.double()) if v.is_floating_point()
                else v.clone()) for k, v in sd.items()}


def _buffers(model):
    return {k: v.detach().cpu().clone() for k, v in model.named_buffers()}


@pytest.mark.parametrize("enable_bn", [True, False])
def test_mixup_hook_vs_float64(enable_bn):
    sd, model = _unet()
    weight, seed = 0.7, 4321
    eh = _drive(_hook(weight=weight, enable_bn=enable_bn), model)
    g = torch.Generator().manual_seed(6)
    img, img_tf = torch.rand(3, 1, 32, 32, generator=g), torch.rand(3, 1, 32, 32, generator=g)
    tgt, tgt_tf = torch.randint(0, 4, (3, 1, 32, 32), generator=g), torch.randint(0, 4, (3, 1, 32, 32), generator=g)
    before = _buffers(model)
    loss = eh(labeled_image=img.to(DEV), labeled_image_tf=img_tf.to(DEV), labeled_target=tgt.to(DEV),
              labeled_target_tf=tgt_tf.to(DEV), seed=seed)
    loss.backward()
    torch.cuda.synchronize()
    after = _buffers(model)
    lam, index = M.draw(seed, 6)
    assert 0.0 < lam < 1.0 and index.tolist() != list(range(6))
    p64 = _params64(sd)
    logits = O.unet_forward(M.mixed_x(img, img_tf, lam, index), p64, train=True)
    ref = M.mixup_loss(logits, tgt, tgt_tf, lam, index)
    (weight * ref).backward()
    ref = float(ref.detach())
    assert abs(float(loss) - weight * ref) <= 1e-4 * weight * ref, (float(loss), weight * ref)
    for k, p in model.named_parameters():
        err = _rel_l2(p.grad, p64[k].grad)
        assert err <= 5e-3, (k, err)
    with eh.meters.focus_on("mix_reg"):
        got = eh.meters["mixup_ls"].summary()["mean"]
    assert abs(got - ref) <= 1e-4 * ref, (got, ref)  # the meter holds the unweighted loss
    moved = [k for k in before if not torch.equal(before[k], after[k])]
    if enable_bn:
        assert any("running_mean" in k for k in moved)
    else:
        assert moved == []


# ------------------------------------------------------------------------------------------------ one epocher step
def _setup(weight=1.0, fused=False, cmax=128):
    from spcl_amd import ddp
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.optim import FusedRAdam
    from spcl_amd.semi_seg.epochers.mixup import MixUpEpocher
    sd, model = _unet(cmax=cmax)
    hook = _hook(weight=weight)
    flat = None
    if fused:  # the trainer's plumbing: one flat parameter stepped by the fused RAdam
        flat = ddp.FlatParams([p for p in model.parameters() if p.requires_grad])
        opt = FusedRAdam([flat.param], lr=1e-6, weight_decay=1e-5)
    else:
        opt = torch.optim.SGD(model.parameters(), lr=0.0)
    ep = MixUpEpocher(model=model, optimizer=opt, labeled_loader=[], unlabeled_loader=None, sup_criterion=KL_div(),
                      num_batches=1, device=DEV, flat_params=flat)
    ep.add_hooks([hook()])
    ep.init()
    return sd, model, ep


def test_mixup_step_vs_float64_oracle():
    sd, model, ep = _setup(weight=1.0)
    lab = _batch(2, 64, 1)
    seed = 1234
    with ep.meters.focus_on(ep.meter_focus):
        sup, reg = ep.step(lab, seed=seed)
    torch.cuda.synchronize()
    img, img_tf, tgt, tgt_tf = lab[0]
    lam, index = M.draw(seed, 4)
    p64 = _params64(sd)
    names = [k for k, v in p64.items() if v.requires_grad]
    osup = O.finetune_loss(O.unet_forward(img.double(), p64, train=True), tgt.squeeze(1))
    oreg = 1.0 * M.mixup_loss(O.unet_forward(M.mixed_x(img, img_tf, lam, index), p64, train=True), tgt, tgt_tf, lam, index)
    greg = dict(zip(names, torch.autograd.grad(oreg, [p64[k] for k in names], retain_graph=True)))
    (osup + oreg).backward()
    osup, oreg = osup.detach(), oreg.detach()
    # the condition under which the 5e-3 bar tests the mix-up gradient: it is no small part of any parameter's gradient
    share = {k: float(greg[k].norm() / p64[k].grad.norm()) for k in names}
    print("smallest share of the regulariser in a parameter's gradient:", min(share.values()))
    assert min(share.values()) >= 0.25, min(share.items(), key=lambda kv: kv[1])
    assert abs(float(sup) - float(osup)) <= 1e-4 * abs(float(osup)), (float(sup), float(osup))
    assert abs(float(reg) - float(oreg)) <= 1e-4 * abs(float(oreg)), (float(reg), float(oreg))
    for k, p in model.named_parameters():
        err = _rel_l2(p.grad, p64[k].grad)
        assert err <= 5e-3, (k, err)
    stats = ep.meters.statistics()
    assert abs(stats["semi"]["reg_loss"]["mean"] - float(oreg)) <= 1e-4 * float(oreg)
    assert abs(stats["mix_reg"]["mixup_ls"]["mean"] - float(oreg)) <= 1e-4 * float(oreg)


def test_further_mixup_steps_issue_no_host_sync():
    sd, model, ep = _setup(weight=0.01, fused=True)
    with ep.meters.focus_on(ep.meter_focus):
        ep.step(_batch(2, 64, 1), seed=1)
        torch.cuda.synchronize()
        batches = [_batch(2, 64, 10 + k) for k in range(2)]
        moved = [(tuple(t.pin_memory() for t in b[0]),) + b[1:] for b in batches]
        torch.cuda.set_sync_debug_mode("error")
        try:
            for k, lab in enumerate(moved):
                ep.step(lab, seed=2 + k)
        finally:
            torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    ep.close_hooks()


def test_mixup_trainer_epochs_checkpoints_and_resume(tmp_path):
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.epochers.mixup import MixUpEpocher
    from spcl_amd.semi_seg.trainers.semi import MixUpTrainer
    lab = [_batch(2, 64, 30 + k) for k in range(3)]
    unl = [_batch(2, 64, 40 + k) for k in range(3)]
    val = [((b[0][0], b[0][2]), b[1], b[2]) for b in lab]
    cfg = {"Optim": {"name": "RAdam", "lr": 1e-5, "weight_decay": 1e-5}, "Data": {"name": "acdc"},
           "Trainer": {"max_epoch": 2}, "MixUpParams": {"weight": 0.01, "enable_bn": True}}

    def build(seed, save_dir):  # main_mixup.py:51-62
        torch.manual_seed(seed)
        model = UNet(input_dim=1, num_classes=4, max_channel=128)
        tr = MixUpTrainer(model=model, labeled_loader=lab, unlabeled_loader=unl, val_loader=val, test_loader=None,
                          criterion=KL_div(), save_dir=save_dir, max_epoch=2, num_batches=3, device=DEV, config=cfg)
        tr.register_hooks(_hook(**cfg["MixUpParams"]))
        tr.init()
        return model, tr

    model, tr = build(3, str(tmp_path))
    assert tr.train_epocher is MixUpEpocher
    initial = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    kept = {}
    save_to = tr.save_to

    def save_and_keep(name):  # the first epoch's ``last.pth`` (the second overwrites it) and the host generator's state then
        save_to(name)
        if name == "last.pth" and tr._cur_epoch == 1:
            shutil.copy(tmp_path / "last.pth", tmp_path / "epoch1.pth")
            kept["random"] = random.getstate()

    tr.save_to = save_and_keep
    random.seed(77)  # (the epocher draws each step's seed from python's generator)
    hist = tr.start_training()
    assert len(hist) == 2
    flat = str(hist[-1]["tra"])
    for name in ("sup_loss", "reg_loss", "mix_reg", "mixup_ls"):
        assert name in flat, (name, flat)
    for f in ("best.pth", "last.pth"):
        assert "__hooks__" in torch.load(tmp_path / f, map_location="cpu")
    final = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    assert any(not torch.equal(final[k], initial[k]) for k in final if "weight" in k)
    # resumed from the first epoch's checkpoint, another model runs the second epoch to the same bits
    model2, tr2 = build(4, None)
    tr2.resume_from_path(str(tmp_path / "epoch1.pth"))
    assert tr2._cur_epoch == 1
    random.setstate(kept["random"])
    hist2 = tr2.start_training()
    assert [h["epoch"] for h in hist2] == [2]
    for k, v in model2.state_dict().items():
        assert torch.equal(v.cpu(), final[k]), k
