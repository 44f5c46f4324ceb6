"""GPU: the semi-supervised step (SemiSupervisedEpocher with the UDA-IIC hooks, dense paddings [1, 3]) against a float64
restatement on the CPU oracle's UNet: supervised and regularisation losses and every parameter's gradient, single-stage
and two-stage with and without ``disable_bn`` (running statistics then stay untouched in the second pass).  Steps 2..N
issue no synchronising call.  SemiTrainer runs two epochs, writes best / last checkpoints holding ``__hooks__`` and
resumes the hook parameters bit for bit."""
import pytest
import torch
import torch.nn.functional as F

from oracle import spcl_oracle as O
from tests import _iic_oracle as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UDAIIC = {"feature_names": ["Conv5", "Up_conv3", "Up_conv2"], "mi_weights": [0.1, 0.05, 0.05], "dense_paddings": [1, 3],
          "consistency_weight": 1}


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _batch(n, size, seed):
    g = torch.Generator().manual_seed(seed)
    img, img_tf = torch.rand(n, 1, size, size, generator=g), torch.rand(n, 1, size, size, generator=g)
    tgt = torch.randint(0, 4, (n, 1, size, size), generator=g)
    names = [f"patient{k:03d}_00_{k}" for k in range(n)]
    return (img, img_tf, tgt, tgt.clone()), names, (["0"] * n, names)


def _setup(two_stage, disable_bn, n=2, size=64, cmax=128):
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.epochers.semi import SemiSupervisedEpocher
    sd = O.init_unet_state(1, 4, cmax, seed=41)
    model = UNet(input_dim=1, num_classes=4, max_channel=cmax)
    model.load_state_dict(sd)
    model.to(DEV).train().set_compute_dtype(torch.float32)
    torch.manual_seed(42)
    hook = create_hook_from_config(model, {"Data": {"name": "acdc"}, "Trainer": {"max_epoch": 2},
                                           "DiscreteMIConsistencyParams": UDAIIC})[0]
    hook.to(DEV)
    params = list(model.parameters()) + list(hook.parameters())
    opt = torch.optim.SGD(params, lr=0.0)
    ep = SemiSupervisedEpocher(model=model, optimizer=opt, labeled_loader=[], unlabeled_loader=[],
                               sup_criterion=KL_div(), num_batches=1, device=DEV, two_stage=two_stage,
                               disable_bn=disable_bn)
    ep.add_hooks([hook()])
    return sd, model, hook, ep


def _oracle(sd, hook, lab, unl, seed, two_stage, disable_bn):
    n = unl[0][0].shape[0]
    dec = O.random_flip_decisions(seed, n)
    flags = [int(d[0]) | (int(d[1]) << 1) for d in dec]
    p64 = {k: ((v.double().requires_grad_(True) if "running" not in k else v.double()) if v.is_floating_point()
               else v.clone()) for k, v in sd.items()}
    hp = {k: v.detach().double().cpu().requires_grad_(True) for k, v in hook.state_dict().items()}
    limg, ltgt = lab[0][0].double(), lab[0][2]
    uimg, ucf = unl[0][0].double(), unl[0][1].double()
    utf = R.flip(ucf, flags)

    def net(x, until=None, track=True):
        s = dict(p64) if track else {k: (v.clone() if "running" in k else v) for k, v in p64.items()}
        return O.unet_forward(x, s, until, train=True)

    if not two_stage:
        x = torch.cat([limg, uimg, utf])
        logits = net(x)
        ll, ul, utl = logits[:n], logits[n:2 * n], logits[2 * n:]
        feats = {f: net(x, f, track=False)[-2 * n:] for f in UDAIIC["feature_names"]}
    else:
        ll = net(limg)
        x = torch.cat([uimg, utf])
        lu = net(x, track=not disable_bn)
        ul, utl = lu[:n], lu[n:]
        feats = {f: net(x, f, track=False)[-2 * n:] for f in UDAIIC["feature_names"]}
    sup = O.finetune_loss(ll, ltgt.squeeze(1))
    reg = 0.0
    for h, (f, w) in enumerate(zip(UDAIIC["feature_names"], UDAIIC["mi_weights"])):
        fe = feats[f]
        terms = []
        for s in range(5):
            pre = f"_hooks.0._hooks.{h}._projector._headers.{s}"
            if f == "Conv5":
                z = fe.mean(dim=(2, 3)) @ hp[f"{pre}.2.weight"].t() + hp[f"{pre}.2.bias"]
                terms.append(R.iid_loss(z[:n].softmax(1), z[n:].softmax(1))[0])
            else:
                z = F.conv2d(fe, hp[f"{pre}.0.weight"], hp[f"{pre}.0.bias"])
                pad = UDAIIC["dense_paddings"][h - 1]
                terms.append(R.iid_segmentation_loss(R.flip(z[:n], flags).softmax(1), z[n:].softmax(1), pad))
        reg = reg + sum(terms) / 5 * w
    reg = reg + R.consistency(ul, utl, 1.0, flags)
    (sup + reg).backward()
    return sup, reg, p64, hp, flags


class UNetStats:
    @staticmethod
    def after_labelled_pass(sd, lab):
        """Conv1's first BatchNorm running mean after one training pass of the labelled images on a fresh copy"""
        from spcl_amd.semi_seg.arch import UNet
        m = UNet(input_dim=1, num_classes=4, max_channel=128)
        m.load_state_dict(sd)
        m.to(DEV).train().set_compute_dtype(torch.float32)
        with torch.no_grad():
            m(lab[0][0].to(DEV))
        return m.state_dict()["_Conv1.conv.1.running_mean"].cpu()


@pytest.mark.parametrize("two_stage,disable_bn", [(False, False), (True, False), (True, True)])
def test_semi_step_vs_float64_oracle(two_stage, disable_bn):
    sd, model, hook, ep = _setup(two_stage, disable_bn)
    lab, unl = _batch(2, 64, 1), _batch(2, 64, 2)
    seed = 1234
    assert ep.flip_flags(seed, 2).cpu().tolist() == [int(d[0]) | (int(d[1]) << 1) for d in O.random_flip_decisions(seed, 2)]
    with ep.meters.focus_on(ep.meter_focus):
        sup, reg = ep.step(lab, unl, seed=seed)
    torch.cuda.synchronize()
    osup, oreg, p64, hp, _ = _oracle(sd, hook, lab, unl, seed, two_stage, disable_bn)
    assert abs(float(sup) - float(osup)) <= 1e-4 * abs(float(osup)), (float(sup), float(osup))
    assert abs(float(reg) - float(oreg)) <= 1e-4 * abs(float(oreg)), (float(reg), float(oreg))
    msd = dict(model.named_parameters())
    for k, p in msd.items():
        assert _rel_l2(p.grad, p64[k].grad) <= 5e-3, (k, _rel_l2(p.grad, p64[k].grad))
    for k, p in hook.named_parameters():
        assert _rel_l2(p.grad, hp[k].grad) <= 5e-3, (k, _rel_l2(p.grad, hp[k].grad))
    # running statistics: under disable_bn only the labelled pass moves them
    if disable_bn:
        ref = UNetStats.after_labelled_pass(sd, lab)
        got = model.state_dict()["_Conv1.conv.1.running_mean"].cpu()
        assert torch.allclose(got, ref, rtol=1e-4, atol=1e-6), (got, ref)


def test_semi_steps_issue_no_host_sync():
    sd, model, hook, ep = _setup(True, True)
    with ep.meters.focus_on(ep.meter_focus):
        ep.step(_batch(2, 64, 1), _batch(2, 64, 2), seed=1)
        torch.cuda.synchronize()
        batches = [(_batch(2, 64, 10 + k), _batch(2, 64, 20 + k)) for k in range(2)]
        moved = [tuple(((tuple(t.pin_memory() for t in b[0]),) + b[1:]) for b in pair) for pair in batches]
        torch.cuda.set_sync_debug_mode("error")
        try:
            for k, (lab, unl) in enumerate(moved):
                ep.step(lab, unl, seed=2 + k)
        finally:
            torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    ep.close_hooks()


def test_semi_trainer_epochs_checkpoints_and_resume(tmp_path):
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.trainers.finetune import SemiTrainer  # noqa: F401 (the module the new_trainer alias names)
    from spcl_amd.semi_seg.trainers.semi import SemiTrainer as ST
    torch.manual_seed(3)
    model = UNet(input_dim=1, num_classes=4, max_channel=128)
    lab = [_batch(2, 64, 30 + k) for k in range(3)]
    unl = [_batch(2, 64, 40 + k) for k in range(3)]
    val = [((b[0][0], b[0][2]), b[1], b[2]) for b in lab]
    cfg = {"Optim": {"name": "RAdam", "lr": 1e-5, "weight_decay": 1e-5}, "Data": {"name": "acdc"},
           "Trainer": {"max_epoch": 2}, "DiscreteMIConsistencyParams": UDAIIC}
    tr = ST(model=model, labeled_loader=lab, unlabeled_loader=unl, val_loader=val, test_loader=None, criterion=KL_div(),
            save_dir=str(tmp_path), max_epoch=2, num_batches=3, device=DEV, two_stage=True, disable_bn=True, config=cfg)
    tr.register_hooks(*create_hook_from_config(model, cfg))
    tr.init()
    hist = tr.start_training()
    assert len(hist) == 2
    tra = hist[-1]["tra"]
    flat = str(tra)
    for name in ("sup_loss", "reg_loss", "discreteMI/conv5", "discreteMI/up_conv2", "consistency", "mi"):
        assert name in flat, (name, flat)
    for f in ("best.pth", "last.pth"):
        assert "__hooks__" in torch.load(tmp_path / f, map_location="cpu")
    saved = {k: v.clone() for k, v in tr.__hooks__.state_dict().items()}
    model2 = UNet(input_dim=1, num_classes=4, max_channel=128)
    tr2 = ST(model=model2, labeled_loader=lab, unlabeled_loader=unl, val_loader=val, test_loader=None, criterion=KL_div(),
             save_dir=None, max_epoch=2, num_batches=3, device=DEV, two_stage=True, disable_bn=True, config=cfg)
    tr2.register_hooks(*create_hook_from_config(model2, cfg))
    tr2.init()
    tr2.resume_from_path(str(tmp_path / "last.pth"))
    for k, v in tr2.__hooks__.state_dict().items():
        assert torch.equal(v.cpu(), saved[k].cpu()), k
