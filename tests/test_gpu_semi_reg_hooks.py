"""GPU: the mean-teacher and entropy-minimisation hooks.

Each hook on given logits against the float64 criterion (as tests/test_gpu_iic_hooks.py drives the consistency hook); the
teacher after a call is the float64 moving average of its previous value and the student within the bound derived in
tests/test_gpu_semi_reg_kernels.py, and its parameters are views of one storage.  One ``SemiSupervisedEpocher.step`` per
hook over a ``FlatParams`` (the one-launch moving average): ``reg_loss`` against float64, every parameter's gradient against
supervised gradient + the float64 d(logits) pulled back through a second, identically initialised model, the teacher moved
by the student's weights from BEFORE the optimizer step and untouched by the optimizer.  Further steps issue no
synchronising call.  A ``SemiTrainer`` built from ``MeanTeacherParameters`` trains, checkpoints and resumes bit for bit."""
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import spcl_oracle as O
from tests import _iic_oracle as R
from tests.test_gpu_semi_step import _batch, _rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
MT = {"name": "mse", "weight": 10, "alpha": 0.999, "weight_decay": 0.000001}


def _unet(seed=41, cmax=128):
    from spcl_amd.semi_seg.arch import UNet
    sd = O.init_unet_state(1, 4, cmax, seed=seed)
    model = UNet(input_dim=1, num_classes=4, max_channel=cmax)
    model.load_state_dict(sd)
    model.to(DEV).train().set_compute_dtype(torch.float32)
    return sd, model


def _drive(th, model=None):
    """an epocher hook with meters of its own and (for the mean teacher) an epocher that holds the student"""
    from spcl_amd.contrastyou.meters import MeterInterface
    eh = th()
    meters = MeterInterface(default_focus="semi")
    eh.meters = meters
    eh.configure_meters(meters)
    eh._epocher = types.SimpleNamespace(_model=model)
    return eh


def _mt64(t, s64, flags, teacher_softmax=False):
    tt = R.flip(t.double().cpu(), flags)
    if teacher_softmax:
        tt = tt.softmax(1)
    return F.mse_loss(tt.detach(), s64.softmax(1))


def _ema_check(got, before, student, alpha, decay):
    """every teacher parameter against the float64 moving average: three f32 roundings and the f32 scalars, 4 * 2^-24 * max"""
    for k in before:
        ref = (alpha * before[k].double() + (1 - alpha) * student[k].double()) * (1 - decay)
        bound = 4 * U * torch.maximum(before[k].double().abs(), student[k].double().abs())
        err = (got[k].double() - ref).abs()
        assert bool((err <= bound).all()), (k, float((err / bound.clamp_min(1e-300)).max()))


def _snapshot(module):
    return {k: p.detach().cpu().clone() for k, p in module.named_parameters()}


@pytest.mark.parametrize("teacher_softmax", [False, True])
def test_mean_teacher_hook_vs_float64(teacher_softmax):
    from spcl_amd.semi_seg.hooks.mt import MeanTeacherTrainerHook
    _, model = _unet()
    th = MeanTeacherTrainerHook("meanteacher", 10.0, model, alpha=0.999, weight_decay=1e-5, teacher_softmax=teacher_softmax)
    th.to(DEV)
    with torch.no_grad():  # a student that has moved away from its teacher
        g = torch.Generator().manual_seed(5)
        for p in model.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g).to(DEV))
    th._updater.step = 3  # alpha_t = 3/4
    eh = _drive(th, model)
    g = torch.Generator().manual_seed(1)
    img = torch.rand(3, 1, 32, 32, generator=g).to(DEV)
    b = torch.randn(3, 4, 32, 32, generator=g)
    flags = [3, 0, 1]
    with torch.no_grad():
        tout = th.teacher_model(img).float().cpu()  # (training mode: batch statistics, the same at the hook's own pass)
    before, student = _snapshot(th.teacher_model), _snapshot(model)
    bd = b.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    loss = eh(unlabeled_tf_logits=bd, unlabeled_image=img, seed=0, affine_transformer=None,
              flip_flags=torch.tensor(flags, dtype=torch.uint8, device=DEV))
    loss.backward()
    b64 = b.double().requires_grad_(True)
    ref = 10.0 * _mt64(tout, b64, flags, teacher_softmax)
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * float(ref), (float(loss), float(ref))
    assert _rel_l2(bd.grad, b64.grad) <= 1e-5
    # the moving average ran in this call (a bare model: one launch per parameter tensor), on a flat teacher
    assert th._updater.step == 4
    _ema_check(_snapshot(th.teacher_model), before, student, 0.75, 1e-5)
    tp = list(th.teacher_model.parameters())
    assert len({p.untyped_storage().data_ptr() for p in tp}) == 1
    assert not any(p.requires_grad for p in tp)
    assert sorted(th.state_dict()) == sorted("_teacher_model." + k for k in model.state_dict())
    # without flags the hook draws the transformer's decisions under the seed, as mt.py:50-51 does
    from spcl_amd.semi_seg.epochers.helper import TensorRandomFlip
    seed = 1234
    dec = O.random_flip_decisions(seed, 3)
    with torch.no_grad():
        tout = th.teacher_model(img).float().cpu()
    loss2 = eh(unlabeled_tf_logits=bd, unlabeled_image=img, seed=seed,
               affine_transformer=TensorRandomFlip(axis=[1, 2], threshold=0.8))
    ref2 = 10.0 * _mt64(tout, b.double(), [int(d[0]) | (int(d[1]) << 1) for d in dec], teacher_softmax)
    assert abs(float(loss2) - float(ref2)) <= 1e-5 * float(ref2)


def test_entropy_hook_vs_float64():
    from spcl_amd.contrastyou.losses.kl import Entropy
    from spcl_amd.semi_seg.hooks import create_entropy_min_hook
    eh = _drive(create_entropy_min_hook(weight=0.5))
    g = torch.Generator().manual_seed(2)
    a = torch.randn(3, 4, 20, 24, generator=g)
    ad = a.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    loss = eh(unlabeled_tf_logits=None, unlabeled_logits_tf=ad, seed=0, affine_transformer=None)
    loss.backward()
    a64 = a.double().requires_grad_(True)
    ref = 0.5 * Entropy()(a64.softmax(1))
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * float(ref)
    assert _rel_l2(ad.grad, a64.grad) <= 1e-5


# ------------------------------------------------------------------------------------------------ one epocher step
def _setup(section, params, lr=0.05, n=2, size=64):
    from spcl_amd import ddp
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.epochers.semi import SemiSupervisedEpocher
    sd, model = _unet()
    (hook,) = create_hook_from_config(model, {"Data": {"name": "acdc"}, "Trainer": {"max_epoch": 2}, section: params})
    hook.to(DEV)
    flat = ddp.FlatParams([p for p in model.parameters() if p.requires_grad] +
                          [p for p in hook.parameters() if p.requires_grad])
    opt = torch.optim.SGD([flat.param], lr=lr)
    ep = SemiSupervisedEpocher(model=model, optimizer=opt, labeled_loader=[], unlabeled_loader=[], sup_criterion=KL_div(),
                               num_batches=1, device=DEV, flat_params=flat)
    ep.add_hooks([hook()])
    return sd, model, hook, ep, flat


def _reference_grads(sd, lab, unl, flags, dlogits_of):
    """supervised gradients + the pull-back of a float64 d(logits) through a second, identically initialised model.
    ``dlogits_of(unlabeled_logits, unlabeled_tf_logits) -> (which, d)``: the logits the regulariser reads (0: of the
    unlabelled images, 1: of their flipped second view) and its float64 gradient for them"""
    from spcl_amd import functional as F_hip
    from spcl_amd.semi_seg.arch import UNet
    model = UNet(input_dim=1, num_classes=4, max_channel=128)
    model.load_state_dict(sd)
    model.to(DEV).train().set_compute_dtype(torch.float32)
    n = unl[0][0].shape[0]
    fl = torch.tensor(flags, dtype=torch.uint8, device=DEV)
    utf = F_hip.flip_batch(unl[0][1].to(DEV).contiguous(), fl)
    logits = model(torch.cat([lab[0][0].to(DEV), unl[0][0].to(DEV), utf], dim=0))
    ll, ul, utl = torch.split(logits, [n, n, n], dim=0)
    sup, _ = F_hip.sup_loss_kl_onehot(ll, lab[0][2].to(DEV).squeeze(1), 1e-16)
    which, d = dlogits_of(ul.detach().double().cpu(), utl.detach().double().cpu())
    target = (ul, utl)[which]
    params = dict(model.named_parameters())
    grads = torch.autograd.grad([sup, target], list(params.values()),
                                grad_outputs=[torch.ones_like(sup), d.float().to(DEV)])
    return float(sup), dict(zip(params, grads))


def _check_step_grads(model, flat, ref_grads):
    views = {id(p): v for p, v in zip(flat.params, flat.views)}
    for k, p in model.named_parameters():
        err = _rel_l2(views[id(p)], ref_grads[k])
        assert err <= 5e-3, (k, err)


def test_semi_step_with_the_mean_teacher():
    sd, model, hook, ep, flat = _setup("MeanTeacherParameters", MT)
    lab, unl = _batch(2, 64, 1), _batch(2, 64, 2)
    seed = 1234
    flags = [int(d[0]) | (int(d[1]) << 1) for d in O.random_flip_decisions(seed, 2)]
    teacher = hook.teacher_model
    inside = {id(p) for p in flat.params}
    assert flat.numel == sum(p.numel() for p in model.parameters())
    assert all(id(p) not in inside and not p.requires_grad for p in teacher.parameters())
    with torch.no_grad():  # a student that has moved away from its teacher; alpha_t = 3/4
        g = torch.Generator().manual_seed(5)
        for p in model.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g).to(DEV))
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        tout = teacher(unl[0][0].to(DEV)).double().cpu()
    hook._updater.step = 3
    t_before, s_before = _snapshot(teacher), _snapshot(model)
    with ep.meters.focus_on(ep.meter_focus):
        sup, reg = ep.step(lab, unl, seed=seed)
    torch.cuda.synchronize()
    s_after = _snapshot(model)
    assert any(not torch.equal(s_after[k], s_before[k]) for k in s_before)  # (the optimizer did step)
    # the teacher: moved by the student's weights from before the optimizer step, in one launch over the flat slices
    _ema_check(_snapshot(teacher), t_before, s_before, 0.75, MT["weight_decay"])
    assert len({p.untyped_storage().data_ptr() for p in teacher.parameters()}) == 1
    assert hook._updater.step == 4
    from spcl_amd.semi_seg.hooks.mt import _dense_run
    assert _dense_run([p.data for p in model.parameters()]) is not None

    holder = {}

    def dlogits(ul, utl):
        u64 = utl.clone().requires_grad_(True)
        loss = MT["weight"] * _mt64(tout, u64, flags)
        loss.backward()
        holder["reg"] = float(loss)
        return 1, u64.grad

    osup, ref_grads = _reference_grads(sd, lab, unl, flags, dlogits)
    assert abs(float(sup) - osup) <= 1e-4 * abs(osup), (float(sup), osup)
    assert abs(float(reg) - holder["reg"]) <= 1e-4 * abs(holder["reg"]), (float(reg), holder["reg"])
    _check_step_grads(model, flat, ref_grads)


def test_semi_step_with_entropy_minimisation():
    from spcl_amd.contrastyou.losses.kl import Entropy
    sd, model, hook, ep, flat = _setup("EntropyMinParameters", {"weight": 0.3})
    lab, unl = _batch(2, 64, 1), _batch(2, 64, 2)
    seed = 1234
    flags = [int(d[0]) | (int(d[1]) << 1) for d in O.random_flip_decisions(seed, 2)]
    with ep.meters.focus_on(ep.meter_focus):
        sup, reg = ep.step(lab, unl, seed=seed)
    torch.cuda.synchronize()
    holder = {}

    def dlogits(ul, utl):
        u64 = ul.clone().requires_grad_(True)
        loss = 0.3 * Entropy()(R.flip(u64, flags).softmax(1))
        loss.backward()
        holder["reg"] = float(loss)
        return 0, u64.grad

    osup, ref_grads = _reference_grads(sd, lab, unl, flags, dlogits)
    assert abs(float(sup) - osup) <= 1e-4 * abs(osup), (float(sup), osup)
    assert abs(float(reg) - holder["reg"]) <= 1e-4 * abs(holder["reg"]), (float(reg), holder["reg"])
    _check_step_grads(model, flat, ref_grads)


@pytest.mark.parametrize("section,params", [("MeanTeacherParameters", MT), ("EntropyMinParameters", {"weight": 0.3})])
def test_further_steps_issue_no_host_sync(section, params):
    sd, model, hook, ep, flat = _setup(section, params)
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


def test_semi_trainer_with_the_mean_teacher_checkpoints_and_resumes(tmp_path):
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.trainers.semi import SemiTrainer as ST
    torch.manual_seed(3)
    model = UNet(input_dim=1, num_classes=4, max_channel=128)
    lab = [_batch(2, 64, 30 + k) for k in range(3)]
    unl = [_batch(2, 64, 40 + k) for k in range(3)]
    val = [((b[0][0], b[0][2]), b[1], b[2]) for b in lab]
    cfg = {"Optim": {"name": "RAdam", "lr": 1e-5, "weight_decay": 1e-5}, "Data": {"name": "acdc"},
           "Trainer": {"max_epoch": 2}, "MeanTeacherParameters": MT}
    tr = ST(model=model, labeled_loader=lab, unlabeled_loader=unl, val_loader=val, test_loader=None, criterion=KL_div(),
            save_dir=str(tmp_path), max_epoch=2, num_batches=3, device=DEV, two_stage=True, disable_bn=True, config=cfg)
    tr.register_hooks(*create_hook_from_config(model, cfg))
    tr.init()
    teacher = tr.__hooks__[0].teacher_model
    inside = {id(p) for p in tr._flat.params}
    assert tr._flat.numel == sum(p.numel() for p in model.parameters())
    assert all(id(p) not in inside for p in teacher.parameters())
    hist = tr.start_training()
    assert len(hist) == 2
    flat = str(hist[-1]["tra"])
    for name in ("sup_loss", "reg_loss", "meanteacher"):
        assert name in flat, (name, flat)
    assert tr.__hooks__[0]._updater.step == 6
    # six updates in: the teacher is neither the initial weights nor the student
    sd_t, sd_s = teacher.state_dict(), model.state_dict()
    assert not torch.equal(sd_t["_Conv1.conv.0.weight"], sd_s["_Conv1.conv.0.weight"])
    assert "__hooks__" in torch.load(tmp_path / "last.pth", map_location="cpu")
    saved = {k: v.clone() for k, v in tr.__hooks__.state_dict().items()}
    assert any(k.endswith("_teacher_model._Conv1.conv.0.weight") for k in saved)
    model2 = UNet(input_dim=1, num_classes=4, max_channel=128)
    tr2 = ST(model=model2, labeled_loader=lab, unlabeled_loader=unl, val_loader=val, test_loader=None, criterion=KL_div(),
             save_dir=None, max_epoch=2, num_batches=3, device=DEV, two_stage=True, disable_bn=True, config=cfg)
    tr2.register_hooks(*create_hook_from_config(model2, cfg))
    tr2.init()
    tr2.resume_from_path(str(tmp_path / "last.pth"))
    got = tr2.__hooks__.state_dict()
    assert sorted(got) == sorted(saved)
    for k, v in got.items():
        assert torch.equal(v.cpu(), saved[k].cpu()), k
