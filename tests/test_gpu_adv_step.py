"""GPU: one step of ``AdversarialEpocher`` against the float64 restatement of the adversarial scheme
(tests/_adv_oracle.adversarial_step) fed the logits the HIP UNet produced -- supervised, generator and discriminator losses,
the gradient that reaches the unlabelled logits, the discriminator's gradients at its optimizer step, three
running-statistic updates; ``reg_weight = 0`` touches neither the unlabelled loader nor the discriminator; and
``AdversarialTrainer`` over two epochs with checkpoints and a resume.  UNet at ``max_channel=128`` on 64 x 64 slices (the
smallest input the discriminator's head accepts).  Tolerance: ``_adv_oracle.bound``; measured values are printed."""
import pytest
import torch

from oracle import spcl_oracle as O
from tests import _adv_oracle as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _check(name, got, f32, ref64):
    err, tol = A.rel_l2(got, ref64), A.bound(f32, ref64)
    print(f"{name}: rel L2 {err:.3e} (float32 CPU {A.rel_l2(f32, ref64):.3e}, bound {tol:.3e})")
    assert err <= tol, (name, err, tol)


def _batch(n, size, seed):
    g = torch.Generator().manual_seed(seed)
    img, img_tf = torch.rand(n, 1, size, size, generator=g), torch.rand(n, 1, size, size, generator=g)
    tgt = torch.randint(0, 4, (n, 1, size, size), generator=g)
    names = [f"patient{k:03d}_00_{k}" for k in range(n)]
    return (img, img_tf, tgt, tgt.clone()), names, (["0"] * n, names)


class _Tap:
    """the model as the epocher sees it, remembering every forward's logits and the gradient that reaches them"""

    def __init__(self, model):
        self.model, self.logits, self.grads, self.calls = model, [], {}, {}

    @property
    def num_classes(self):
        return self.model.num_classes

    def train(self):
        self.model.train()
        return self

    def __call__(self, x):
        out = self.model(x)
        i = len(self.logits)
        self.logits.append(out.detach().clone())

        def keep(g, i=i):
            self.grads[i] = g.detach().clone()
            self.calls[i] = self.calls.get(i, 0) + 1
        out.register_hook(keep)
        return out


class _Untouchable:
    def __iter__(self):
        raise AssertionError("the unlabelled loader was asked for an iterator")

    def __next__(self):
        raise AssertionError("the unlabelled loader was advanced")


def _setup(consider_image, reg_weight, labeled_loader=(), unlabeled_loader=(), hidden=16):
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.arch.discr import Discriminator
    from spcl_amd.semi_seg.epochers.adversarial import AdversarialEpocher
    model = UNet(input_dim=1, num_classes=4, max_channel=128)
    model.load_state_dict(O.init_unet_state(1, 4, 128, seed=41))
    model.to(DEV).train().set_compute_dtype(torch.float32)
    torch.manual_seed(43)
    D = Discriminator(5 if consider_image else 4, hidden)
    with torch.no_grad():
        for i in (0, 2, 5, 8, 11):
            D._main[i].weight.mul_(6.0)
    D.to(DEV).train()
    tap = _Tap(model)
    ep = AdversarialEpocher(model=tap, optimizer=torch.optim.SGD(model.parameters(), lr=0.0), labeled_loader=list(labeled_loader),
                            unlabeled_loader=unlabeled_loader, sup_criterion=KL_div(), num_batches=1, device=DEV,
                            discriminator=D, discr_optimizer=torch.optim.SGD(D.parameters(), lr=0.0), reg_weight=reg_weight,
                            dis_consider_image=consider_image)
    return model, D, tap, ep


@pytest.mark.parametrize("consider_image", [False, True])
def test_adversarial_step_vs_float64_oracle(consider_image):
    from spcl_amd import functional as F_hip
    rw = 0.5
    model, D, tap, ep = _setup(consider_image, rw)
    state0 = {k: v.detach().clone() for k, v in D.state_dict().items()}
    lab, unl = _batch(2, 64, 1), _batch(3, 64, 2)
    with ep.meters.focus_on(ep.meter_focus):
        sup, gen, dis = ep.step(lab, unl)
        stats = ep.meters.statistics()
    torch.cuda.synchronize()
    assert len(tap.logits) == 2 and tap.calls == {0: 1, 1: 1}  # two forwards; the discriminator update reached neither
    ll, ul = tap.logits[0].cpu(), tap.logits[1].cpu()
    want = {}
    for dt in (torch.float64, torch.float32):
        net = A.load_into(A.discriminator(5 if consider_image else 4, 16, dt), state0).train()
        out = A.adversarial_step(net, ll.to(dt), ul.to(dt), lab[0][0].to(dt), unl[0][0].to(dt), rw, consider_image)
        want[dt] = out + (O.finetune_loss(ll.to(dt), lab[0][2].squeeze(1)).detach(), net.state_dict())
    w64, w32 = want[torch.float64], want[torch.float32]
    _check("sup_loss", sup, w32[4], w64[4])
    _check("gen_loss", gen, w32[0], w64[0])
    _check("dis_loss", dis, w32[1], w64[1])
    _check("gradient at the unlabelled logits", tap.grads[1], w32[2], w64[2])
    # the labelled logits receive the supervised gradient alone
    probe = tap.logits[0].clone().requires_grad_(True)
    s2, _ = F_hip.sup_loss_kl_onehot(probe, lab[0][2].squeeze(1).to(DEV), 1e-16)
    assert torch.equal(torch.autograd.grad(s2, probe)[0], tap.grads[0])
    # the discriminator's gradients at its optimizer step: its own update's, nothing left from the segmentation pass
    for k, p in D.named_parameters():
        kk = k.split(".", 1)[1]
        _check(f"discriminator gradient {k}", p.grad, w32[3][kk], w64[3][kk])
    # three training-mode forwards moved the running statistics
    for k, v in D.state_dict().items():
        kk = k.split(".", 1)[1]
        if k.endswith("num_batches_tracked"):
            assert int(v) == 3 == int(w64[5][kk]), k
        elif "running" in k:
            _check(f"after the step, {k}", v, w32[5][kk], w64[5][kk])
    adv = stats["adv_reg"]
    assert abs(adv["gen_loss"]["mean"] - float(gen.detach())) <= 1e-6 * abs(float(gen.detach()))
    assert abs(adv["dis_loss"]["mean"] - float(dis.detach())) <= 1e-6 * abs(float(dis.detach()))
    assert "reg_loss" not in stats[ep.meter_focus] and "sup_loss" in stats[ep.meter_focus]


def test_segmentation_pass_computes_no_discriminator_gradient():
    from spcl_amd import functional as F_hip
    model, D, tap, ep = _setup(False, 0.5)
    logits = torch.randn(2, 4, 64, 64, device=DEV, requires_grad=True)
    with D.no_weight_grads():
        loss = D.bce(F_hip.softmax_classes(logits), 1)
    loss.backward()
    assert logits.grad is not None and float(logits.grad.abs().sum()) > 0
    assert all(p.grad is None for p in D.parameters())
    assert D._weight_grads is True  # the context put the switch back


def test_zero_reg_weight_touches_nothing():
    lab = _batch(2, 64, 1)
    model, D, tap, ep = _setup(True, 0.0, labeled_loader=[lab], unlabeled_loader=_Untouchable())
    before = {k: v.detach().clone() for k, v in D.state_dict().items()}
    stats = ep.run()
    torch.cuda.synchronize()
    for k, v in D.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert all(p.grad is None for p in D.parameters())
    adv = stats["adv_reg"]
    assert adv["gen_loss"]["mean"] == 0.0 and adv["dis_loss"]["mean"] == 0.0 and adv["reg_weight"]["mean"] == 0.0
    assert len(tap.logits) == 1 and stats[ep.meter_focus]["sup_loss"]["mean"] > 0


def _stores():
    from spcl_amd.semi_seg.data import ACDCSliceStore, synthetic_slice_store
    store = synthetic_slice_store(scans=4, slices_per_scan=(5, 6), size=72, device="cuda", seed=2)
    targets = (store.images * 4).floor().clamp(0, 3).to(torch.uint8)
    return ACDCSliceStore(store.images, store._filenames, targets=targets), store


def test_adversarial_trainer_epochs_checkpoints_and_resume(tmp_path):
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.data.creator import ScanBatchLoader, UnlabeledDeviceLoader
    from spcl_amd.semi_seg.data.loader import LabeledDeviceLoader
    from spcl_amd.semi_seg.trainers.semi import AdversarialTrainer
    labelled, unlabelled = _stores()
    cfg = {"Optim": {"name": "RAdam", "lr": 1e-5, "weight_decay": 1e-5}, "Scheduler": {"multiplier": 300, "warmup_max": 10},
           "Data": {"name": "acdc"}, "RandomSeed": 10, "Trainer": {"max_epoch": 2}}

    def build(save_dir):
        torch.manual_seed(3)
        model = UNet(input_dim=1, num_classes=4, max_channel=128)
        tr = AdversarialTrainer(model=model, labeled_loader=LabeledDeviceLoader(labelled, batch_size=2, out_hw=(64, 64)),
                                unlabeled_loader=UnlabeledDeviceLoader(unlabelled, batch_size=2, out_hw=(64, 64)),
                                val_loader=ScanBatchLoader(labelled, out_hw=(64, 64)), test_loader=None, criterion=KL_div(),
                                save_dir=save_dir, max_epoch=2, num_batches=3, device=DEV, two_stage=False, disable_bn=False,
                                config=cfg, reg_weight=0.1, dis_consider_image=True)
        tr.init()
        return tr

    tr = build(str(tmp_path))
    d0 = {k: v.detach().clone() for k, v in tr._discriminator.state_dict().items()}
    hist = tr.start_training()
    assert len(hist) == 2
    tra = hist[-1]["tra"]
    assert set(tra["adv_reg"]) == {"dis_loss", "gen_loss", "reg_weight"} and "reg_loss" not in tra["semi"]
    assert tra["adv_reg"]["reg_weight"]["mean"] == pytest.approx(0.1) and tra["adv_reg"]["dis_loss"]["mean"] > 0
    assert int(tr._discriminator._main[3].num_batches_tracked) == 2 * 3 * 3  # three passes per step
    assert not torch.equal(tr._discriminator._main[0].weight, d0["_main.0.weight"])  # its optimizer moved it
    # the scheduler drives the model's optimizer only
    assert tr._dis_optimizer.param_groups[0]["lr"] == 1e-5
    assert tr._optimizer.param_groups[0]["lr"] == pytest.approx(1e-5 * (299.0 * 2 / 10 + 1.0))
    for f in ("best.pth", "last.pth"):
        sd = torch.load(tmp_path / f, map_location="cpu")
        assert "_discriminator" in sd and "_dis_optimizer" in sd and len(sd["_discriminator"]) == 20
    saved = {k: v.detach().clone() for k, v in tr._discriminator.state_dict().items()}
    saved_opt = tr._dis_optimizer.state_dict()
    tr2 = build(None)
    tr2.resume_from_path(str(tmp_path / "last.pth"))
    for k, v in tr2._discriminator.state_dict().items():
        assert torch.equal(v.cpu(), saved[k].cpu()), k
    for a, b in zip(tr2._dis_optimizer.state_dict()["state"].values(), saved_opt["state"].values()):
        for k in a:  # (the tensors: step count, moments, device-side lr; ``lr_host`` is a host cache, unset after a load)
            if torch.is_tensor(a[k]):
                assert torch.equal(a[k].cpu(), b[k].cpu()), k
    assert tr2._dis_optimizer.param_groups[0]["lr"] == 1e-5
    assert tr2._cur_epoch == 2
