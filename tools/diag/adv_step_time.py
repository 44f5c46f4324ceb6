"""Time the adversarial baseline's discriminator at the configured batch (5 labelled + 5 unlabelled class maps of
4 x 224 x 224, ``hidden_dim`` 64) and the whole adversarial step next to a hook-less semi-supervised step:

* the three discriminator passes of one step on HIP -- the generator term (unlabelled map, target 1, gradient w.r.t. the map
  only: no weight gradient is computed), then the labelled (target 1) and unlabelled (target 0) maps with the weight
  gradients -- in total (device events) and per kernel (the library's own launch timer, ``spcl_profile_*``: mean microseconds
  per step and launches per step of every kernel symbol, largest first);
* the same three passes in torch's own formulation on the same device: ``nn.Sequential`` of ``nn.Conv2d`` /
  ``nn.BatchNorm2d`` / ``nn.LeakyReLU`` / ``nn.Sigmoid`` and ``nn.BCELoss`` (the first pass differentiates the weights too,
  as the reference's does);
* one whole step of ``AdversarialEpocher`` (``reg_weight`` 0.5, flat parameters and the fused RAdam for both networks) and
  one of ``SemiSupervisedEpocher`` without hooks on the same UNet and batches.

Every figure is the mean of its repetitions after a warm-up; the measurement is repeated ``--rounds`` times in one process
so that the spread shows.  Lines are printed as they come and written to ``--out`` at the end.  No pass / fail bar.

    python tools/diag/adv_step_time.py [--reps 20] [--rounds 3] [--out profiles/adv_step_time.txt]"""
import argparse
import ctypes
import os
import sys

import torch
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
DEV = "cuda:0"
N, C, HW, HIDDEN = 5, 4, 224, 64


def _time(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _sequential(state):
    h = HIDDEN
    net = nn.Sequential(
        nn.Conv2d(C, h, 4, 2, 1, bias=False), nn.LeakyReLU(0.2, inplace=True),
        nn.Conv2d(h, 2 * h, 4, 2, 1, bias=False), nn.BatchNorm2d(2 * h), nn.LeakyReLU(0.2, inplace=True),
        nn.Conv2d(2 * h, 4 * h, 4, 2, 1, bias=False), nn.BatchNorm2d(4 * h), nn.LeakyReLU(0.2, inplace=True),
        nn.Conv2d(4 * h, 8 * h, 4, 2, 1, bias=False), nn.BatchNorm2d(8 * h), nn.LeakyReLU(0.2, inplace=True),
        nn.Conv2d(8 * h, 1, 4, 1, 0, bias=False), nn.Sigmoid())
    net.load_state_dict({k.split(".", 1)[1]: v for k, v in state.items()})
    return net.to(DEV).train()


def _kernel_table(fn, reps):
    from spcl_amd import native as n
    fn()
    torch.cuda.synchronize()
    n.call("spcl_profile_enable", 1)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    cnt = n.call("spcl_profile_count")
    name = ctypes.create_string_buffer(256)
    us, by, fl = ctypes.c_float(), ctypes.c_double(), ctypes.c_double()
    acc = {}
    for i in range(cnt):
        n.call("spcl_profile_get", i, name, 256, ctypes.byref(us), ctypes.byref(by), ctypes.byref(fl))
        a = acc.setdefault(name.value.decode(), [0.0, 0])
        a[0] += us.value
        a[1] += 1
    n.call("spcl_profile_enable", 0)
    return sorted(((k, v[0] / reps, v[1] / reps) for k, v in acc.items()), key=lambda r: -r[1])


def _discriminator_passes(say, reps, table):
    from spcl_amd import functional as F_hip
    from spcl_amd.semi_seg.arch.discr import Discriminator
    torch.manual_seed(10)
    D = Discriminator(C, HIDDEN).to(DEV).train()
    ref = _sequential(D.state_dict())
    g = torch.Generator().manual_seed(1)
    lab = torch.randn(N, C, HW, HW, generator=g).softmax(1).to(DEV).contiguous(memory_format=torch.channels_last)
    unl = torch.randn(N, C, HW, HW, generator=g).softmax(1).to(DEV).contiguous(memory_format=torch.channels_last)
    unit = F_hip.register_unit_gradient(torch.ones((), device=DEV))
    bce = nn.BCELoss()
    out = {}

    def hip():
        x = unl.detach().requires_grad_(True)
        with D.no_weight_grads():
            D.bce(x, 1).backward(gradient=unit)
        for p in D.parameters():
            p.grad = None
        loss = D.bce(lab, 1) + D.bce(unl, 0)
        loss.backward(gradient=unit)
        out["hip"] = (float(loss.detach()) if "hip" not in out else out["hip"][0], x.grad)

    def torch_ops():
        x = unl.detach().requires_grad_(True)
        d = ref(x)
        bce(d, torch.ones_like(d)).backward()
        ref.zero_grad(set_to_none=True)
        dl, du = ref(lab), ref(unl)
        loss = bce(dl, torch.ones_like(dl)) + bce(du, torch.zeros_like(du))
        loss.backward()
        out["torch"] = (float(loss.detach()) if "torch" not in out else out["torch"][0], x.grad)

    t_hip, t_torch = _time(hip, reps), _time(torch_ops, reps)
    say(f"three discriminator passes, forward + backward: HIP {t_hip:.2f} ms, torch nn.Sequential {t_torch:.2f} ms "
        f"(HIP / torch = {t_hip / t_torch:.2f}; first measured dis_loss {out['hip'][0]:.6f} vs {out['torch'][0]:.6f})")
    if table:
        rows = _kernel_table(hip, max(2, reps // 4))
        total = sum(r[1] for r in rows)
        say(f"  HIP kernels per step (launch timer; sum {total / 1e3:.2f} ms):")
        for k, us, cnt in rows:
            say(f"    {us:9.1f} us  {cnt:5.1f} launches  {k}")
    return t_hip, t_torch


def _whole_steps(say, reps):
    from spcl_amd import ddp as _ddp
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.optim import FusedRAdam
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.arch.discr import Discriminator
    from spcl_amd.semi_seg.epochers.adversarial import AdversarialEpocher
    from spcl_amd.semi_seg.epochers.semi import SemiSupervisedEpocher

    def batch(seed):
        g = torch.Generator().manual_seed(seed)
        img, img_tf = torch.rand(N, 1, HW, HW, generator=g).to(DEV), torch.rand(N, 1, HW, HW, generator=g).to(DEV)
        tgt = torch.randint(0, 4, (N, 1, HW, HW), generator=g).to(DEV)
        names = [f"patient{k:03d}_00_{k}" for k in range(N)]
        return (img, img_tf, tgt, tgt.clone()), names, (["0"] * N, names)

    lab, unl = batch(1), batch(2)
    res = {}
    for kind in ("adversarial", "semi"):
        torch.manual_seed(3)
        model = UNet(input_dim=1, num_classes=4).to(DEV).train()
        flat = _ddp.FlatParams(list(model.parameters()))
        opt = FusedRAdam([flat.param], lr=1e-7, weight_decay=1e-5)
        if kind == "adversarial":
            D = Discriminator(C, HIDDEN).to(DEV).train()
            dflat = _ddp.FlatParams(list(D.parameters()))
            ep = AdversarialEpocher(model=model, optimizer=opt, labeled_loader=[], unlabeled_loader=[], sup_criterion=KL_div(),
                                    num_batches=1, device=DEV, flat_params=flat, discriminator=D,
                                    discr_optimizer=FusedRAdam([dflat.param], lr=1e-7, weight_decay=1e-5), reg_weight=0.5,
                                    dis_consider_image=False, discr_flat_params=dflat)
            step = lambda: ep.step(lab, unl)  # noqa: E731
        else:
            ep = SemiSupervisedEpocher(model=model, optimizer=opt, labeled_loader=[], unlabeled_loader=[],
                                       sup_criterion=KL_div(), num_batches=1, device=DEV, flat_params=flat)
            step = lambda: ep.step(lab, unl, seed=1)  # noqa: E731
        with ep.meters.focus_on(ep.meter_focus):
            res[kind] = _time(step, reps)
    say(f"whole step at {N} + {N} slices of {HW} x {HW}: AdversarialEpocher (reg_weight 0.5) {res['adversarial']:.2f} ms, "
        f"SemiSupervisedEpocher without hooks (labelled + unlabelled pair in one forward) {res['semi']:.2f} ms")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "adv_step_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adv_step_time.py measures on the GPU: no device found")
    import spcl_amd  # noqa: F401
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"discriminator({C}, {HIDDEN}) on {N} + {N} class maps of {C} x {HW} x {HW} f32 channels-last; {args.reps} reps per figure")
    for r in range(args.rounds):
        say(f"round {r}")
        _discriminator_passes(say, args.reps, table=(r == 0))
        _whole_steps(say, args.reps)
    with open(args.out, "w") as out:  # (written once, at the end: a run that fails midway leaves no truncated file)
        out.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
