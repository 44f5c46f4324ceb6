"""Time the mix-up baseline at the reference's batch shape (config/base.yaml: 5 labelled slices of 224 x 224 and their second
views, UNet of 16 .. 256 channels, 4 classes):

* the two launches alone -- ``spcl_mixup_images`` over 5 + 5 x 1 x 224 x 224 and ``spcl_mixup_kl_onehot`` (loss + gradient of
  the logits) over 10 x 4 x 224 x 224 --;
* the same work in the reference's torch formulation on the same tensors (semi_seg/hooks/mixup.py:19-32,66-77): two int64
  one-hot maps, the concatenations, the gathers by the permutation, the blends, softmax, ``KL_div`` with its simplex
  assertions, ``.item()`` and autograd's backward to the logits -- the baseline: no earlier version of this project runs
  mix-up;
* the ``MixUpEpocher`` step with the hook against the hook-less ``FineTuneEpocher`` step (eager launches both).

Device events around replayed calls; every shape is warmed up first; each figure is the mean of ``--reps`` repetitions, the
whole measurement is repeated ``--rounds`` times in one process so that the spread shows.

    python tools/diag/mixup_step_time.py [--reps 30] [--rounds 3]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
DEV = "cuda:0"
LAM, SEED = 0.23538938957272115, 7


def _time(fn, reps, warmup=3):
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


def _batch(n, size, seed):
    g = torch.Generator().manual_seed(seed)
    img, img_tf = torch.rand(n, 1, size, size, generator=g), torch.rand(n, 1, size, size, generator=g)
    tgt, tgt_tf = torch.randint(0, 4, (n, 1, size, size), generator=g), torch.randint(0, 4, (n, 1, size, size), generator=g)
    names = [f"patient{k:03d}_00_{k}" for k in range(n)]
    return (tuple(t.to(DEV) for t in (img, img_tf, tgt, tgt_tf)), names, (["0"] * n, names))


def _kernel_times(reps):
    from spcl_amd import functional as F_hip
    (img, img_tf, tgt, tgt_tf), _, _ = _batch(5, 224, 1)
    g = torch.Generator().manual_seed(2)
    logits = torch.randn(10, 4, 224, 224, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    index = torch.randperm(10, generator=g)
    plan = F_hip.MixupPlan(index, LAM, DEV)
    index_dev = index.to(DEV)
    unit = F_hip.register_unit_gradient(torch.ones((), device=DEV))

    def one_hot(seg):  # deepclustering2 class2one_hot: an int64 [B, C, H, W] map
        return torch.nn.functional.one_hot(seg.squeeze(1), 4).permute(0, 3, 1, 2)

    def simplex(t):
        s = t.sum(1).float()
        return bool(torch.allclose(s, torch.ones_like(s)))

    def kl_div(prob, target, eps=1e-16):  # deepclustering2 KL_div(reduction="mean") in torch ops
        return (-target * torch.log((prob + eps) / (target + eps))).sum(1).mean()

    def images():
        F_hip.mixup_images(img, img_tf, plan)

    def kl():
        x = logits.detach().requires_grad_(True)
        F_hip.mixup_kl_onehot(x, tgt, tgt_tf, plan).backward(gradient=unit)

    def torch_images():
        x = torch.cat([img, img_tf], dim=0)
        return LAM * x + (1 - LAM) * x[index_dev, :]

    def torch_targets():
        y = torch.cat([one_hot(tgt), one_hot(tgt_tf)], dim=0)
        return LAM * y + (1 - LAM) * y[index_dev, :]

    def torch_kl(asserts):
        x = logits.detach().requires_grad_(True)
        prob, target = x.softmax(1), torch_targets().squeeze()
        if asserts:
            assert simplex(prob) and simplex(target)
        loss = kl_div(prob, target)
        if asserts:
            loss.item()  # (mixup.py:76)
        loss.backward()

    return {"mixup_images": _time(images, reps * 10), "mixup_kl_onehot + backward": _time(kl, reps * 10),
            "torch cat / gather / blend of the images": _time(torch_images, reps),
            "torch one-hot / cat / gather / blend / softmax / KL_div / backward": _time(lambda: torch_kl(False), reps),
            "the same with KL_div's assertions and .item()": _time(lambda: torch_kl(True), reps)}


def _step_times(reps):
    from spcl_amd import ddp
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.optim import FusedRAdam
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.epochers.finetune import FineTuneEpocher
    from spcl_amd.semi_seg.epochers.mixup import MixUpEpocher
    from spcl_amd.semi_seg.hooks.mixup import MixUpHook
    lab = _batch(5, 224, 3)
    out = {}
    for name in ("fine-tune step (no hook, eager)", "mix-up step"):
        torch.manual_seed(0)
        model = UNet(input_dim=1, num_classes=4).to(DEV).train()
        flat = ddp.FlatParams([p for p in model.parameters() if p.requires_grad])
        opt = FusedRAdam([flat.param], lr=1e-6, weight_decay=1e-5)
        if name.startswith("fine-tune"):
            ep = FineTuneEpocher(model=model, optimizer=opt, labeled_loader=[], sup_criterion=KL_div(), num_batches=1,
                                 device=DEV, flat_params=flat, graph=False)
            with ep.meters.focus_on(ep.meter_focus):
                out[name] = _time(lambda: ep.step(lab), reps)
        else:
            ep = MixUpEpocher(model=model, optimizer=opt, labeled_loader=[], unlabeled_loader=None, sup_criterion=KL_div(),
                              num_batches=1, device=DEV, flat_params=flat)
            ep.add_hooks([MixUpHook(hook_name=f"mx_hook_time_{len(_step_times.names)}", weight=0.01)()])
            _step_times.names.append(name)
            with ep.meters.focus_on(ep.meter_focus):
                out[name] = _time(lambda: ep.step(lab, seed=SEED), reps)
            ep.close_hooks()
        del ep
    return out


_step_times.names = []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mixup_step_time.py measures on the GPU: no device found")
    import spcl_amd  # noqa: F401
    from spcl_amd import config as _config
    print(f"compute dtype {_config.get_compute_dtype()}, batch 5 + 5 x 1 x 224 x 224, logits 10 x 4 x 224 x 224, "
          f"{args.reps} reps per figure (x 10 for the two launches)")
    for r in range(args.rounds):
        k = _kernel_times(args.reps)
        gbs = 12.0 * 10 * 224 * 224 / (k["mixup_images"] * 1e-3) / 1e9
        print(f"round {r}: " + ", ".join(f"{a} {v * 1e3:.1f} us" for a, v in k.items()) +
              f" (mixup_images: {gbs:.0f} GB/s of 12 B/element)")
        s = _step_times(args.reps)
        base, mix = s["fine-tune step (no hook, eager)"], s["mix-up step"]
        print(f"round {r}: " + ", ".join(f"{a} {v:.3f} ms" for a, v in s.items()) + f" (mix-up +{mix - base:.3f} ms)")


if __name__ == "__main__":
    main()
