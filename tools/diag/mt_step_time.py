"""Time the semi-supervised step with the mean-teacher hook, with the entropy-minimisation hook and without a hook, at the
reference's batch shape (config/base.yaml: 5 labelled + 5 unlabelled slices of 224 x 224, UNet of 16 .. 256 channels, 4
classes), and the teacher's moving average alone in three forms over the UNet's parameters: the single launch over the two
flat buffers (``spcl_ema_update``, what the hook does under ``SemiTrainer``), one launch per parameter tensor (the hook on a
model whose parameters are not one flat buffer), and the reference's formulation in torch ops (``mul_``, ``add_``, ``mul_``
per parameter tensor: deepclustering2 ``ema_updater``) -- the baseline: no earlier version of this project runs a mean
teacher.

Device events around replayed eager steps (the semi step is not captured in a hipGraph); every shape is warmed up first;
each figure is the mean of ``--reps`` repetitions, the whole measurement is repeated ``--rounds`` times so that the spread
shows.

    python tools/diag/mt_step_time.py [--reps 30] [--rounds 3]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
DEV = "cuda:0"


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
    tgt = torch.randint(0, 4, (n, 1, size, size), generator=g)
    names = [f"patient{k:03d}_00_{k}" for k in range(n)]
    batch = (tuple(t.to(DEV) for t in (img, img_tf, tgt, tgt.clone())), names, (["0"] * n, names))
    return batch


def _epocher(section, params):
    from spcl_amd import ddp
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.optim import FusedRAdam
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.epochers.semi import SemiSupervisedEpocher
    torch.manual_seed(0)
    model = UNet(input_dim=1, num_classes=4).to(DEV).train()
    cfg = {"Data": {"name": "acdc"}, "Trainer": {"max_epoch": 2}}
    if section:
        cfg[section] = params
    hooks = create_hook_from_config(model, cfg)
    for h in hooks:
        h.to(DEV)
    flat = ddp.FlatParams([p for p in model.parameters() if p.requires_grad] +
                          [p for h in hooks for p in h.parameters() if p.requires_grad])
    opt = FusedRAdam([flat.param], lr=1e-6, weight_decay=1e-5)
    ep = SemiSupervisedEpocher(model=model, optimizer=opt, labeled_loader=[], unlabeled_loader=[], sup_criterion=KL_div(),
                               num_batches=1, device=DEV, flat_params=flat)
    ep.add_hooks([h() for h in hooks])
    return ep


def _step_times(reps):
    out = {}
    lab, unl = _batch(5, 224, 1), _batch(5, 224, 2)
    for name, section, params in (("no hook", None, None),
                                  ("entropy", "EntropyMinParameters", {"weight": 0.1}),
                                  ("meanteacher", "MeanTeacherParameters",
                                   {"name": "mse", "weight": 10, "alpha": 0.999, "weight_decay": 1e-6})):
        ep = _epocher(section, params)
        with ep.meters.focus_on(ep.meter_focus):
            out[name] = _time(lambda: ep.step(lab, unl, seed=7), reps)
        ep.close_hooks()
        del ep
    return out


def _ema_times(reps):
    from spcl_amd import functional as F_hip
    from spcl_amd.semi_seg.arch import UNet
    torch.manual_seed(0)
    shapes = [p.shape for p in UNet(input_dim=1, num_classes=4).parameters()]
    n = sum(s.numel() for s in shapes)
    tflat, sflat = torch.randn(n, device=DEV), torch.randn(n, device=DEV)

    def views(flat):
        out, off = [], 0
        for s in shapes:
            out.append(flat[off:off + s.numel()].view(s))
            off += s.numel()
        return out

    tv, sv = views(tflat), views(sflat)
    alpha, decay = 0.999, 1e-6

    def single():
        F_hip.ema_update_(tflat, sflat, alpha, decay)

    def per_tensor():
        for t, s in zip(tv, sv):
            F_hip.ema_update_(t, s, alpha, decay)

    def torch_ops():
        for t, s in zip(tv, sv):
            t.mul_(alpha).add_(s, alpha=1 - alpha)
            t.mul_(1 - decay)

    res = {"single launch": _time(single, reps * 10), "per-tensor launches": _time(per_tensor, reps),
           "torch ops per tensor": _time(torch_ops, reps)}
    return len(shapes), n, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mt_step_time.py measures on the GPU: no device found")
    import spcl_amd  # noqa: F401
    from spcl_amd import config as _config
    print(f"compute dtype {_config.get_compute_dtype()}, batch 5 + 5 + 5 x 1 x 224 x 224, {args.reps} reps per figure")
    for r in range(args.rounds):
        steps = _step_times(args.reps)
        base = steps["no hook"]
        print(f"round {r}: semi step " + ", ".join(f"{k} {v:.3f} ms" for k, v in steps.items()) +
              f" (entropy +{steps['entropy'] - base:.3f}, meanteacher +{steps['meanteacher'] - base:.3f})")
        k, n, ema = _ema_times(args.reps)
        gbs = 12.0 * n / (ema["single launch"] * 1e-3) / 1e9
        print(f"round {r}: EMA of {k} tensors / {n} parameters: " + ", ".join(f"{a} {v * 1e3:.1f} us" for a, v in ema.items()) +
              f" (single launch: {gbs:.0f} GB/s of 12 B/element)")


if __name__ == "__main__":
    main()
