"""Time the PICA criteria (csrc/pica.hip) at the UDA-IIC reference sizes -- 5 unlabelled slices and their transformed copies,
5 subheads x 20 clusters -- with their backward:

* ``dense_p1`` / ``dense_p3``: ``functional.pica_loss`` at ``Up_conv3`` (112 x 112), padding 1 / 3, against the plain torch
  formulation on the same device (the reference's ``PUISegLoss`` arithmetic, f32: tests/_pica_oracle.py) and against
  ``functional.iic_loss`` at the same shape (the two share the joint launches);
* ``global``: the same three at ``Conv5`` (pooled feature: [5, 100] logits);
* ``step_bf16``: one whole ``SemiSupervisedEpocher`` step (5 + 5 slices of 224 x 224, bf16, flat parameters, fused RAdam)
  without a hook, with the ``Conv5`` hook and with the ``Up_conv3`` hook (padding 1).

Each step runs in a child process of its own under ``timeout``; the first child that ends with a non-zero status ends the run
(nothing more is started on the device) and the status is handed on.  Every figure is the mean of its repetitions after a
warm-up; the whole list of steps is run ``--rounds`` times so that the spread shows.  No pass / fail bar.

    python tools/diag/pica_step_time.py [--reps 20] [--rounds 2] [--out profiles/pica_step_time.txt]"""
import argparse
import os
import subprocess
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
DEV = "cuda:0"
N, S, K, HW = 5, 5, 20, 224
FLAGS = [1, 0, 3, 2, 1]
STEPS = (("dense_p1", 240), ("dense_p3", 420), ("global", 120), ("step_bf16", 300))  # (step, its time limit in seconds)


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


def _criteria(say, reps, dense, pad):
    from spcl_amd import functional as F_hip
    from tests import _iic_oracle as R
    from tests import _pica_oracle as P
    size = 112 if dense else 1
    g = torch.Generator().manual_seed(1)
    lx = torch.randn(N, S * K, size, size, generator=g).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    ly = torch.randn(N, S * K, size, size, generator=g).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    flags = torch.tensor(FLAGS, dtype=torch.uint8, device=DEV) if dense else None
    first = {}

    def pica():
        out = []
        loss = F_hip.pica_loss(lx, ly, num_subheads=S, num_clusters=K, padding=pad, dense=dense, scale=1.0 / S, flags=flags, out=out)
        loss.backward()
        first.setdefault("pica", (loss.detach(), out[0]))

    def iic():
        loss = F_hip.iic_loss(lx, ly, num_subheads=S, num_clusters=K, padding=pad, dense=dense, scale=1.0 / S, flags=flags)
        loss.backward()

    def torch_ops():
        px = R.grouped_softmax(R.flip(lx, FLAGS) if dense else lx, S, K)
        py = R.grouped_softmax(ly, S, K)
        if dense:
            terms = [P.pui_seg_loss(a, b, pad) for a, b in zip(px, py)]
        else:
            terms = [P.pui_loss(a.flatten(1), b.flatten(1)) for a, b in zip(px, py)]
        loss = sum(t[0] for t in terms) / S
        loss.backward()
        first.setdefault("torch", (loss.detach(), sum(t[1] for t in terms).detach() / S))

    tp, ti = _time(pica, reps), _time(iic, reps)
    tt = _time(torch_ops, 3 if dense else reps, warmup=1)
    where = f"Up_conv3 ({N} x {S * K} x 112 x 112), padding {pad}" if dense else f"Conv5 ([{N}, {S * K}] logits)"
    say(f"{where}: one call forward + backward: pica_loss {tp * 1e3:.0f} us, iic_loss {ti * 1e3:.0f} us, torch formulation "
        f"{tt * 1e3:.0f} us; pica / iic = {tp / ti:.2f}, pica / torch = {tp / tt:.3f}; loss / ce: kernel "
        f"{float(first['pica'][0]):.6f} / {float(first['pica'][1]):.6f}, torch {float(first['torch'][0]):.6f} / "
        f"{float(first['torch'][1]):.6f}")


def _whole_steps(say, reps):
    from spcl_amd import config
    from spcl_amd import ddp as _ddp
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.optim import FusedRAdam
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.epochers.semi import SemiSupervisedEpocher
    from spcl_amd.semi_seg.hooks import create_pica_hooks

    def batch(seed):
        g = torch.Generator().manual_seed(seed)
        img, img_tf = torch.rand(N, 1, HW, HW, generator=g).to(DEV), torch.rand(N, 1, HW, HW, generator=g).to(DEV)
        tgt = torch.randint(0, 4, (N, 1, HW, HW), generator=g).to(DEV)
        names = [f"patient{k:03d}_00_{k}" for k in range(N)]
        return (img, img_tf, tgt, tgt.clone()), names, (["0"] * N, names)

    lab, unl = batch(1), batch(2)
    before = config.get_compute_dtype()
    config.set_compute_dtype(torch.bfloat16)
    try:
        res = {}
        for kind, feature, pads in (("no hook", None, []), ("Conv5 hook", "Conv5", []), ("Up_conv3 hook (padding 1)", "Up_conv3", [1])):
            torch.manual_seed(3)
            model = UNet(input_dim=1, num_classes=4).to(DEV).train()
            model.set_compute_dtype(torch.bfloat16)
            params = list(model.parameters())
            hooks = []
            if feature:
                th = create_pica_hooks(model=model, feature_names=[feature], weights=[0.1], paddings=pads)
                th.to(DEV)
                params += list(th.parameters())
                hooks = [th()]
            flat = _ddp.FlatParams(params)
            opt = FusedRAdam([flat.param], lr=1e-7, weight_decay=1e-5)
            ep = SemiSupervisedEpocher(model=model, optimizer=opt, labeled_loader=[], unlabeled_loader=[], sup_criterion=KL_div(),
                                       num_batches=1, device=DEV, flat_params=flat)
            ep.add_hooks(hooks)
            with ep.meters.focus_on(ep.meter_focus):
                res[kind] = _time(lambda: ep.step(lab, unl, seed=1), reps)
            ep.close_hooks()
        say(f"whole SemiSupervisedEpocher step at {N} + {N} slices of {HW} x {HW}, bf16: "
            + ", ".join(f"{k} {v:.2f} ms" for k, v in res.items()))
    finally:
        config.set_compute_dtype(before)


def _run_step(step, reps):
    import spcl_amd  # noqa: F401

    def say(text):
        print(text, flush=True)

    if step == "dense_p1":
        _criteria(say, reps, True, 1)
    elif step == "dense_p3":
        _criteria(say, reps, True, 3)
    elif step == "global":
        _criteria(say, reps, False, 0)
    elif step == "step_bf16":
        _whole_steps(say, reps)
    else:
        raise SystemExit(f"unknown step {step!r}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--step", default=None, help="run this one step in this process (what the driver starts)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pica_step_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pica_step_time.py measures on the GPU: no device found")
    if args.step:
        return _run_step(args.step, args.reps)
    lines = [f"PICA criteria on the logits of {N} unlabelled slices and their transformed copies, {S} subheads x {K} clusters; "
             f"{args.reps} reps per figure (3 for the dense torch formulation)"]
    print(lines[0], flush=True)
    status = 0
    for rnd, (step, limit) in ((r, s) for r in range(args.rounds) for s in STEPS):
        if step == STEPS[0][0]:
            lines.append(f"round {rnd}")
            print(lines[-1], flush=True)
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step,
                            "--reps", str(args.reps)], stdout=subprocess.PIPE, text=True)
        got = [ln for ln in r.stdout.splitlines() if ln.strip()]
        print("\n".join(got), flush=True)
        lines += got
        if r.returncode != 0:
            status = r.returncode
            lines.append(f"step {step} ended with status {status}: stopped here, the steps after it were not run")
            print(lines[-1], flush=True)
            break
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        out.write("\n".join(lines) + "\n")
    sys.exit(status)


if __name__ == "__main__":
    main()
