"""Time the pseudo-labelling criterion (``functional.pseudo_label_ce``, csrc/pseudo_label.hip) at the reference's batch shape
(10 x 4 x 224 x 224 class maps), forward + backward, each variant replayed from a captured graph:

* the fused launch with fixed thresholds and with self-adaptive ones (the threshold update rides in the same launch);
* (a) the same arithmetic in plain torch ops on the same device tensors: per-sample flips, softmax, max, the compare against
  ``tau[y]``, ``cross_entropy(reduction="none")``, mask, mean, autograd's backward; for the adaptive variant also the two
  means and the moving-average arithmetic on the float64 state -- the baseline: no earlier version of this project runs
  this criterion;
* (b) ``functional.consistency_softmax_mse`` at the same shape: the sibling that reads the same two maps and writes the same
  gradient.

and the whole semi-supervised step (``--dtype``, bf16 by default; 5 labelled + 5 + 5 unlabelled slices of
224 x 224) without a hook, with the consistency hook and with this hook (``self`` fixed, ``self`` adaptive, ``ema``).

Device events around replays (criterion) or eager steps (whole step); everything is warmed up first; the variants are timed
in alternating order, the order rotating from round to round, and every round is printed so that the spread shows.
``--lib`` times another build of the library (one compiled with ``-DSPCL_PSEUDO_LABEL_CLOSE=0`` skips the sums of the close:
the difference is the close's cost); ``--part`` selects what is timed.

    python tools/diag/pseudo_label_step_time.py [--reps 200] [--rounds 4] [--part all|criterion|fused|step]
        [--dtype bf16|fp32] [--lib PATH]"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
DEV = "cuda:0"
SHAPE = (10, 4, 224, 224)
FLAGS = [3, 0, 1, 2, 0, 3, 1, 2, 0, 3]
THRESHOLD, MOMENTUM = 0.6, 0.999


def _events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _captured(fn, warmup=3):
    """``fn`` warmed up on a side stream and captured: -> the graph (replay() repeats its launches)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph


def _flip_torch(x, flags):
    out = []
    for v, f in zip(x, flags):
        if f & 1:
            v = v.flip(-2)
        if f & 2:
            v = v.flip(-1)
        out.append(v)
    return torch.stack(out, dim=0)


def _criterion_variants(part):
    from spcl_amd import functional as F_hip
    g = torch.Generator().manual_seed(11)

    def cl(x):
        return x.to(DEV).contiguous(memory_format=torch.channels_last)

    teacher, student = cl(3.0 * torch.randn(*SHAPE, generator=g)), cl(torch.randn(*SHAPE, generator=g))
    flags = torch.tensor(FLAGS, dtype=torch.uint8, device=DEV)
    unit = F_hip.register_unit_gradient(torch.ones((), device=DEV))
    C, M = SHAPE[1], SHAPE[0] * SHAPE[2] * SHAPE[3]
    tau_fixed = torch.full((C,), THRESHOLD, device=DEV)
    tau_a, state_a = F_hip.pseudo_label_state(C, DEV)
    tau_t, state_t = F_hip.pseudo_label_state(C, DEV)
    kept = {}

    def fused(tau, state):
        def run():
            x = student.detach().requires_grad_(True)
            out = []
            F_hip.pseudo_label_ce(teacher, x, tau, 1.0, flags, state=state, momentum=MOMENTUM, out=out).backward(gradient=unit)
            if state is None:
                kept["fused"] = out[1]
        return run

    def consistency():
        x = student.detach().requires_grad_(True)
        F_hip.consistency_softmax_mse(teacher, x, 1.0, flags).backward(gradient=unit)

    def torch_ops(tau, state):
        def run():
            x = student.detach().requires_grad_(True)
            q = _flip_torch(teacher, FLAGS).softmax(1)
            conf, y = q.max(1)
            keep = conf >= tau[y]
            ce = torch.nn.functional.cross_entropy(x, y, reduction="none")
            (ce * keep).mean().backward()
            if state is None:
                kept["torch"] = keep.sum()
            else:
                stats = torch.cat([conf.double().mean().reshape(1), q.double().mean((0, 2, 3))])
                state.mul_(MOMENTUM).add_(stats, alpha=1.0 - MOMENTUM)
                tau.copy_(state[1:] / state[1:].max() * state[0])
        return run

    variants = [("fused, fixed thresholds", fused(tau_fixed, None)), ("fused, adaptive thresholds", fused(tau_a, state_a))]
    if part != "fused":
        variants += [("consistency_softmax_mse", consistency), ("torch ops, fixed", torch_ops(tau_fixed, None)),
                     ("torch ops, adaptive", torch_ops(tau_t, state_t))]
    graphs = [(name, _captured(fn)) for name, fn in variants]
    note = f"at the fixed thresholds the fused launch keeps {int(kept['fused'][C:].sum())} of {M} pixels"
    if "torch" in kept:
        note += f", torch's mask {int(kept['torch'])}"
    return graphs, note


def _batch(n, size, seed):
    g = torch.Generator().manual_seed(seed)
    img, img_tf = torch.rand(n, 1, size, size, generator=g), torch.rand(n, 1, size, size, generator=g)
    tgt = torch.randint(0, 4, (n, 1, size, size), generator=g)
    names = [f"patient{k:03d}_00_{k}" for k in range(n)]
    return (tuple(t.to(DEV) for t in (img, img_tf, tgt, tgt.clone())), names, (["0"] * n, names))


def _epocher(hook_of, dtype):
    from spcl_amd import ddp
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.optim import FusedRAdam
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.epochers.semi import SemiSupervisedEpocher
    torch.manual_seed(0)
    model = UNet(input_dim=1, num_classes=4).to(DEV).train()
    model.set_compute_dtype(dtype)
    hooks = [h.to(DEV) for h in hook_of(model)]
    flat = ddp.FlatParams([p for p in model.parameters() if p.requires_grad] +
                          [p for h in hooks for p in h.parameters() if p.requires_grad])
    opt = FusedRAdam([flat.param], lr=1e-6, weight_decay=1e-5)
    ep = SemiSupervisedEpocher(model=model, optimizer=opt, labeled_loader=[], unlabeled_loader=[], sup_criterion=KL_div(),
                               num_batches=1, device=DEV, flat_params=flat)
    ep.add_hooks([h() for h in hooks])
    return ep


def _step_variants(dtype):
    from spcl_amd.semi_seg import hooks as H
    lab, unl = _batch(5, 224, 1), _batch(5, 224, 2)
    makers = [("no hook", lambda m: []),
              ("consistency", lambda m: [H.create_consistency_hook(weight=1.0)]),
              ("pseudolabel self fixed", lambda m: [H.create_pseudo_label_hook(model=m, weight=1.0, threshold=0.3)]),
              ("pseudolabel self adaptive", lambda m: [H.create_pseudo_label_hook(model=m, weight=1.0, adaptive=True)]),
              ("pseudolabel ema", lambda m: [H.create_pseudo_label_hook(model=m, weight=1.0, threshold=0.3, teacher="ema")])]
    out = []
    for name, maker in makers:
        ep = _epocher(maker, dtype)

        def step(ep=ep):
            with ep.meters.focus_on(ep.meter_focus):
                ep.step(lab, unl, seed=7)

        for _ in range(3):
            step()
        torch.cuda.synchronize()
        out.append((name, step))
    return out


def _rounds(variants, reps, rounds, unit, scale):
    """every variant once per round, the order rotating; -> the lines and {name: [per-round figures]}"""
    lines, table = [], {name: [] for name, _ in variants}
    for r in range(rounds):
        order = variants[r % len(variants):] + variants[:r % len(variants)]
        for name, fn in order:
            table[name].append(_events(fn, reps) * scale)
        lines.append(f"round {r}: " + ", ".join(f"{name} {table[name][-1]:.1f} {unit}" for name, _ in variants))
    lines.append("min .. max: " + ", ".join(f"{name} {min(v):.1f} .. {max(v):.1f} {unit}" for name, v in table.items()))
    return lines, table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--part", choices=("all", "criterion", "fused", "step"), default="all")
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16", help="compute dtype of the whole step")
    ap.add_argument("--lib", default=None, help="another build of libspcl_hip.so to time")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pseudo_label_step_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pseudo_label_step_time.py measures on the GPU: no device found")
    import spcl_amd  # noqa: F401
    from spcl_amd import native
    if args.lib:
        native.LIB_PATH = os.path.abspath(args.lib)
    lines = [f"library {os.path.relpath(native.LIB_PATH, REPO)}"]
    if args.part != "step":
        M = SHAPE[0] * SHAPE[2] * SHAPE[3]
        graphs, note = _criterion_variants(args.part)
        lines.append(f"criterion, forward + backward, class maps {' x '.join(map(str, SHAPE))} f32 channels-last, threshold "
                     f"{THRESHOLD}, momentum {MOMENTUM}; graph replays, {args.reps} per figure; {note}; the fused launch moves "
                     f"at most {(3 * M * SHAPE[1] * 4 + M) / 1e6:.1f} MB")
        lines += _rounds([(name, g.replay) for name, g in graphs], args.reps, args.rounds, "us", 1e3)[0]
    if args.part in ("all", "step"):
        steps = _step_variants(torch.bfloat16 if args.dtype == "bf16" else torch.float32)
        lines.append(f"semi-supervised step, compute dtype {args.dtype}, batch 5 + 5 + 5 x 1 x 224 x 224, eager, "
                     f"{max(10, args.reps // 5)} steps per figure")
        lines += _rounds(steps, max(10, args.reps // 5), args.rounds, "us", 1e3)[0]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
