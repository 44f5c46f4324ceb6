"""Time cross pseudo supervision (``functional.cross_pseudo_ce``, csrc/cross_pseudo.hip; semi_seg/hooks/cps.py).

Criterion, forward + backward of BOTH class maps, at 10 x 4 x 224 x 224 and 32 x 4 x 224 x 224, replayed from a captured graph
and as call + synchronise:

* (a) the fused launch ``cross_pseudo_ce`` (no thresholds: plain CPS);
* (b) the two-call composition ``pseudo_label_ce(b -> a) + pseudo_label_ce(a -> b)`` with ``tau = 0``: the same arithmetic
  from what the package already had (both maps read twice, both soft-maxes formed twice, two launches, two memsets);
* (c) the plain torch formulation: two ``softmax``, two ``argmax``, two ``F.cross_entropy``, masks, autograd's backward.

Whole step: one eager ``SemiSupervisedEpocher`` step (``--dtype``, bf16 by default; 5 labelled + 5 + 5 unlabelled slices of
224 x 224, the sizes of tools/diag/pseudo_label_step_time.py) without a hook and with the CPS hook.  ``--parent ROOT`` times the
hook-less step of this tree and of another checkout (the parent commit, built) in alternating child processes.

Device events around replays or eager steps, a host clock around call + synchronise; everything is warmed up first; the
variants are timed in alternating order, the order rotating from round to round, and every round is printed so that the
spread shows.

    python tools/diag/cps_time.py [--reps 200] [--rounds 4] [--part all|criterion|step|nohook] [--dtype bf16|fp32]
        [--parent ROOT] [--root ROOT]"""
import argparse
import os
import subprocess
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"
SHAPES = ((10, 4, 224, 224), (32, 4, 224, 224))


def _events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _call_sync(fn, reps):
    """host clock around ``fn(); synchronize()``, per call, in ms"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


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


def _criterion_variants(shape):
    """-> [(name, eager callable)], a note on what the three variants computed"""
    from spcl_amd import functional as F_hip
    g = torch.Generator().manual_seed(23)

    def cl(x):
        return x.to(DEV).contiguous(memory_format=torch.channels_last)

    a, b = cl(3.0 * torch.randn(*shape, generator=g)), cl(3.0 * torch.randn(*shape, generator=g))
    unit = F_hip.register_unit_gradient(torch.ones((), device=DEV))
    zeros = torch.zeros(shape[1], device=DEV)
    seen = {}

    def fused():
        x, y = a.detach().requires_grad_(True), b.detach().requires_grad_(True)
        loss = F_hip.cross_pseudo_ce(x, y)
        loss.backward(gradient=unit)
        seen["fused"] = (loss.detach(), x.grad, y.grad)

    def two_calls():
        x, y = a.detach().requires_grad_(True), b.detach().requires_grad_(True)
        loss = F_hip.pseudo_label_ce(b, x, zeros) + F_hip.pseudo_label_ce(a, y, zeros)
        loss.backward(gradient=unit)
        seen["two calls"] = (loss.detach(), x.grad, y.grad)

    def torch_ops():
        x, y = a.detach().requires_grad_(True), b.detach().requires_grad_(True)
        with torch.no_grad():
            pa, pb = x.softmax(1), y.softmax(1)
            ya, yb = x.argmax(1), y.argmax(1)
            keep_a, keep_b = pa.max(1).values >= 0.0, pb.max(1).values >= 0.0
        ce = torch.nn.functional.cross_entropy
        loss = (ce(x, yb, reduction="none") * keep_b).mean() + (ce(y, ya, reduction="none") * keep_a).mean()
        loss.backward()
        seen["torch"] = (loss.detach(), x.grad, y.grad)

    variants = [("(a) cross_pseudo_ce", fused), ("(b) 2 x pseudo_label_ce", two_calls), ("(c) torch ops", torch_ops)]
    for _, fn in variants:
        fn()
    torch.cuda.synchronize()
    ref = seen["fused"]
    note = []
    for key in ("two calls", "torch"):
        loss, gx, gy = seen[key]
        note.append(f"{key}: loss rel {abs(float(loss) - float(ref[0])) / abs(float(ref[0])):.1e}, gradients rel L2 "
                    f"{float((gx - ref[1]).norm() / ref[1].norm()):.1e} / {float((gy - ref[2]).norm() / ref[2].norm()):.1e}")
    eager = {key: float(v[0]) for key, v in seen.items()}

    def replays_write_their_loss(graphs):
        """after the timed rounds: zero each captured loss, replay once more, and compare with the eager value -- a replay
        whose closing workgroup did not run would leave the zero"""
        found = []
        for (name, replay), key in zip(graphs, ("fused", "two calls", "torch")):
            seen[key][0].zero_()
            replay()
            torch.cuda.synchronize()
            ok = float(seen[key][0]) == eager[key]
            found.append(f"{name} {'wrote the eager value again' if ok else 'did NOT write its loss (' + repr(float(seen[key][0])) + ')'}")
        return "after the timed replays each captured loss was zeroed and one more replay run: " + ", ".join(found)

    return variants, "against (a): " + "; ".join(note), replays_write_their_loss


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


def _step_variants(dtype, with_hook=True):
    from spcl_amd.semi_seg import hooks as H
    lab, unl = _batch(5, 224, 1), _batch(5, 224, 2)
    makers = [("no hook", lambda m: [])]
    if with_hook:
        makers += [("cps", lambda m: [H.create_cross_pseudo_hook(model=m, weight=1.5)]),
                   ("cps, threshold 0.3, unlabelled maps", lambda m: [H.create_cross_pseudo_hook(
                       model=m, weight=1.5, threshold=0.3, on=("unlabeled", "unlabeled_tf"))])]
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


def _rounds(variants, timer, reps, rounds, unit, scale):
    """every variant once per round, the order rotating; -> the lines and {name: [per-round figures]}"""
    lines, table = [], {name: [] for name, _ in variants}
    for r in range(rounds):
        order = variants[r % len(variants):] + variants[:r % len(variants)]
        for name, fn in order:
            table[name].append(timer(fn, reps) * scale)
        lines.append(f"round {r}: " + ", ".join(f"{name} {table[name][-1]:.1f} {unit}" for name, _ in variants))
    lines.append("min .. max: " + ", ".join(f"{name} {min(v):.1f} .. {max(v):.1f} {unit}" for name, v in table.items()))
    return lines, table


def _parent_rounds(args):
    """the hook-less step of this tree and of ``args.parent``, one child process per figure set, alternating"""
    lines = [f"hook-less semi-supervised step, compute dtype {args.dtype}, this tree against {args.parent_name}: child "
             f"processes in alternating order, each {args.rounds} figures of {max(10, args.reps // 5)} eager steps"]
    for k in range(2 * args.children):
        root, name = ((REPO, "this tree"), (os.path.abspath(args.parent), args.parent_name))[k % 2]
        cmd = [sys.executable, os.path.abspath(__file__), "--part", "nohook", "--root", root, "--reps", str(args.reps),
               "--rounds", str(args.rounds), "--dtype", args.dtype, "--out", ""]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if done.returncode != 0:
            raise SystemExit(f"child {k} ({name}) failed ({done.returncode}):\n{done.stdout}")
        figures = [line for line in done.stdout.splitlines() if line.startswith("min .. max")]
        lines.append(f"child {k}, {name}: {figures[-1]}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--part", choices=("all", "criterion", "step", "nohook"), default="all")
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16", help="compute dtype of the whole step")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its hook-less step is timed too")
    ap.add_argument("--parent-name", default="the parent commit")
    ap.add_argument("--children", type=int, default=2, help="child processes per tree for --parent")
    ap.add_argument("--root", default=REPO, help="the checkout whose package is imported")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cps_time.txt"))
    args = ap.parse_args()
    lines = []
    if args.parent and args.part in ("all", "step"):  # children first: this process has not opened the device yet
        lines += _parent_rounds(args)
    sys.path.insert(0, os.path.abspath(args.root))
    if not torch.cuda.is_available():
        raise SystemExit("cps_time.py measures on the GPU: no device found")
    import spcl_amd  # noqa: F401
    from spcl_amd import native
    lines.insert(0, f"library {os.path.relpath(native.LIB_PATH, os.path.abspath(args.root))}, C ABI {native.ABI_VERSION}")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    if args.part in ("all", "criterion"):
        for shape in SHAPES:
            variants, note, check = _criterion_variants(shape)
            M = shape[0] * shape[2] * shape[3]
            lines.append(f"criterion, forward + backward of both class maps {' x '.join(map(str, shape))} f32 channels-last, no "
                         f"thresholds; {note}; (a) moves {4 * M * shape[1] * 4 / 1e6:.1f} MB")
            graphs = [(name, _captured(fn).replay) for name, fn in variants]
            lines.append(f"graph replays, {args.reps} per figure")
            lines += _rounds(graphs, _events, args.reps, args.rounds, "us", 1e3)[0]
            lines.append(check(graphs))
            lines.append(f"call + synchronise (host clock), {args.reps} per figure")
            lines += _rounds(variants, _call_sync, args.reps, args.rounds, "us", 1e3)[0]
    if args.part in ("all", "step", "nohook"):
        steps = _step_variants(dtype, with_hook=args.part != "nohook")
        n = max(10, args.reps // 5)
        lines.append(f"semi-supervised step, compute dtype {args.dtype}, batch 5 + 5 + 5 x 1 x 224 x 224, eager, {n} steps per "
                     "figure")
        step_lines, table = _rounds(steps, _events, n, args.rounds, "us", 1e3)
        lines += step_lines
        if "cps" in table:
            base = min(table["no hook"])
            lines.append("factor over the hook-less step (minima): " + ", ".join(
                f"{name} {min(v) / base:.2f}x" for name, v in table.items() if name != "no hook"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
