"""Time CutMix for cross pseudo supervision (csrc/cutmix.hip: ``functional.cutmix_boxes``, ``cutmix_images``,
``cross_pseudo_ce_mixed``; semi_seg/hooks/cps.py with ``"cutmix"`` in ``on``).

Criterion, forward + backward of BOTH student maps, at 10 x 4 x 224 x 224 and 32 x 4 x 224 x 224, boxes of seed 23 at the range
(0.25, 0.5), roll 1, replayed from a captured graph and as call + synchronise:

* (a) the fused launch ``cross_pseudo_ce_mixed`` (no thresholds), the teachers read through the boxes;
* (b) the composition from the package's ops: two ``torch.where`` gathers of the teacher maps, then ``pseudo_label_ce(where(t_b),
  s_a, zeros)`` and the mirrored call (each teacher map read and written once more, both soft-maxes formed twice);
* (c) the plain torch formulation: the two gathers, two ``softmax``, two ``argmax``, two ``F.cross_entropy``, autograd.

The box launch alone, and the image mix against ``torch.where(mask, x.roll(-1, 0), x)`` with the mask given (f32 N x 1 x 224 x
224).

Whole step: one eager ``SemiSupervisedEpocher`` step (``--dtype``, bf16 by default; 5 labelled + 5 + 5 unlabelled slices of
224 x 224) in four forms: without a hook, with plain CPS, with ``on: [labeled, unlabeled, unlabeled_tf, cutmix]`` and with ``on:
[cutmix]``.  Eager-step figures differ more between processes than between trees (README), so ``--children K`` runs the step
part in K child processes one after the other and reports, per form, the minimum over all of them and the range of the
children's own minima.

Device events around replays or eager steps, a host clock around call + synchronise; everything is warmed up first; the
variants are timed in alternating order, the order rotating from round to round, and every round is printed so that the
spread shows.

``--part parent --parent ROOT`` (a built checkout of the parent commit) writes a file of its own, ``profiles/cps_cutmix_parent.txt``:
in alternating child processes, this tree and the parent, (1) the flagship ``bench.py`` pre-train step and (2) the criterion
part of ``tools/diag/cps_time.py`` -- ``cross_pseudo.hip`` shares device code with ``cutmix.hip`` through ``pixel_criterion.hpp``,
so the sibling's own launch is timed on both trees.

    python tools/diag/cps_cutmix_time.py [--reps 200] [--rounds 4] [--part all|criterion|step|parent] [--dtype bf16|fp32]
        [--children 3] [--parent ROOT] [--pairs 2]"""
import argparse
import json
import os
import re
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cps_time import DEV, REPO, SHAPES, _batch, _call_sync, _captured, _epocher, _events, _rounds  # noqa: E402

SEED, RANGE = 23, (0.25, 0.5)


def _criterion_variants(shape):
    """-> [(name, eager callable)], a note on what the variants computed, a check that replays write their loss"""
    from spcl_amd import functional as F_hip
    g = torch.Generator().manual_seed(SEED)
    N, C, H, W = shape

    def cl(x):
        return x.to(DEV).contiguous(memory_format=torch.channels_last)

    s_a, s_b, t_a, t_b = (cl(3.0 * torch.randn(*shape, generator=g)) for _ in range(4))
    boxes = F_hip.cutmix_boxes(SEED, N, H, W, RANGE, device=DEV)
    ys, xs = torch.arange(H, device=DEV).view(1, H, 1), torch.arange(W, device=DEV).view(1, 1, W)
    y0, x0, bh, bw = (boxes[:, k].long().view(N, 1, 1) for k in range(4))
    mask = ((ys >= y0) & (ys < y0 + bh) & (xs >= x0) & (xs < x0 + bw)).view(N, 1, H, W)
    unit = F_hip.register_unit_gradient(torch.ones((), device=DEV))
    zeros = torch.zeros(C, device=DEV)
    seen = {}

    def fused():
        x, y = s_a.detach().requires_grad_(True), s_b.detach().requires_grad_(True)
        loss = F_hip.cross_pseudo_ce_mixed(x, y, t_a, t_b, boxes, 1)
        loss.backward(gradient=unit)
        seen["fused"] = (loss.detach(), x.grad, y.grad)

    def composed():
        x, y = s_a.detach().requires_grad_(True), s_b.detach().requires_grad_(True)
        ma, mb = torch.where(mask, t_a.roll(-1, 0), t_a), torch.where(mask, t_b.roll(-1, 0), t_b)
        loss = F_hip.pseudo_label_ce(mb, x, zeros) + F_hip.pseudo_label_ce(ma, y, zeros)
        loss.backward(gradient=unit)
        seen["composed"] = (loss.detach(), x.grad, y.grad)

    def torch_ops():
        x, y = s_a.detach().requires_grad_(True), s_b.detach().requires_grad_(True)
        with torch.no_grad():
            ma, mb = torch.where(mask, t_a.roll(-1, 0), t_a), torch.where(mask, t_b.roll(-1, 0), t_b)
            pa, pb = ma.softmax(1), mb.softmax(1)
            ya, yb = ma.argmax(1), mb.argmax(1)
            keep_a, keep_b = pa.max(1).values >= 0.0, pb.max(1).values >= 0.0
        ce = torch.nn.functional.cross_entropy
        loss = (ce(x, yb, reduction="none") * keep_b).mean() + (ce(y, ya, reduction="none") * keep_a).mean()
        loss.backward()
        seen["torch"] = (loss.detach(), x.grad, y.grad)

    variants = [("(a) cross_pseudo_ce_mixed", fused), ("(b) 2 x where + 2 x pseudo_label_ce", composed), ("(c) torch ops", torch_ops)]
    for _, fn in variants:
        fn()
    torch.cuda.synchronize()
    ref = seen["fused"]
    note = []
    for key in ("composed", "torch"):
        loss, gx, gy = seen[key]
        note.append(f"{key}: loss rel {abs(float(loss) - float(ref[0])) / abs(float(ref[0])):.1e}, gradients rel L2 "
                    f"{float((gx - ref[1]).norm() / ref[1].norm()):.1e} / {float((gy - ref[2]).norm() / ref[2].norm()):.1e}")
    eager = {key: float(v[0]) for key, v in seen.items()}

    def replays_write_their_loss(graphs):
        found = []
        for (name, replay), key in zip(graphs, ("fused", "composed", "torch")):
            seen[key][0].zero_()
            replay()
            torch.cuda.synchronize()
            ok = float(seen[key][0]) == eager[key]
            found.append(f"{name} {'wrote the eager value again' if ok else 'did NOT write its loss (' + repr(float(seen[key][0])) + ')'}")
        return "after the timed replays each captured loss was zeroed and one more replay run: " + ", ".join(found)

    inside = float(mask.sum()) / (N * H * W)
    return variants, f"{inside:.3f} of the pixels inside a box; against (a): " + "; ".join(note), replays_write_their_loss


def _mix_variants(N):
    """the box launch, and the image mix against torch.where with the mask given"""
    from spcl_amd import functional as F_hip
    g = torch.Generator().manual_seed(SEED)
    x = torch.rand(N, 1, 224, 224, generator=g).to(DEV)
    word = torch.tensor([SEED], dtype=torch.int32, device=DEV)
    boxes = F_hip.cutmix_boxes(word, N, 224, 224, RANGE)
    ys, xs = torch.arange(224, device=DEV).view(1, 224, 1), torch.arange(224, device=DEV).view(1, 1, 224)
    y0, x0, bh, bw = (boxes[:, k].long().view(N, 1, 1) for k in range(4))
    mask = ((ys >= y0) & (ys < y0 + bh) & (xs >= x0) & (xs < x0 + bw)).view(N, 1, 224, 224)
    same = torch.equal(F_hip.cutmix_images(x, boxes, 1), torch.where(mask, x.roll(-1, 0), x))
    variants = [("cutmix_boxes", lambda: F_hip.cutmix_boxes(word, N, 224, 224, RANGE)),
                ("cutmix_images", lambda: F_hip.cutmix_images(x, boxes, 1)),
                ("torch.where(mask, roll, x)", lambda: torch.where(mask, x.roll(-1, 0), x))]
    return variants, f"the two mixes are {'bit-equal' if same else 'DIFFERENT'}"


def _step_variants(dtype):
    from spcl_amd.semi_seg import hooks as H
    lab, unl = _batch(5, 224, 1), _batch(5, 224, 2)
    every = ("labeled", "unlabeled", "unlabeled_tf", "cutmix")
    makers = [("no hook", lambda m: []),
              ("cps", lambda m: [H.create_cross_pseudo_hook(model=m, weight=1.5)]),
              ("cps + cutmix on all four maps", lambda m: [H.create_cross_pseudo_hook(model=m, weight=1.5, on=every)]),
              ("cps on cutmix only", lambda m: [H.create_cross_pseudo_hook(model=m, weight=1.5, on=("cutmix",))])]
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


def _children(args):
    """the step part in ``args.children`` child processes, one after the other; -> their lines and the summary"""
    lines, minima = [], {}
    for k in range(args.children):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", "step", "--reps", str(args.reps), "--rounds",
               str(args.rounds), "--dtype", args.dtype, "--children", "0", "--out", ""]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        if done.returncode != 0:
            raise SystemExit(f"child {k} failed ({done.returncode}):\n{done.stdout}")
        figures = [line for line in done.stdout.splitlines() if line.startswith("min .. max")][-1]
        lines.append(f"child {k}: {figures}")
        for name, low in re.findall(r"(?:: |, )([^,:]+?) ([0-9.]+) \.\. [0-9.]+ us", figures):
            minima.setdefault(name, []).append(float(low))
    base = min(minima["no hook"])
    lines.append("over the children -- minimum (range of the children's minima), factor over the hook-less minimum: " + "; ".join(
        f"{name} {min(v):.1f} us ({min(v):.1f} .. {max(v):.1f}), {min(v) / base:.2f}x" for name, v in minima.items()))
    return lines


def _parent_pairs(args):
    """this tree and ``args.parent`` in alternating child processes: bench.py's pre-train step, cps_time.py's criterion part"""
    trees = ((REPO, "this tree"), (os.path.abspath(args.parent), "the parent commit"))
    lines = [f"flagship pre-train step (bench.py --gpus 1 --steps 200 --warmup 20 --no-cpu-baseline --no-extras), {args.pairs} "
             "alternating pairs of child processes"]
    for k in range(args.pairs):
        for root, name in trees:
            cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "200", "--warmup", "20",
                   "--no-cpu-baseline", "--no-extras"]
            done = subprocess.run(cmd, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            if done.returncode != 0:
                raise SystemExit(f"bench.py of {name} failed ({done.returncode}):\n{done.stdout[-2000:]}")
            result = json.loads([line for line in done.stdout.splitlines() if line.startswith("{")][-1])
            lines.append(f"pair {k}, {name}: {result['ms_per_step']} ms per step, {result['value']} {result['unit']}")
    lines.append(f"cross_pseudo_ce against its two-call composition and torch (tools/diag/cps_time.py --part criterion --reps "
                 f"{args.reps}), {args.pairs} alternating pairs of child processes; per child the four `min .. max` lines: graph "
                 "replays and call + synchronise at 10 x 4 x 224 x 224, then at 32 x 4 x 224 x 224")
    for k in range(args.pairs):
        for root, name in trees:
            cmd = [sys.executable, os.path.join(root, "tools", "diag", "cps_time.py"), "--part", "criterion", "--reps",
                   str(args.reps), "--rounds", str(args.rounds), "--root", root, "--out", ""]
            done = subprocess.run(cmd, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            if done.returncode != 0:
                raise SystemExit(f"cps_time.py of {name} failed ({done.returncode}):\n{done.stdout[-2000:]}")
            for line in done.stdout.splitlines():
                if line.startswith("min .. max"):
                    lines.append(f"pair {k}, {name}: {line}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--part", choices=("all", "criterion", "step", "parent"), default="all")
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16", help="compute dtype of the whole step")
    ap.add_argument("--children", type=int, default=3, help="child processes for the step part (0: time it in this process)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for --part parent")
    ap.add_argument("--pairs", type=int, default=2, help="alternating pairs of child processes for --part parent")
    ap.add_argument("--out", default=None, help="default profiles/cps_cutmix_time.txt (profiles/cps_cutmix_parent.txt for "
                                                "--part parent); an empty string writes no file")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "cps_cutmix_parent.txt" if args.part == "parent" else "cps_cutmix_time.txt")
    if args.part == "parent":  # child processes only: this process never opens the device
        if not args.parent:
            raise SystemExit("--part parent needs --parent ROOT")
        text = "\n".join(_parent_pairs(args)) + "\n"
        print(text, end="")
        if args.out:
            with open(args.out, "w") as f:
                f.write(text)
        return
    lines = []
    n = max(10, args.reps // 5)
    if args.part in ("all", "step") and args.children > 0:  # children first: this process has not opened the device yet
        lines.append(f"semi-supervised step, compute dtype {args.dtype}, batch 5 + 5 + 5 x 1 x 224 x 224, eager, {args.children} "
                     f"child processes, each {args.rounds} figures of {n} steps per form")
        lines += _children(args)
    sys.path.insert(0, REPO)
    if not torch.cuda.is_available():
        raise SystemExit("cps_cutmix_time.py measures on the GPU: no device found")
    import spcl_amd  # noqa: F401
    from spcl_amd import native
    lines.insert(0, f"library {os.path.relpath(native.LIB_PATH, REPO)}, C ABI {native.ABI_VERSION}")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    if args.part in ("all", "criterion"):
        for shape in SHAPES:
            variants, note, check = _criterion_variants(shape)
            M = shape[0] * shape[2] * shape[3]
            lines.append(f"criterion, forward + backward of both student maps {' x '.join(map(str, shape))} f32 channels-last, no "
                         f"thresholds; {note}; (a) moves {6 * M * shape[1] * 4 / 1e6:.1f} MB")
            graphs = [(name, _captured(fn).replay) for name, fn in variants]
            lines.append(f"graph replays, {args.reps} per figure")
            lines += _rounds(graphs, _events, args.reps, args.rounds, "us", 1e3)[0]
            lines.append(check(graphs))
            lines.append(f"call + synchronise (host clock), {args.reps} per figure")
            lines += _rounds(variants, _call_sync, args.reps, args.rounds, "us", 1e3)[0]
            variants, note = _mix_variants(shape[0])
            lines.append(f"boxes and image mix, {shape[0]} x 1 x 224 x 224 f32; {note}")
            graphs = [(name, _captured(fn).replay) for name, fn in variants]
            lines.append(f"graph replays, {args.reps} per figure")
            lines += _rounds(graphs, _events, args.reps, args.rounds, "us", 1e3)[0]
            lines.append(f"call + synchronise (host clock), {args.reps} per figure")
            lines += _rounds(variants, _call_sync, args.reps, args.rounds, "us", 1e3)[0]
    if args.part == "step" and args.children == 0:
        steps = _step_variants(dtype)
        lines.append(f"semi-supervised step, compute dtype {args.dtype}, batch 5 + 5 + 5 x 1 x 224 x 224, eager, {n} steps per figure")
        lines += _rounds(steps, _events, n, args.rounds, "us", 1e3)[0]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
