"""Time the soft-Dice + class-weighted KL criterion (csrc/sup_dice.hip) at 32 x 4 x 224^2 and 10 x 5 x 224^2:

* forward + backward of ``DiceKLLoss.from_logits`` against the composed torch formulation of the same loss on the same device
  (softmax, one-hot, the three sums, the Dice ratio, the weighted log term, autograd) and against the existing fused
  ``functional.sup_loss_kl_onehot`` (one pass: what the second pass costs), both eagerly (call + synchronise) and replayed
  from a captured graph (device time between events); the achieved fraction of the algorithmic bytes -- two reads and one
  write of the class map plus two reads of the labels -- is printed beside the replayed time.
* one ``FineTuneEpocher`` step (UNet max_channel 256, bf16, 32 x 224^2, replayed from its hipGraph) with ``KL_div`` and with
  ``DiceKLLoss``, each in a process of its own, alternating; with ``--parent ROOT`` (a built checkout of the parent commit)
  the ``KL_div`` step of that tree runs in the same alternation.

Every figure is the median over ``--windows`` windows of ``--reps`` calls (smallest and largest window beside it).  The lines
are printed and written to ``--out``.  No pass / fail bar.

    python tools/diag/sup_dice_time.py [--reps 50] [--windows 9] [--rounds 3] [--parent ROOT] [--out profiles/sup_dice_time.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"
SHAPES = ((32, 4, 224, 224), (10, 5, 224, 224))


def _stat(samples, unit="us", scale=1e3, digits=1):
    s = sorted(samples)
    return f"{statistics.median(s) * scale:.{digits}f} {unit} ({s[0] * scale:.{digits}f} - {s[-1] * scale:.{digits}f})"


def _wall(fn, reps, windows, warmup=3):
    """ms per call + synchronise"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
            torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / reps * 1e3)
    return out


def _replayed(fn, reps, windows):
    """ms of device time per replay of the captured call"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        keep = fn()  # noqa: F841 -- the outputs live as long as the graph
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            g.replay()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return out


def _kernel_us(fn, reps):
    """{kernel symbol: mean microseconds per call} of the library's kernels inside ``fn`` (its own launch timer,
    ``spcl_profile_*``: events around every launch)"""
    import ctypes

    from spcl_amd import native as n
    fn()
    torch.cuda.synchronize()
    n.call("spcl_profile_enable", 1)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    name = ctypes.create_string_buffer(256)
    us, by, fl = ctypes.c_float(), ctypes.c_double(), ctypes.c_double()
    total = {}
    for i in range(n.call("spcl_profile_count")):
        n.call("spcl_profile_get", i, name, 256, ctypes.byref(us), ctypes.byref(by), ctypes.byref(fl))
        key = name.value.decode()
        total[key] = total.get(key, 0.0) + us.value
    n.call("spcl_profile_enable", 0)
    return {k: v / reps for k, v in total.items()}


def _torch_dice_kl(x, y, w, dice_weight, kl_weight, smooth=1e-5, eps=1e-16):
    """the composed formulation in float32 torch ops (whole batch one group, every class)"""
    C = x.shape[1]
    p = torch.softmax(x, dim=1)
    t = torch.nn.functional.one_hot(y, C).permute(0, 3, 1, 2).to(p.dtype)
    inter, psum, tsum = (p * t).sum((0, 2, 3)), p.sum((0, 2, 3)), t.sum((0, 2, 3))
    l_dice = 1 - ((2 * inter + smooth) / (psum + tsum + smooth)).mean()
    l_kl = (-(t * w.view(1, C, 1, 1) * torch.log((p + eps) / (1 + eps))).sum(1)).mean()
    return dice_weight * l_dice + kl_weight * l_kl


def _criterion_lines(reps, windows):
    from spcl_amd import functional as F_hip
    from spcl_amd.contrastyou.losses import DiceKLLoss
    lines = []
    for N, C, H, W in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(5)
        x = (3 * torch.randn((N, H, W, C), device=DEV, generator=g)).permute(0, 3, 1, 2).requires_grad_(True)
        y = torch.randint(0, C, (N, H, W), device=DEV, generator=g)
        weights = [0.5 + 0.25 * c for c in range(C)]
        w = torch.tensor(weights, device=DEV)
        crit = DiceKLLoss(dice_weight=0.7, kl_weight=1.3, class_weight=weights)

        def hip():
            return torch.autograd.grad(crit.from_logits(x, y), x)

        def ref():
            return torch.autograd.grad(_torch_dice_kl(x, y, w, 0.7, 1.3), x)

        def one_pass():
            return torch.autograd.grad(F_hip.sup_loss_kl_onehot(x, y)[0], x)

        got, want = float(crit.from_logits(x, y).detach()), float(_torch_dice_kl(x, y, w, 0.7, 1.3).detach())
        dg, dw = hip()[0], ref()[0]
        same = (f"loss {got:.7f} / {want:.7f}, gradient relative L2 difference "
                f"{float((dg - dw).double().norm() / dw.double().norm()):.1e}")
        moved = N * H * W * (3 * C * 4 + 2 * 8)
        lines.append(f"  {N} x {C} x {H} x {W}")
        res = {}
        for name, fn in (("DiceKLLoss (two passes)", hip), ("torch ops, composed", ref), ("sup_loss_kl_onehot (one pass)", one_pass)):
            res[name] = (_wall(fn, reps, windows), _replayed(fn, reps, windows))
        base = statistics.median(res["DiceKLLoss (two passes)"][1])
        for name, (wall, rep) in res.items():
            extra = ""
            if name.startswith("DiceKLLoss"):
                extra = (f"   ({moved / 1e6:.1f} MB algorithmic: {moved / (base * 1e-3) / 1e12:.2f} TB/s achieved)")
            elif name.startswith("torch"):
                extra = f"   (torch / HIP = {statistics.median(rep) / base:.1f}x replayed)"
            else:
                extra = f"   (the second pass and the float64 sums cost {(base - statistics.median(rep)) * 1e3:+.1f} us)"
            lines.append(f"      {name:32s} call + synchronise {_stat(wall)}   replayed from a graph {_stat(rep)}{extra}")
        for sym, us in _kernel_us(hip, reps).items():
            lines.append(f"      kernel alone: {us:7.1f} us  {sym[:100]}")
        lines.append(f"      {same}")
    return lines


def _step_child(root, criterion, steps, windows):
    """one process: ms per replayed FineTuneEpocher step of the tree at ``root`` -> one JSON line"""
    sys.path.insert(0, root)
    import spcl_amd  # noqa: F401
    from spcl_amd import ddp
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.optim import FusedRAdam
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.epochers import FineTuneEpocher
    if criterion == "kl":
        crit = KL_div()
    else:
        from spcl_amd.contrastyou.losses import DiceKLLoss
        crit = DiceKLLoss(class_weight=[0.5, 1.0, 1.5, 2.0])
    bs, size = 32, 224
    torch.manual_seed(4)
    net = UNet(input_dim=1, num_classes=4, max_channel=256).to(DEV)
    net.set_compute_dtype(torch.bfloat16)
    flat = ddp.FlatParams([p for p in net.parameters() if p.requires_grad])
    opt = FusedRAdam([flat.param], lr=1e-4, weight_decay=1e-5)
    ep = FineTuneEpocher(model=net, optimizer=opt, labeled_loader=iter([]), sup_criterion=crit, num_batches=10 ** 9,
                         device="cuda", flat_params=flat, graph=True)
    net.train()
    g = torch.Generator(device=DEV).manual_seed(8)
    batches = []
    for k in range(4):
        img = torch.rand(bs, 1, size, size, device=DEV, generator=g)
        tgt = torch.randint(0, 4, (bs, 1, size, size), device=DEV, generator=g)
        groups = [f"patient{(i + k) % 3:03d}_00" for i in range(bs)]
        batches.append(((img, img, tgt, tgt), [f"f{i}" for i in range(bs)], (["0"] * bs, groups)))
    out = []
    with ep.meters.focus_on(ep.meter_focus):
        for k in range(6):
            ep.step(batches[k % 4])
        torch.cuda.synchronize()
        for _ in range(windows):
            t0 = time.perf_counter()
            for k in range(steps):
                ep.step(batches[k % 4])
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) / steps * 1e3)
    assert ep._step_graph.captured and not ep._step_graph.failed
    print(json.dumps({"ms": out}))


def _step_lines(parent, steps, windows, rounds):
    runs = [("this commit, KL_div", REPO, "kl"), ("this commit, DiceKLLoss", REPO, "dice_kl")]
    if parent:
        runs.insert(1, ("parent commit, KL_div", os.path.abspath(parent), "kl"))
    times = {name: [] for name, _, _ in runs}
    for r in range(rounds):
        order = runs[r % len(runs):] + runs[:r % len(runs)]  # (no run keeps the place behind the same neighbour)
        for name, root, criterion in order:  # (alternating: one process per run, one after the other)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step-child", root, "--criterion", criterion,
                                "--reps", str(steps), "--windows", str(windows)], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"{name}: the step process failed ({r.returncode})\n{r.stderr[-2000:]}")
            times[name].append(statistics.median(json.loads(r.stdout.strip().splitlines()[-1])["ms"]))
    lines = [f"one FineTuneEpocher step (UNet max_channel 256, bf16, 32 x 224 x 224, replayed from its hipGraph, wall time over "
             f"{steps} steps), ms per step: median of {rounds} alternating processes (smallest - largest = the run-to-run spread)"]
    for name, t in times.items():
        lines.append(f"  {name:26s} {_stat(t, 'ms', 1.0, 3)}")
    if not parent:
        lines.append("  (no --parent tree given: the KL_div step of the parent commit was not measured in this run)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its KL_div step is timed too)")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--step-child", metavar="ROOT", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--criterion", default="kl", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sup_dice_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sup_dice_time.py measures on the GPU: no device found")
    if args.step_child:
        return _step_child(args.step_child, args.criterion, args.reps, args.windows)
    sys.path.insert(0, REPO)
    import spcl_amd  # noqa: F401
    lines = [f"DiceKLLoss.from_logits (dice_weight 0.7, kl_weight 1.3, class weights), forward + backward, f32 channels-last "
             f"logits; median of {args.windows} windows of {args.reps} calls (smallest - largest window)"]
    lines += _criterion_lines(args.reps, args.windows)
    if not args.no_step:
        lines += _step_lines(args.parent, 30, 5, args.rounds)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
