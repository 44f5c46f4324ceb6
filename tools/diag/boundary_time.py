"""Time the boundary loss (csrc/boundary.hip, contrastyou/losses/boundary.py):

* ``functional.signed_distance_maps`` at 10 x 3 x 224^2 and 32 x 3 x 224^2 on smooth blobs and on per-pixel random labels,
  replayed from a captured graph (device time between events), with the two kernels' own times; against the host path every
  published implementation takes (labels to the host, scipy ``distance_transform_edt`` per (slice, class), upload: wall time)
  and against a torch-only device formulation without [HW, HW] matrices (column distances by cummax / cummin, row minima over
  an [.., W, W] broadcast: replayed from a graph).  The three results are compared bit for bit.
* ``BoundaryLoss.from_logits`` forward + backward against ``DiceKLLoss`` alone (what the boundary term adds: the maps, a third
  read of the logits, the gradient accumulation) and against the composed torch formulation given precomputed maps.
* one ``FineTuneEpocher`` step (UNet max_channel 256, bf16, 32 x 224^2, replayed from its hipGraph) with ``kl``, ``dice_kl`` and
  ``boundary``, each in a process of its own, alternating; with ``--parent ROOT`` (a built checkout of the parent commit) that
  tree's ``kl`` and ``dice_kl`` steps run in the same alternation.

Every figure is the median over ``--windows`` windows of ``--reps`` calls (smallest and largest window beside it).  The lines
are printed and written to ``--out``.  No pass / fail bar.

    python tools/diag/boundary_time.py [--reps 50] [--windows 9] [--rounds 3] [--parent ROOT] [--out profiles/boundary_time.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from sup_dice_time import _kernel_us, _replayed, _stat, _torch_dice_kl, _wall  # noqa: E402

DEV = "cuda:0"
CLASSES = (1, 2, 3)


def _blobs(N, H, W, g):
    """discs of the three foreground classes (radius 8 - 48) on background"""
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    lab = torch.zeros(N, H, W, dtype=torch.long)
    for i in range(N):
        for k in range(4):
            cy, cx = (torch.rand(2, generator=g) * torch.tensor([H, W])).tolist()
            r = 8.0 + float(torch.rand((), generator=g)) * 40.0
            lab[i][(ys - cy) ** 2 + (xs - cx) ** 2 <= r * r] = 1 + k % 3
    return lab


def _host_maps(labels, classes):
    """the host path: copy down, scipy per (slice, class), upload -> [N, S, H, W] f32 on the labels' device"""
    import numpy as np
    from scipy.ndimage import distance_transform_edt as edt
    lab = labels.cpu().numpy()
    out = np.zeros((lab.shape[0], len(classes)) + lab.shape[1:], dtype=np.float32)
    for n in range(lab.shape[0]):
        for s, c in enumerate(classes):
            m = lab[n] == c
            if m.any() and not m.all():
                out[n, s] = edt(~m) * ~m - (edt(m) - 1.0) * m
    return torch.from_numpy(out).to(labels.device)


def _torch_maps(labels, classes):
    """a torch-only device formulation: separable like the kernels, the row minima as one [N, S, H, W, W] broadcast (no
    [HW, HW] matrix; 4 W bytes per pixel and plane of scratch)"""
    N, H, W = labels.shape
    dev, far = labels.device, 1 << 15  # (far^2 + (W - 1)^2 < 2^31)
    m = torch.stack([labels == c for c in classes], 1)
    ys = torch.arange(H, device=dev, dtype=torch.int32).view(1, 1, H, 1)
    xs = torch.arange(W, device=dev, dtype=torch.int32)
    dx2 = (xs.view(W, 1) - xs.view(1, W)) ** 2

    def vertical(mask):  # distance to the nearest True of the column, `far` where it has none
        up = torch.where(mask, ys, -far).cummax(2).values
        down = torch.where(mask, ys, far).flip(2).cummin(2).values.flip(2)
        return torch.minimum(torch.where(up < 0, far, ys - up), torch.where(down >= far, far, down - ys))

    def row_min(g):
        return ((g * g).unsqueeze(-2) + dx2).amin(-1)

    d2 = torch.where(m, row_min(vertical(~m)), row_min(vertical(m)))
    d = d2.double().sqrt()
    return torch.where(d2 >= far * far, torch.zeros_like(d), torch.where(m, 1.0 - d, d)).float()


def _map_lines(reps, windows):
    from spcl_amd import functional as F_hip
    lines = ["signed_distance_maps, classes (1, 2, 3) of int64 labels:"]
    g = torch.Generator().manual_seed(3)
    for N in (10, 32):
        for kind in ("blobs", "random"):
            lab = (_blobs(N, 224, 224, g) if kind == "blobs" else torch.randint(0, 4, (N, 224, 224), generator=g)).to(DEV)
            hip = F_hip.signed_distance_maps(lab, CLASSES)
            host, tch = _host_maps(lab, CLASSES), _torch_maps(lab, CLASSES)
            rep = _replayed(lambda: F_hip.signed_distance_maps(lab, CLASSES), reps, windows)
            eager = _wall(lambda: F_hip.signed_distance_maps(lab, CLASSES), reps, windows)
            rep_t = _replayed(lambda: _torch_maps(lab, CLASSES), max(reps // 10, 3), max(windows // 3, 3))
            t_host = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _host_maps(lab, CLASSES)
                torch.cuda.synchronize()
                t_host.append((time.perf_counter() - t0) * 1e3)
            base = statistics.median(rep)
            lines.append(f"  {N} x 3 x 224 x 224, {kind} (largest |phi| {float(hip.abs().max()):.1f})")
            lines.append(f"      HIP, two launches               replayed from a graph {_stat(rep)}   call + synchronise {_stat(eager)}")
            for sym, us in _kernel_us(lambda: F_hip.signed_distance_maps(lab, CLASSES), reps).items():
                lines.append(f"      kernel alone: {us:7.1f} us  {sym[:100]}")
            lines.append(f"      torch ops on the device         replayed from a graph {_stat(rep_t)}   "
                         f"(torch / HIP = {statistics.median(rep_t) / base:.0f}x)")
            lines.append(f"      host: copy, scipy edt, upload   wall {_stat(t_host, 'ms', 1.0, 1)}   "
                         f"({statistics.median(t_host) / (N * 3):.2f} ms per (slice, class); host / HIP = "
                         f"{statistics.median(t_host) / base:.0f}x)")
            lines.append(f"      same bits: HIP == host {torch.equal(hip, host)}, HIP == torch {torch.equal(hip, tch)}")
    return lines


def _criterion_lines(reps, windows):
    from spcl_amd import functional as F_hip
    from spcl_amd.contrastyou.losses import BoundaryLoss, DiceKLLoss
    lines = ["BoundaryLoss.from_logits (DiceKLLoss(0.7, 1.3, class weights) + alpha L_B, alpha 0.25, classes 1 .. C-1), forward + "
             "backward, f32 channels-last logits, blob labels:"]
    g = torch.Generator().manual_seed(5)
    for N, C, H, W in ((32, 4, 224, 224), (10, 5, 224, 224)):
        gd = torch.Generator(device=DEV).manual_seed(5)
        x = (3 * torch.randn((N, H, W, C), device=DEV, generator=gd)).permute(0, 3, 1, 2).requires_grad_(True)
        y = (_blobs(N, H, W, g) % C).to(DEV)
        weights = [0.5 + 0.25 * c for c in range(C)]
        w = torch.tensor(weights, device=DEV)
        classes = tuple(range(1, C))
        region = DiceKLLoss(dice_weight=0.7, kl_weight=1.3, class_weight=weights)
        crit = BoundaryLoss(region=DiceKLLoss(dice_weight=0.7, kl_weight=1.3, class_weight=weights), alpha=0.25)
        phi = F_hip.signed_distance_maps(y, classes)
        alpha = torch.full((), 0.25, device=DEV)

        def torch_loss():
            return _torch_dice_kl(x, y, w, 0.7, 1.3) + 0.25 * (torch.softmax(x, 1)[:, 1:] * phi).mean()

        fns = (("BoundaryLoss (maps + region + boundary)", lambda: torch.autograd.grad(crit.from_logits(x, y), x)),
               ("DiceKLLoss alone", lambda: torch.autograd.grad(region.from_logits(x, y), x)),
               ("boundary term alone, maps given", lambda: torch.autograd.grad(F_hip.boundary_loss(x, phi, classes, alpha), x)),
               ("torch ops, composed, maps given", lambda: torch.autograd.grad(torch_loss(), x)))
        got, want = float(crit.from_logits(x, y).detach()), float(torch_loss().detach())
        dg, dw = fns[0][1]()[0], fns[3][1]()[0]
        lines.append(f"  {N} x {C} x {H} x {W}")
        res = {name: (_wall(fn, reps, windows), _replayed(fn, reps, windows)) for name, fn in fns}
        base = statistics.median(res[fns[0][0]][1])
        for name, (wall, rep) in res.items():
            extra = ""
            if name.startswith("DiceKLLoss"):
                extra = f"   (the boundary term costs {(base - statistics.median(rep)) * 1e3:+.1f} us on top)"
            elif name.startswith("torch"):
                extra = f"   (torch / HIP = {statistics.median(rep) / base:.1f}x, the maps not counted for torch)"
            lines.append(f"      {name:40s} call + synchronise {_stat(wall)}   replayed from a graph {_stat(rep)}{extra}")
        for sym, us in _kernel_us(fns[0][1], reps).items():
            lines.append(f"      kernel alone: {us:7.1f} us  {sym[:100]}")
        lines.append(f"      loss {got:.7f} / {want:.7f}, gradient relative L2 difference "
                     f"{float((dg - dw).double().norm() / dw.double().norm()):.1e}")
    return lines


def _step_child(root, criterion, steps, windows):
    """one process: ms per replayed FineTuneEpocher step of the tree at ``root`` -> one JSON line"""
    sys.path.insert(0, root)
    import spcl_amd  # noqa: F401
    from spcl_amd import ddp
    from spcl_amd.contrastyou.losses import build_sup_criterion
    from spcl_amd.optim import FusedRAdam
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.epochers import FineTuneEpocher
    crit = build_sup_criterion({"SupCriterion": {"name": criterion}})
    bs, size = 32, 224
    torch.manual_seed(4)
    net = UNet(input_dim=1, num_classes=4, max_channel=256).to(DEV)
    net.set_compute_dtype(torch.bfloat16)
    flat = ddp.FlatParams([p for p in net.parameters() if p.requires_grad])
    opt = FusedRAdam([flat.param], lr=1e-4, weight_decay=1e-5)
    ep = FineTuneEpocher(model=net, optimizer=opt, labeled_loader=iter([]), sup_criterion=crit, num_batches=10 ** 9,
                         cur_epoch=5, device="cuda", flat_params=flat, graph=True)
    net.train()
    g, gd = torch.Generator().manual_seed(8), torch.Generator(device=DEV).manual_seed(8)
    batches = []
    for k in range(4):
        img = torch.rand(bs, 1, size, size, device=DEV, generator=gd)
        tgt = _blobs(bs, size, size, g).unsqueeze(1).to(DEV)
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
    runs = [(f"this commit, {c}", REPO, c) for c in ("kl", "dice_kl", "boundary")]
    if parent:
        runs[1:1] = [(f"parent commit, {c}", os.path.abspath(parent), c) for c in ("kl", "dice_kl")]
    times = {name: [] for name, _, _ in runs}
    for r in range(rounds):
        order = runs[r % len(runs):] + runs[:r % len(runs)]  # (no run keeps the place behind the same neighbour)
        for name, root, criterion in order:  # (alternating: one process per run, one after the other)
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--step-child", root, "--criterion", criterion,
                                  "--reps", str(steps), "--windows", str(windows)], capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                raise SystemExit(f"{name}: the step process failed ({res.returncode})\n{res.stderr[-2000:]}")
            times[name].append(statistics.median(json.loads(res.stdout.strip().splitlines()[-1])["ms"]))
    lines = [f"one FineTuneEpocher step (UNet max_channel 256, bf16, 32 x 224 x 224, blob labels, replayed from its hipGraph, wall "
             f"time over {steps} steps), ms per step: median of {rounds} alternating processes (smallest - largest = the "
             f"run-to-run spread)"]
    for name, t in times.items():
        lines.append(f"  {name:26s} {_stat(t, 'ms', 1.0, 3)}")
    if not parent:
        lines.append("  (no --parent tree given: the steps of the parent commit were not measured in this run)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its steps are timed too)")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--step-child", metavar="ROOT", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--criterion", default="kl", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "boundary_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("boundary_time.py measures on the GPU: no device found")
    if args.step_child:
        return _step_child(args.step_child, args.criterion, args.reps, args.windows)
    sys.path.insert(0, REPO)
    import spcl_amd  # noqa: F401
    lines = [f"median of {args.windows} windows of {args.reps} calls (smallest - largest window)"]
    lines += _map_lines(args.reps, args.windows)
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
