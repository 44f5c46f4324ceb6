"""Forward + backward of ``SupConLoss3`` (soft pair weights, csrc/supcon_weighted.hip) against the plain torch formulation of
the same formula on the same device, both modes, at n = 30 (the training size: one workgroup, one launch) and n = 2048 (the
row kernels), d = 128, t = 0.07.

Each side is captured once into a hipGraph (forward, then ``torch.autograd.grad`` to the two inputs) and replayed: per round
``--reps`` replays of one, then of the other, between device events; the figure is the median over ``--rounds`` rounds with
the rounds' extremes beside it.  The torch side is written from the formula

    s = z z^T / t,  D_i = sum_{j != i} exp(s_ij),  W_i = sum_{j != i} P_ij,
    out mode: -mean_i [ sum_j P_ij (s_ij - log D_i) / W_i ]      in mode: -mean_i [ log(sum_j P_ij exp(s_ij) / D_i) / W_i ]

with P = pos_weight tiled 2 x 2 and the diagonal removed (built once, outside the timed graph), float32.  Before timing, the
two sides' losses and gradients are compared.

    python tools/diag/weighted_supcon_time.py [--out profiles/weighted_supcon_time.txt]"""
import argparse
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)
DEV = "cuda:0"


def torch_loss(z1, z2, P, off, t, out_mode):
    z = torch.cat([z1, z2])
    s = z @ z.t() / t
    l = s - s.max(dim=1, keepdim=True).values.detach()
    x = torch.exp(l) * off
    D, W = x.sum(1), P.sum(1)
    if out_mode:
        return -((P * l).sum(1) / W - torch.log(D)).mean()
    return -(torch.log((P * x).sum(1) / D) / W).mean()


def capture(fn, z1, z2):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):  # warm-up outside the capture: code objects, allocator
            torch.autograd.grad(fn(z1, z2), (z1, z2))
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        loss = fn(z1, z2)
        d1, d2 = torch.autograd.grad(loss, (z1, z2))
    return g, (loss, d1, d2)


def time_pair(graphs, reps, rounds, warmup):
    for g in graphs:
        for _ in range(warmup):
            g.replay()
    out = [[] for _ in graphs]
    for _ in range(rounds):
        for k, g in enumerate(graphs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                g.replay()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) / reps)
    return out


def spread(xs):
    return f"{statistics.median(xs):.4f} (min {min(xs):.4f}, max {max(xs):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses.contrast_loss import SupConLoss3
    lines = [f"SupConLoss3 forward + backward, d = 128, t = 0.07, float32; hipGraph replays, {args.reps} per round, "
             f"{args.rounds} rounds, fused and torch interleaved; device events, ms per forward + backward: median (min, max)"]
    for n in (30, 2048):
        g = torch.Generator().manual_seed(n)
        z1 = torch.nn.functional.normalize(torch.randn(n, 128, generator=g), dim=1).to(DEV).requires_grad_(True)
        z2 = torch.nn.functional.normalize(torch.randn(n, 128, generator=g), dim=1).to(DEV).requires_grad_(True)
        w = (0.05 + 0.95 * torch.rand(n, n, generator=g)).to(DEV)
        off = 1 - torch.eye(2 * n, device=DEV)
        P = w.repeat(2, 2) * off
        for out_mode in (True, False):
            crit = SupConLoss3(out_mode=out_mode, sync_checks=False)
            gf, rf = capture(lambda a, b: crit(a, b, pos_weight=w), z1, z2)
            gt, rt = capture(lambda a, b: torch_loss(a, b, P, off, 0.07, out_mode), z1, z2)
            gf.replay()
            gt.replay()
            torch.cuda.synchronize()
            crit.check()
            dl = abs(float(rf[0]) - float(rt[0]))
            dg = max(float((rf[k] - rt[k]).abs().max()) for k in (1, 2))
            gm = max(float(rt[k].abs().max()) for k in (1, 2))
            tf, tt = time_pair([gf, gt], args.reps, args.rounds, args.warmup)
            ratio = statistics.median(tt) / statistics.median(tf)
            lines.append(f"n = {n:4d} {'out' if out_mode else 'in '} mode  fused {spread(tf)} ms | torch {spread(tt)} ms | "
                         f"torch / fused = {ratio:.2f} | loss {float(rf[0]):.6f}, |fused - torch| = {dl:.1e}; gradients differ by "
                         f"at most {dg:.1e} (largest entry {gm:.1e})")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
