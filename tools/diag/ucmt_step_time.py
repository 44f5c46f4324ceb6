"""Time the uncertainty-aware mean teacher's criterion at the reference's batch shape (10 x 4 x 224 x 224 class maps, K = 8
noisy teacher predictions):

* the fused launch -- ``functional.ucmt_softmax_mse`` and its backward (the gradient is written by the forward launch) --;
* the same arithmetic as the reference writes it (semi_seg/epochers/comparable.py:78-105) in torch ops on the same device
  tensors: 9 per-sample flips, ``average_iter`` (7 adds and a divide), 3 softmaxes, the entropy, the compare, the un-reduced
  MSE, ``mean(1)``, the multiply, ``mean()`` and autograd's backward to the student's logits -- the baseline: no earlier
  version of this project runs this criterion.

The teacher's K + 1 forward passes are the same in both and are not timed.  Device events around replayed calls; every
shape is warmed up first; each figure is the mean of ``--reps`` repetitions, the whole measurement is repeated ``--rounds``
times in one process so that the spread shows.  The lines are printed and written to ``--out``.

    python tools/diag/ucmt_step_time.py [--reps 30] [--rounds 3] [--out profiles/ucmt_step_time.txt]"""
import argparse
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
DEV = "cuda:0"
SHAPE, K, THRESHOLD = (10, 4, 224, 224), 8, 0.75
FLAGS = [3, 0, 1, 2, 0, 3, 1, 2, 0, 3]


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


def _flip_torch(x, flags):  # what ``torch.stack([affine_transformer(v) for v in x])`` does per sample (comparable.py:79-80)
    out = []
    for v, f in zip(x, flags):
        if f & 1:
            v = v.flip(-2)
        if f & 2:
            v = v.flip(-1)
        out.append(v)
    return torch.stack(out, dim=0)


def _times(reps):
    from spcl_amd import functional as F_hip
    g = torch.Generator().manual_seed(2)

    def cl(x):
        return x.to(DEV).contiguous(memory_format=torch.channels_last)

    teacher, student = cl(torch.randn(*SHAPE, generator=g)), cl(torch.randn(*SHAPE, generator=g))
    noisy = [cl(3.0 * torch.randn(*SHAPE, generator=g)) for _ in range(K)]
    flags = torch.tensor(FLAGS, dtype=torch.uint8, device=DEV)
    unit = F_hip.register_unit_gradient(torch.ones((), device=DEV))

    def fused():
        x = student.detach().requires_grad_(True)
        out = []
        F_hip.ucmt_softmax_mse(teacher, noisy, x, THRESHOLD, 1.0, flags, out=out).backward(gradient=unit)
        return out[0]

    def torch_ops(item):
        x = student.detach().requires_grad_(True)
        reg = torch.nn.functional.mse_loss(x.softmax(1), _flip_torch(teacher, FLAGS).softmax(1).detach(), reduction="none")
        preds = [_flip_torch(t, FLAGS) for t in noisy]
        avg = sum(preds) / float(len(preds))
        q = avg.softmax(1)
        entropy = -(q * (q + 1e-16).log()).sum(1) / math.log(avg.shape[1])
        mask = (entropy <= THRESHOLD).float()
        ratio = mask.mean()
        if item:
            ratio.item()  # (comparable.py:101)
        (reg.mean(1) * mask).mean().backward()
        return ratio

    kept = int(fused())
    ratio = float(torch_ops(False))
    return {"fused launch + backward": _time(fused, reps * 10),
            "torch flips / average / softmaxes / entropy / compare / MSE / backward": _time(lambda: torch_ops(False), reps),
            "the same with the reference's .item()": _time(lambda: torch_ops(True), reps)}, kept, ratio


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ucmt_step_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ucmt_step_time.py measures on the GPU: no device found")
    import spcl_amd  # noqa: F401
    M = SHAPE[0] * SHAPE[2] * SHAPE[3]
    moved = (K + 3) * M * SHAPE[1] * 4 + M
    lines = [f"class maps {' x '.join(map(str, SHAPE))} f32 channels-last, K = {K} noisy maps, threshold {THRESHOLD}, "
             f"{args.reps} reps per figure (x 10 for the fused launch); the fused launch moves {moved / 1e6:.1f} MB"]
    for r in range(args.rounds):
        t, kept, ratio = _times(args.reps)
        fused, plain = t["fused launch + backward"], t["torch flips / average / softmaxes / entropy / compare / MSE / backward"]
        lines.append(f"round {r}: " + ", ".join(f"{a} {v * 1e3:.1f} us" for a, v in t.items()) +
                     f" (torch / fused = {plain / fused:.1f}x; fused: {moved / (fused * 1e-3) / 1e9:.0f} GB/s; kept {kept} of {M} "
                     f"pixels, torch's mask keeps {ratio * M:.0f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
