"""Time the strong intensity view of the unlabelled pair (csrc/strong_view.hip: ``functional.strong_view_params``,
``strong_view_apply``; semi_seg/hooks/strongview.py).

Kernels, at 10 and 32 slices of 1 x 224 x 224, f32 and bf16, every gate open (all five ops on every slice: the dearest table),
seed word 23, all four flip values, replayed from a captured graph and as call + synchronise:

* (a) ``strong_view_params`` + ``strong_view_apply`` (two launches) against the parent's single ``flip_batch`` launch, and the
  two launches on their own; the apply launch under an all-neutral table (the pure-copy path) as well;
* (b) the same against a plain torch formulation on the same device: ``clamp``, ``pow``, the two affine ops, grouped ``conv2d``
  of the replicate-padded image with the 5 x 5 binomial kernel, ``randn``, ``clamp``, two ``where(flip)``, with the per-sample
  values read from the same table (the mean included: torch is not charged for it).

Whole step, (c): one eager ``SemiSupervisedEpocher`` step (``--dtype``, bf16 by default; 5 labelled + 5 + 5 unlabelled slices of
224 x 224) without a hook, with ``PseudoLabelParameters`` (``teacher: self``) alone, and with ``StrongViewParameters`` (defaults)
beside it, timed in one process in alternating order.

Accuracy: the measured maximum error of every case of tests/test_gpu_strong_view_kernels.py's float64 comparison (a child
``pytest`` process; the lines the tests print).

Device events around replays or eager steps, a host clock around call + synchronise; everything is warmed up first; the
variants are timed in alternating order, the order rotating from round to round, and every round is printed so that the
spread shows.

``--part parent --parent ROOT`` (a built checkout of the parent commit) writes ``profiles/strong_view_parent.txt``: in
alternating child processes, this tree and the parent, the flagship ``bench.py`` pre-train step and the criterion part of
``tools/diag/cps_time.py`` -- the change touches neither, so the two trees must agree within the box's run-to-run spread.

    python tools/diag/strong_view_time.py [--reps 200] [--rounds 4] [--part all|kernels|step|accuracy|parent]
        [--dtype bf16|fp32] [--parent ROOT] [--pairs 2]"""
import argparse
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cps_time import DEV, REPO, _batch, _call_sync, _captured, _epocher, _events, _rounds  # noqa: E402
from cps_cutmix_time import _parent_pairs  # noqa: E402

SEED = 23
OPS = ("gamma", "contrast", "brightness", "blur", "noise")


def _kernel_variants(N, dtype):
    from spcl_amd import functional as F_hip
    g = torch.Generator().manual_seed(SEED)
    x = torch.rand(N, 1, 224, 224, generator=g).to(dtype).to(DEV)
    flags = (torch.arange(N) % 4).to(torch.uint8).to(DEV)
    word = torch.tensor([SEED], dtype=torch.int32, device=DEV)
    cfg = F_hip.StrongViewConfig(**{name: {"p": 1.0} for name in OPS})
    table = F_hip.strong_view_params(x, word, cfg)
    neutral = torch.zeros_like(table)
    neutral[:, :3] = 1.0
    col = [table[:, k].view(N, 1, 1, 1).to(dtype) for k in range(8)]
    fh, fw = ((flags & 1) != 0).view(N, 1, 1, 1), ((flags & 2) != 0).view(N, 1, 1, 1)
    taps = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    kernel = torch.outer(taps, taps).view(1, 1, 5, 5).to(dtype).to(DEV)

    def torch_ops():
        a = x.clamp(0, 1).pow(col[0])
        a = ((a - col[7]) * col[1] + col[7]) * col[2]
        B = torch.nn.functional.conv2d(torch.nn.functional.pad(a, (2, 2, 2, 2), mode="replicate"), kernel, groups=1)
        a = a + col[3] * (B - a)
        a = (a + col[4] * torch.randn_like(a)).clamp(0, 1)
        a = torch.where(fh, a.flip(2), a)
        return torch.where(fw, a.flip(3), a)

    same = torch.equal(F_hip.strong_view_apply(x, flags, neutral), F_hip.flip_batch(x, flags))
    # the two formulations draw other noise: compare them with the noise column at zero
    quiet = table.clone()
    quiet[:, 4] = 0.0
    col[4] = quiet[:, 4].view(N, 1, 1, 1).to(dtype)
    diff = float((F_hip.strong_view_apply(x, flags, quiet).float() - torch_ops().float()).abs().max())
    col[4] = table[:, 4].view(N, 1, 1, 1).to(dtype)
    variants = [("flip_batch (the parent's launch)", lambda: F_hip.flip_batch(x, flags)),
                ("(a) params + apply", lambda: F_hip.strong_view(x, flags, word, cfg)),
                ("params alone", lambda: F_hip.strong_view_params(x, word, cfg)),
                ("apply alone", lambda: F_hip.strong_view_apply(x, flags, table)),
                ("apply, all-neutral table", lambda: F_hip.strong_view_apply(x, flags, neutral)),
                ("(b) torch ops", torch_ops)]
    note = (f"an all-neutral table is {'bit-equal to' if same else 'DIFFERENT from'} flip_batch; without noise the kernel and the "
            f"torch formulation differ by at most {diff:.2e}")
    return variants, note


def _step_variants(dtype):
    from spcl_amd.semi_seg import hooks as H
    lab, unl = _batch(5, 224, 1), _batch(5, 224, 2)
    pseudo = dict(weight=1.0, threshold=0.95, teacher="self")
    makers = [("no hook", lambda m: []),
              ("pseudolabel", lambda m: [H.create_pseudo_label_hook(model=m, **pseudo)]),
              ("pseudolabel + strongview", lambda m: [H.create_pseudo_label_hook(model=m, **pseudo),
                                                      H.create_strong_view_hook(seed=SEED)])]
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


def _accuracy():
    cmd = [sys.executable, "-m", "pytest", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
           os.path.join(REPO, "tests", "test_gpu_strong_view_kernels.py"), "-k", "apply_vs or apply_in_bf16 or table_is"]
    done = subprocess.run(cmd, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    lines = [line.strip().lstrip(".") for line in done.stdout.splitlines() if "strong_view " in line]
    tail = [line for line in done.stdout.splitlines() if " passed" in line or " failed" in line][-1:]
    return ["measured errors against tests/_strong_view_oracle.py (float64 pipeline; table: bit-equal draws, the mean in float32 "
            "spacings)"] + lines + tail


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--part", choices=("all", "kernels", "step", "accuracy", "parent"), default="all")
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16", help="compute dtype of the whole step")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for --part parent")
    ap.add_argument("--pairs", type=int, default=2, help="alternating pairs of child processes for --part parent")
    ap.add_argument("--out", default=None, help="default profiles/strong_view_time.txt (profiles/strong_view_parent.txt for "
                                                "--part parent); an empty string writes no file")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "strong_view_parent.txt" if args.part == "parent" else "strong_view_time.txt")
    lines = []
    if args.part == "parent":  # child processes only: this process never opens the device
        if not args.parent:
            raise SystemExit("--part parent needs --parent ROOT")
        lines = _parent_pairs(args)
    else:
        if args.part in ("all", "accuracy"):  # the child first: this process has not opened the device yet
            lines += _accuracy()
        sys.path.insert(0, REPO)
        if not torch.cuda.is_available():
            raise SystemExit("strong_view_time.py measures on the GPU: no device found")
        import spcl_amd  # noqa: F401
        from spcl_amd import native
        lines.insert(0, f"library {os.path.relpath(native.LIB_PATH, REPO)}, C ABI {native.ABI_VERSION}")
        if args.part in ("all", "kernels"):
            for N in (10, 32):
                for dtype in (torch.float32, torch.bfloat16):
                    variants, note = _kernel_variants(N, dtype)
                    es = 4 if dtype == torch.float32 else 2
                    lines.append(f"strong view of {N} x 1 x 224 x 224 {str(dtype).split('.')[-1]}, every gate open; {note}; apply "
                                 f"reads and writes {2 * N * 224 * 224 * es / 1e6:.1f} MB, params reads half of it")
                    graphs = [(name, _captured(fn).replay) for name, fn in variants]
                    lines.append(f"graph replays, {args.reps} per figure")
                    lines += _rounds(graphs, _events, args.reps, args.rounds, "us", 1e3)[0]
                    lines.append(f"call + synchronise (host clock), {args.reps} per figure")
                    lines += _rounds(variants, _call_sync, args.reps, args.rounds, "us", 1e3)[0]
        if args.part in ("all", "step"):
            n = max(10, args.reps // 5)
            dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
            steps = _step_variants(dtype)
            lines.append(f"semi-supervised step, compute dtype {args.dtype}, batch 5 + 5 + 5 x 1 x 224 x 224, eager, one process, "
                         f"{n} steps per figure")
            lines += _rounds(steps, _events, n, args.rounds, "us", 1e3)[0]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
