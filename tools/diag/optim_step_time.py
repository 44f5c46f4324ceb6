"""What honouring ``Optim.name`` on the hot path costs or saves (contrastyou/trainer/base.py:60-69 builds
``optim.__dict__[name]``: RAdam, Adam, AdamW and SGD are all legal names).

Part ``optim``: for each of the four optimizers, the fused step's launches (optim.FusedRAdam / FusedAdam / FusedAdamW /
FusedSGD: a coefficient launch and one streaming kernel) against ``torch.optim``'s default (foreach) step, each on a flat
fp32 tensor of the pre-train flat parameter's size (the encoder of the base UNet + the projector of the self-paced hook).
The two run interleaved in one process: per round ``--reps`` steps of one, then of the other, between device events; the
figure is the median over ``--rounds`` rounds, with the rounds' extremes beside it.

Part ``step``: the pre-train step of the benchmark's flagship configuration (ACDC meta-label self-paced pre-training, base
UNet, bs 32 at 224^2, bf16 -- bench.py build_step's recipe) with the optimizer ``build_optimizer(--optim, ...)`` returns, on
the product loop ``PretrainEncoderEpocher.step``: host clock around ``--reps`` steps that end in a device synchronise, median
over ``--rounds`` rounds.  ``--tree DIR`` imports the package from another checkout (built there), and ``--against DIR``
runs this part in fresh child processes, alternating this checkout and DIR, ``--alternations`` times each: the way to compare
with a parent commit in which ``Optim.name: Adam`` still meant an eager ``torch.optim.Adam`` step.

    python tools/diag/optim_step_time.py --part optim
    python tools/diag/optim_step_time.py --part step --optim Adam [--against ../parent-checkout]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["optim", "step"], required=True)
    ap.add_argument("--optim", default="Adam")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--tree", default=HERE, help="checkout to import the package from (default: this one)")
    ap.add_argument("--against", default=None, help="part step: alternate child runs of this checkout and that one")
    ap.add_argument("--alternations", type=int, default=2)
    ap.add_argument("--json", action="store_true", help="part step: print one JSON line only")
    return ap.parse_args()


def _spread(xs):
    return f"{statistics.median(xs):.4f} (min {min(xs):.4f}, max {max(xs):.4f})"


def _build_pretrain():
    """bench.py build_step's model, hook and flat parameter (flagship configuration)"""
    import torch
    from spcl_amd import ddp
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.hooks import create_sp_infonce_hooks
    torch.manual_seed(10)
    model = UNet(input_dim=1, num_classes=4, max_channel=256, momentum=0.1).to(DEV)
    model.set_compute_dtype(torch.bfloat16)
    hook = create_sp_infonce_hooks(model=model, feature_names="Conv5", weights=1.0, contrast_ons="partition",
                                   begin_values=3.0, end_values=70.0, mode="soft", max_epoch=80, p=0.5, correct_grad=True,
                                   data_name="acdc", sync_checks=False).to(DEV)
    for sub in hook._hooks:
        sub._scheduler.epoch = 40
    for name in model.decoder_names:
        getattr(model, "_" + name).requires_grad_(False)
    flat = ddp.FlatParams([p for p in model.parameters() if p.requires_grad] + list(hook.parameters()))
    return model, hook, flat


def part_optim(args):
    import torch
    from spcl_amd import optim
    _, _, flat = _build_pretrain()
    n = flat.param.numel()
    del flat
    print(f"flat fp32 parameter of {n} elements; {args.reps} steps per round, {args.rounds} rounds, fused and torch.optim "
          f"(foreach) interleaved; device events, ms per step: median (min, max) over the rounds")
    cases = (("RAdam", optim.FusedRAdam, torch.optim.RAdam, dict(weight_decay=1e-5), 28),
             ("Adam", optim.FusedAdam, torch.optim.Adam, dict(weight_decay=1e-5), 28),
             ("AdamW", optim.FusedAdamW, torch.optim.AdamW, dict(weight_decay=1e-5), 28),
             ("SGD momentum=0.9", optim.FusedSGD, torch.optim.SGD, dict(weight_decay=1e-5, momentum=0.9), 20),
             ("SGD", optim.FusedSGD, torch.optim.SGD, dict(weight_decay=1e-5), 12))
    g = torch.Generator(device=DEV).manual_seed(1)
    for name, fused_cls, torch_cls, kw, bytes_per in cases:
        opts = []
        for cls in (fused_cls, torch_cls):
            p = torch.nn.Parameter(torch.randn(n, device=DEV, generator=g))
            p.grad = torch.randn(n, device=DEV, generator=g) * 1e-3
            opts.append(cls([p], lr=1e-4, **kw))
        for o in opts:
            for _ in range(args.warmup):
                o.step()
        torch.cuda.synchronize()
        times = ([], [])
        for _ in range(args.rounds):
            for o, ts in zip(opts, times):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.reps):
                    o.step()
                b.record()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b) / args.reps)
        f, t = statistics.median(times[0]), statistics.median(times[1])
        print(f"{name:17s} fused {_spread(times[0])} ms | torch.optim {_spread(times[1])} ms | torch / fused = {t / f:.2f} | "
              f"fused: {bytes_per} B/element -> {bytes_per * n / (f * 1e-3) / 1e9:.0f} GB/s incl. the coefficient launch")


def part_step(args):
    import random
    import torch
    from spcl_amd.semi_seg.epochers import PretrainEncoderEpocher
    from spcl_amd.semi_seg.trainers.pretrain import build_optimizer
    from spcl_amd.synthetic import SyntheticPretrainLoader
    model, hook, flat = _build_pretrain()
    opt = build_optimizer(args.optim, flat.param, {"lr": 5e-7 * 400, "weight_decay": 1e-5})
    loader = SyntheticPretrainLoader(bs=32, size=224, device=torch.device(DEV), seed=1234, resident=True, meta="acdc", pool=1)
    ep = PretrainEncoderEpocher(model=model, optimizer=opt, chain_dataloader=loader, num_batches=10 ** 9, device=DEV,
                                inference_until="Conv5", flat_params=flat)
    ep.add_hooks([hook()])
    model.train()
    random.seed(4321)
    per_round = []
    with ep.meters.focus_on(ep.meter_focus):
        for _ in range(args.warmup):
            ep.step(next(loader))
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            for _ in range(args.reps):
                ep.step(next(loader))
            torch.cuda.synchronize()
            per_round.append((time.perf_counter() - t0) / args.reps * 1e3)
    sg = ep._step_graph
    res = {"optim": args.optim, "optimizer_class": f"{type(opt).__module__}.{type(opt).__name__}",
           "graph_captured": bool(sg is not None and sg.captured), "replays": 0 if sg is None else sg.replays,
           "ms_per_step_rounds": [round(x, 4) for x in per_round], "ms_per_step_median": round(statistics.median(per_round), 4)}
    if args.json:
        print(json.dumps(res))
    else:
        print(f"pre-train step, bs 32 x 2 views x 224^2 bf16, Optim.name {args.optim} -> {res['optimizer_class']}, hipGraph "
              f"{'captured (%d replays)' % res['replays'] if res['graph_captured'] else 'NOT captured (eager launches)'}: "
              f"{_spread(per_round)} ms per step over {args.rounds} rounds of {args.reps} steps")
    return res


def part_step_against(args):
    """fresh child processes, this checkout and the other one in turn"""
    trees = {"this checkout": HERE, "other checkout": os.path.abspath(args.against)}
    runs = {k: [] for k in trees}
    for k in range(args.alternations):
        for label, tree in trees.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--part", "step", "--optim", args.optim, "--reps", str(args.reps),
                   "--rounds", str(args.rounds), "--warmup", str(args.warmup), "--tree", tree, "--json"]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit(f"child run of {label} failed ({out.returncode}):\n{out.stderr[-2000:]}")
            res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
            runs[label].append(res)
            print(f"run {k} {label}: {res['optimizer_class']}, graph captured {res['graph_captured']}, "
                  f"{res['ms_per_step_median']:.4f} ms per step (rounds {res['ms_per_step_rounds']})", flush=True)
    med = {k: statistics.median(r["ms_per_step_median"] for r in v) for k, v in runs.items()}
    print(f"Optim.name {args.optim}: this checkout {med['this checkout']:.4f} ms per step, other checkout "
          f"{med['other checkout']:.4f} ms per step; other / this = {med['other checkout'] / med['this checkout']:.2f}")


def main():
    args = _args()
    if args.part == "step" and args.against:
        return part_step_against(args)
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("optim_step_time.py measures on the GPU: no device found")
    import spcl_amd  # noqa: F401
    if args.part == "optim":
        part_optim(args)
    else:
        part_step(args)


if __name__ == "__main__":
    main()
