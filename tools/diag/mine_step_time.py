"""Time one call of the MINE estimator with its backward at three positions of the 224 x 224 UNet -- ``Conv5`` (256 channels,
14 x 14: the reference's position), ``Up_conv4`` (64 channels, 56 x 56) and ``Up_conv3`` (32 channels, 112 x 112) -- at the
unlabelled batch size of the other step-time tools (5 slices, so a feature of 10 samples), in f32 and bf16, three ways on the
same device:

* (a) the fused path: ``MineEstimator.from_feature`` (csrc/mine.hip around the conv3x3 + BatchNorm + ReLU kernels);
* (b) the composition of the ops the package had before: ``flip_batch`` / ``torch.roll`` / ``torch.cat``, the same
  ``conv_bn_relu`` calls, ``adaptive_pool2d(., "max")`` and torch's ``linear`` / ``softplus`` / ``mean``
  (tests/_mine_oracle.composed_on_device);
* (c) torch's own ``nn.Sequential`` of the reference (stock ``nn.Conv2d`` / ``nn.BatchNorm2d`` / ...), with torch's ``flip`` /
  ``cat``, in the same storage dtype (channels-last);

with the library's own launch timer for (a) (``spcl_profile_*``: mean microseconds and launches per call of every kernel
symbol).  Then one whole ``SemiSupervisedEpocher`` step (5 + 5 slices of 224 x 224, flat parameters, fused RAdam) without a
hook, with the ``Conv5`` hook, and with the ``Conv5`` + ``Up_conv3`` hooks.

Every figure is the mean of its repetitions after a warm-up; the measurement is repeated ``--rounds`` times in one process so
that the spread shows.  Lines are printed as they come and written to ``--out`` at the end.  No pass / fail bar.

    python tools/diag/mine_step_time.py [--reps 20] [--rounds 3] [--out profiles/mine_step_time.txt]"""
import argparse
import copy
import ctypes
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
DEV = "cuda:0"
N, HW = 5, 224
POSITIONS = (("Conv5", 256, 14), ("Up_conv4", 64, 56), ("Up_conv3", 32, 112))
FLAGS = [0, 1, 2, 3, 1]


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


def _kernel_table(fn, reps):
    from spcl_amd import native as n
    fn()
    torch.cuda.synchronize()
    n.call("spcl_profile_enable", 1)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    cnt = n.call("spcl_profile_count")
    name = ctypes.create_string_buffer(256)
    us, by, fl = ctypes.c_float(), ctypes.c_double(), ctypes.c_double()
    acc = {}
    for i in range(cnt):
        n.call("spcl_profile_get", i, name, 256, ctypes.byref(us), ctypes.byref(by), ctypes.byref(fl))
        a = acc.setdefault(name.value.decode(), [0.0, 0])
        a[0] += us.value
        a[1] += 1
    n.call("spcl_profile_enable", 0)
    return sorted(((k, v[0] / reps, v[1] / reps) for k, v in acc.items()), key=lambda r: -r[1])


def _estimator_calls(say, reps, table):
    from spcl_amd import config
    from spcl_amd.semi_seg.mi_estimator import MineEstimator
    from tests import _mine_oracle as M
    before = config.get_compute_dtype()
    flags = torch.tensor(FLAGS, dtype=torch.uint8, device=DEV)
    flips = [[d for d, bit in ((1, 1), (2, 2)) if f & bit] for f in FLAGS]
    try:
        for name, C, size in POSITIONS:
            for dtype in (torch.float32, torch.bfloat16):
                config.set_compute_dtype(dtype)
                torch.manual_seed(10)
                fused = MineEstimator(layer_name=name, input_dim=C).to(DEV).train()
                composed = copy.deepcopy(fused)
                stock = M.projector(C)
                stock.load_state_dict({k.split(".", 1)[1]: v.cpu() for k, v in fused.state_dict().items()})
                stock = stock.to(DEV).to(dtype).to(memory_format=torch.channels_last).train()
                g = torch.Generator().manual_seed(1)
                feat = torch.randn(2 * N, C, size, size, generator=g).to(dtype).to(DEV)
                feat = feat.contiguous(memory_format=torch.channels_last)
                out = {}

                def run_fused():
                    x = feat.detach().requires_grad_(True)
                    loss = fused.from_feature(x, flags)
                    loss.backward()
                    out.setdefault("fused", float(loss.detach()))

                def run_composed():
                    x = feat.detach().requires_grad_(True)
                    loss = M.composed_on_device(composed, x, flags)
                    loss.backward()
                    out.setdefault("composed", float(loss.detach()))

                def run_stock():
                    x = feat.detach().requires_grad_(True)
                    feat1 = x[N:]
                    feat2 = torch.stack([torch.flip(s, d) if d else s for s, d in zip(x[:N], flips)], 0)
                    feat2_prime = torch.cat([feat2[1:], feat2[0:1]], 0)
                    ej = -torch.nn.functional.softplus(stock(torch.cat([feat1, feat2], 1)).float()).mean()
                    em = torch.nn.functional.softplus(stock(torch.cat([feat1, feat2_prime], 1)).float()).mean()
                    loss = em - ej
                    loss.backward()
                    out.setdefault("stock", float(loss.detach()))

                ta, tb, tc = _time(run_fused, reps), _time(run_composed, reps), _time(run_stock, reps)
                tag = "f32" if dtype == torch.float32 else "bf16"
                say(f"{name} ({C} ch, {size} x {size}, feature of {2 * N}) {tag}: one call forward + backward: (a) fused "
                    f"{ta * 1e3:.0f} us, (b) composed from existing ops {tb * 1e3:.0f} us, (c) torch nn.Sequential "
                    f"{tc * 1e3:.0f} us; a / b = {ta / tb:.2f}, a / c = {ta / tc:.2f}; first losses {out['fused']:.5f} / "
                    f"{out['composed']:.5f} / {out['stock']:.5f}")
                if table:
                    rows = _kernel_table(run_fused, max(2, reps // 4))
                    say(f"  (a) library kernels per call (launch timer; sum {sum(r[1] for r in rows):.0f} us, "
                        f"{sum(r[2] for r in rows):.0f} launches):")
                    for k, us, cnt in rows:
                        say(f"    {us:9.1f} us  {cnt:5.1f} launches  {k}")
                    rows = _kernel_table(run_composed, max(2, reps // 4))
                    say(f"  (b) library kernels per call (torch's own launches not counted; sum {sum(r[1] for r in rows):.0f} us, "
                        f"{sum(r[2] for r in rows):.0f} launches)")
    finally:
        config.set_compute_dtype(before)


def _whole_steps(say, reps):
    from spcl_amd import ddp as _ddp
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.optim import FusedRAdam
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.epochers.semi import SemiSupervisedEpocher
    from spcl_amd.semi_seg.hooks import create_mine_hooks

    def batch(seed):
        g = torch.Generator().manual_seed(seed)
        img, img_tf = torch.rand(N, 1, HW, HW, generator=g).to(DEV), torch.rand(N, 1, HW, HW, generator=g).to(DEV)
        tgt = torch.randint(0, 4, (N, 1, HW, HW), generator=g).to(DEV)
        names = [f"patient{k:03d}_00_{k}" for k in range(N)]
        return (img, img_tf, tgt, tgt.clone()), names, (["0"] * N, names)

    from spcl_amd import config
    lab, unl = batch(1), batch(2)
    before = config.get_compute_dtype()
    try:
        for dtype in (torch.float32, torch.bfloat16):
            config.set_compute_dtype(dtype)
            _whole_steps_of(say, reps, dtype, lab, unl, UNet, create_mine_hooks, _ddp, FusedRAdam, SemiSupervisedEpocher, KL_div)
    finally:
        config.set_compute_dtype(before)


def _whole_steps_of(say, reps, dtype, lab, unl, UNet, create_mine_hooks, _ddp, FusedRAdam, SemiSupervisedEpocher, KL_div):
    res = {}
    for kind, features in (("no hook", ()), ("Conv5", ("Conv5",)), ("Conv5 + Up_conv3", ("Conv5", "Up_conv3"))):
        torch.manual_seed(3)
        model = UNet(input_dim=1, num_classes=4).to(DEV).train()
        model.set_compute_dtype(dtype)
        params = list(model.parameters())
        hooks = []
        if features:
            th = create_mine_hooks(model=model, feature_names=list(features), weights=[0.1] * len(features))
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
        if features:  # the positions timed above are the features the hooks really see
            seen = {h._feature_name: tuple(h._extractor.feature()[-2 * N:].shape) for h in th._hooks}
            want = {name: (2 * N, C, size, size) for name, C, size in POSITIONS if name in features}
            assert seen == want, (seen, want)
        ep.close_hooks()
    say(f"whole SemiSupervisedEpocher step at {N} + {N} slices of {HW} x {HW}, {'f32' if dtype == torch.float32 else 'bf16'}: "
        + ", ".join(f"{k} {v:.2f} ms" for k, v in res.items()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mine_step_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mine_step_time.py measures on the GPU: no device found")
    import spcl_amd  # noqa: F401
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"MINE estimator on the feature of {N} unlabelled slices and their transformed copies; {args.reps} reps per figure")
    for r in range(args.rounds):
        say(f"round {r}")
        _estimator_calls(say, args.reps, table=(r == 0))
        _whole_steps(say, args.reps)
    with open(args.out, "w") as out:  # (written once, at the end: a run that fails midway leaves no truncated file)
        out.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
