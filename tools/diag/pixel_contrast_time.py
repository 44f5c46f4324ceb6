"""Time the label-guided pixel contrast (csrc/pixel_contrast.hip, semi_seg/hooks/pixelcontrast.py) at the workload's size: 10
labelled slices of 224 x 224, C = 4 classes, K = 256 samples per class, d = 64, on the decoder features ``Up_conv3``
(32 channels x 112 x 112) and ``Up_conv2`` (16 channels x 224 x 224), bf16 channels-last as the UNet leaves them.

``--part kernels``: per feature
  * the sampler alone (``functional.pixel_sample``), and once the criterion alone (``functional.pixel_supcon`` with its
    backward on C K x d unit rows);
  * sample + gather + head + unit rows + criterion, forward + backward down to the feature's and the head's gradients;
  * a torch formulation of the same pipeline on the same device tensors: the key in int64 arithmetic, ``nonzero`` per class,
    key sort, index, two ``mm`` + leaky ReLU, ``normalize``, ``mm``, masks, ``logsumexp``, autograd's backward.
  each replayed from a captured graph and as call + synchronise.  ``nonzero`` synchronises and has a data-dependent shape:
  the torch formulation cannot be captured, and its graph column says so.
``--part step``: one ``SemiSupervisedEpocher`` step (``--dtype``, bf16 by default; 10 labelled + 5 + 5 unlabelled slices) without
  a hook and with the hook on either feature.  ``--tree PATH`` imports the package of another checkout (the parent commit,
  built there): it has no such hook, so only the hook-less step is timed; a job that alternates the two trees shows whether the
  two new keywords of ``regularization(...)`` cost anything.

Device events around replays, a host clock around call + synchronise; everything is warmed up first; the variants are timed
in alternating order, the order rotating from round to round, and every round is printed so that the spread shows.

    python tools/diag/pixel_contrast_time.py [--reps 200] [--rounds 4] [--part all|kernels|step] [--dtype bf16|fp32]
        [--tree PATH] [--out FILE] [--append]"""
import argparse
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"
B, C, K, D, HID, T = 10, 4, 256, 64, 128, 0.1
FEATURES = (("Up_conv3", 32, 112), ("Up_conv2", 16, 224))


def _events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _call_sync(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def _captured(fn, warmup=3):
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


def _blocky_labels(n, size, seed, block=16):
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randint(0, C, (n, 1, size // block, size // block), generator=g)
    return coarse.repeat_interleave(block, 2).repeat_interleave(block, 3)


def _torch_keys(n, seed):
    m = 0xFFFFFFFF
    h = (((torch.arange(n, dtype=torch.int64, device=DEV) + 1) * 0x9E3779B1) & m) ^ seed
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & m
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & m
    return h ^ (h >> 16)


def _kernel_variants(name, cf, hw):
    from spcl_amd import functional as F_hip
    g = torch.Generator().manual_seed(cf)
    feat = torch.randn(B, cf, hw, hw, generator=g).to(torch.bfloat16).to(DEV).contiguous(memory_format=torch.channels_last)
    labels = _blocky_labels(B, 224, 3).squeeze(1).to(torch.uint8).to(DEV)
    cell = F_hip.pixel_contrast_labels(labels, C, (hw, hw))
    word = torch.tensor([5], dtype=torch.int32, device=DEV)
    w1, b1 = (0.1 * torch.randn(HID, cf, 1, 1, generator=g)).to(DEV), torch.zeros(HID, device=DEV)
    w2, b2 = (0.1 * torch.randn(D, HID, 1, 1, generator=g)).to(DEV), torch.zeros(D, device=DEV)
    params = [p.requires_grad_(True) for p in (w1, b1, w2, b2)]
    unit = F_hip.register_unit_gradient(torch.ones((), device=DEV))
    kept = {}

    def sampler():
        kept["count"] = F_hip.pixel_sample(cell, C, K, word)[1]

    def hip():
        x = feat.detach().requires_grad_(True)
        idx, count = F_hip.pixel_sample(cell, C, K, word)
        rows = F_hip.gather_rows(x, idx)
        as_map = rows.view(C * K, 1, 1, cf).permute(0, 3, 1, 2)
        z = F_hip.l2norm_rows(F_hip.pixelwise_mlp(as_map, w1, b1, w2, b2).reshape(C * K, -1))
        loss = F_hip.pixel_supcon(z, count, K, T)
        kept["hip"] = loss.detach()
        kept["grads"] = torch.autograd.grad(loss, [x] + params, unit)

    def torch_ops():
        x = feat.detach().requires_grad_(True)
        flat = x.permute(0, 2, 3, 1).reshape(-1, cf)
        keys = _torch_keys(cell.numel(), 5)
        lab = cell.reshape(-1)
        rows, cls = [], []
        for c in range(C):
            cells = torch.nonzero(lab == c).reshape(-1)
            chosen = cells[torch.argsort(keys[cells])[:K]].sort().values
            rows.append(flat[chosen].float())
            cls.append(torch.full((chosen.numel(),), c, device=DEV))
        rows, cls = torch.cat(rows), torch.cat(cls)
        hid = torch.nn.functional.leaky_relu(rows @ w1.view(HID, cf).t() + b1, 0.01)
        z = torch.nn.functional.normalize(hid @ w2.view(D, HID).t() + b2, dim=1)
        s = (z @ z.t()) / T
        eye = torch.eye(len(z), dtype=torch.bool, device=DEV)
        pos = (cls[:, None] == cls[None, :]) & ~eye
        lse = torch.logsumexp(s.masked_fill(eye, float("-inf")), dim=1)
        npos = pos.sum(1)
        li = lse - (s * pos).sum(1) / npos.clamp_min(1)
        loss = (li * (npos > 0)).sum() / (npos > 0).sum().clamp_min(1)
        kept["torch"] = loss.detach()
        torch.autograd.grad(loss, [x] + params)

    sampler(), hip(), torch_ops()
    torch.cuda.synchronize()
    note = (f"{name}: feature {B} x {cf} x {hw} x {hw} bf16, {cell.numel()} cells, {int((cell >= 0).sum())} eligible, counts "
            f"{kept['count'].tolist()}; loss HIP {float(kept['hip']):.6f}, torch formulation {float(kept['torch']):.6f}")
    variants = [(f"{name} sampler", sampler, True), (f"{name} HIP pipeline", hip, True), (f"{name} torch pipeline", torch_ops, False)]
    return variants, note


def _criterion_variant():
    """the criterion alone, forward + backward, on C K unit rows with every slot valid"""
    from spcl_amd import functional as F_hip
    g = torch.Generator().manual_seed(1)
    z = torch.nn.functional.normalize(torch.randn(C * K, D, generator=g), dim=1).to(DEV)
    count = torch.full((C,), K, dtype=torch.int32, device=DEV)
    unit = F_hip.register_unit_gradient(torch.ones((), device=DEV))

    def criterion():
        x = z.detach().requires_grad_(True)
        torch.autograd.grad(F_hip.pixel_supcon(x, count, K, T), [x], unit)

    criterion()
    return (f"criterion alone {C * K} x {D}", criterion, True)


def _batch(n, size, seed):
    g = torch.Generator().manual_seed(seed)
    img, img_tf = torch.rand(n, 1, size, size, generator=g), torch.rand(n, 1, size, size, generator=g)
    tgt = _blocky_labels(n, size, seed + 100)
    names = [f"patient{k:03d}_00_{k}" for k in range(n)]
    return (tuple(t.to(DEV) for t in (img, img_tf, tgt, tgt.clone())), names, (["0"] * n, names))


def _epocher(hook_of, dtype):
    from spcl_amd import ddp
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.optim import FusedRAdam
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.epochers.semi import SemiSupervisedEpocher
    torch.manual_seed(0)
    model = UNet(input_dim=1, num_classes=C).to(DEV).train()
    model.set_compute_dtype(dtype)
    hooks = [h.to(DEV) for h in hook_of(model)]
    flat = ddp.FlatParams([p for p in model.parameters() if p.requires_grad] +
                          [p for h in hooks for p in h.parameters() if p.requires_grad])
    opt = FusedRAdam([flat.param], lr=1e-6, weight_decay=1e-5)
    ep = SemiSupervisedEpocher(model=model, optimizer=opt, labeled_loader=[], unlabeled_loader=[], sup_criterion=KL_div(),
                               num_batches=1, device=DEV, flat_params=flat)
    ep.add_hooks([h() for h in hooks])
    return ep


def _step_variants(dtype, tag):
    from spcl_amd.semi_seg import hooks as H
    lab, unl = _batch(B, 224, 1), _batch(5, 224, 2)
    makers = [(f"no hook [{tag}]", lambda m: [])]
    if hasattr(H, "create_pixel_contrast_hook"):
        for name, _, _ in FEATURES:
            makers.append((f"pixelcontrast {name} [{tag}]", lambda m, name=name: [H.create_pixel_contrast_hook(
                model=m, weight=1.0, feature_name=name, samples_per_class=K, temperature=T, hidden_dim=HID, output_dim=D)]))
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


def _rounds(variants, reps, rounds, unit, scale, timer=_events):
    lines, table = [], {name: [] for name, _ in variants}
    for r in range(rounds):
        order = variants[r % len(variants):] + variants[:r % len(variants)]
        for name, fn in order:
            table[name].append(timer(fn, reps) * scale)
        lines.append(f"round {r}: " + ", ".join(f"{name} {table[name][-1]:.1f} {unit}" for name, _ in variants))
    lines.append("min .. max: " + ", ".join(f"{name} {min(v):.1f} .. {max(v):.1f} {unit}" for name, v in table.items()))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--part", choices=("all", "kernels", "step"), default="all")
    ap.add_argument("--dtype", choices=("bf16", "fp32"), default="bf16", help="compute dtype of the whole step")
    ap.add_argument("--tree", default=None, help="another checkout whose package is timed (step part: the hook-less step)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pixel_contrast_time.txt"))
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pixel_contrast_time.py measures on the GPU: no device found")
    tree = os.path.abspath(args.tree) if args.tree else REPO
    sys.path.insert(0, tree)
    import spcl_amd  # noqa: F401
    from spcl_amd import native
    tag = "this tree" if tree == REPO else os.path.basename(tree.rstrip("/"))
    lines = [f"tree: {tag}, C ABI {native.ABI_VERSION}"]
    if args.part in ("all", "kernels") and tree == REPO:
        lines.append(f"C = {C}, K = {K}, d = {D}, hidden {HID}, t = {T}; {args.reps} per figure")
        every = []
        for name, cf, hw in FEATURES:
            variants, note = _kernel_variants(name, cf, hw)
            lines.append(note)
            every += variants
        every.append(_criterion_variant())
        graphs = [(name, _captured(fn).replay) for name, fn, capturable in every if capturable]
        lines.append("replayed from a graph (device events); the torch pipeline cannot be captured (nonzero):")
        lines += _rounds(graphs, args.reps, args.rounds, "us", 1e3)
        lines.append("call + synchronise (host clock):")
        lines += _rounds([(name, fn) for name, fn, _ in every], max(20, args.reps // 4), args.rounds, "us", 1e3, _call_sync)
    if args.part in ("all", "step"):
        steps = _step_variants(torch.bfloat16 if args.dtype == "bf16" else torch.float32, tag)
        n = max(10, args.reps // 5)
        lines.append(f"semi-supervised step, compute dtype {args.dtype}, batch {B} + 5 + 5 x 1 x 224 x 224, eager, {n} steps per "
                     "figure (device events)")
        lines += _rounds(steps, n, args.rounds, "us", 1e3)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
