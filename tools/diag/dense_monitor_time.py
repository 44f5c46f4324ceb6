"""Time the dense pre-training monitor:

(a) ``functional.embedding_monitor(group=...)`` (``spcl_embed_monitor_grouped``) against the ungrouped call of the same build
    at (N, d, k) = (8100, 256, 20) -- 81 slices of 10 x 10 cells in 9 scans, the cells of a scan near each other --, both
    replayed from a captured graph;
(b) the grouped call against the plain torch formulation on the same device (normalize, ``mm``, group mask, ``topk``, vote);
(c) ``functional.cell_majority`` at 81 x 224 x 224, grid 10 x 10, against ``adaptive_avg_pool2d`` of the one-hot map plus
    arg-max;
(d) one whole ``DenseEmbeddingMonitor.run`` with a dense hook on ``Up_conv2`` and on ``Up_conv3`` (81 slices of 224 x 224, UNet
    in bf16, forwards included, one read-back), next to the time of 200 decoder pre-train steps of the same trainer.

Every figure of (a) - (c) is the median over ``--windows`` windows of ``--reps`` calls (smallest and largest window beside it)
after a warm-up, with the helpers of ``embed_monitor_time.py``.  The lines are printed and written to ``--out``.  No pass / fail
bar: where the HIP path loses, the line says so.

The profile file ends with a section this tool cannot measure in one checkout, "NULL-group path (the shipped monitor)":
``embed_monitor_time.py`` on the parent commit's build and on this one, in alternating runs on one box.  It is written by hand
from those runs' files and kept when this tool rewrites the lines above it.

    python tools/diag/dense_monitor_time.py [--reps 20] [--windows 7] [--out profiles/dense_monitor_time.txt]"""
import argparse
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
import embed_monitor_time as E  # noqa: E402  (the timing helpers: _wall, _replayed, _stat)

DEV = E.DEV
AB_MARKER = "NULL-group path (the shipped monitor)"
SLICES, GRID, SCAN_LEN = 81, (10, 10), 9
N, D, K, C = SLICES * GRID[0] * GRID[1], 256, 20, 4


def _inputs(seed=5):
    """cells of one scan scatter round the scan's class centres: a row's nearest rows lie in its own scan"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    scan = (torch.arange(N, device=DEV) // (GRID[0] * GRID[1])) // SCAN_LEN
    cls = torch.randint(0, C, (N,), device=DEV, generator=g)
    centres = torch.randn(C, D, device=DEV, generator=g)
    shift = 0.7 * torch.randn(int(scan.max()) + 1, D, device=DEV, generator=g)
    z = centres[cls] + shift[scan] + 0.5 * torch.randn(N, D, device=DEV, generator=g)
    return z, cls.to(torch.int32), scan.to(torch.int32)


def _torch_grouped(z, labels, group, k):
    """the torch formulation of the grouped vote -> (knn_idx, knn_sim, pred, correct)"""
    zh = torch.nn.functional.normalize(z, dim=1)
    s = zh @ zh.T
    s.masked_fill_(group[:, None] == group[None, :], -float("inf"))  # (the row itself is in its own group)
    sim, idx = s.topk(k, dim=1)
    nl = labels[idx]
    eq = nl[:, :, None] == nl[:, None, :]
    score = eq.sum(2) * (k + 1) - eq.float().argmax(2)
    pred = nl.gather(1, score.argmax(1, keepdim=True))[:, 0]
    return idx, sim, pred, (pred == labels).sum()


def _ratio(a, b):
    return statistics.median(a) / statistics.median(b)


def _call_lines(reps, windows):
    from spcl_amd import functional as F_hip
    z, labels, group = _inputs()
    lab64, grp64 = labels.long(), group.long()

    def grouped():
        return F_hip.embedding_monitor(z, labels, None, k=K, group=group)

    def plain():
        return F_hip.embedding_monitor(z, labels, None, k=K)

    def ref():
        return _torch_grouped(z, lab64, grp64, K)

    got, want = grouped(), ref()
    same = (f"neighbour tables equal at {float((got.knn_idx == want[0]).float().mean()) * 100:.3f} % of the entries, correct "
            f"{int(got.correct[0])} / {int(want[3])} of {N} (ungrouped call: {int(plain().correct[0])})")
    g_w, g_g = E._wall(grouped, reps, windows), E._replayed(grouped, reps, windows)
    p_w, p_g = E._wall(plain, reps, windows), E._replayed(plain, reps, windows)
    r_w, r_g = E._wall(ref, reps, windows), E._replayed(ref, reps, windows)
    g_t, p_t = E._kernel_table(grouped, reps), E._kernel_table(plain, reps)
    sweep = lambda t: next((us for name, us in t.items() if "sweep" in name), float("nan"))  # noqa: E731
    verdict = "the HIP call wins" if _ratio(r_g, g_g) > 1.0 else "the HIP call LOSES"
    return [f"(a), (b)  N = {N} ({SLICES} slices x {GRID[0]} x {GRID[1]} cells, {SLICES // SCAN_LEN} scans), d = {D}, k = {K}, L = 1, "
            f"no pairs; median of {windows} windows of {reps} calls (smallest - largest window)",
            f"      grouped call        call + synchronise {E._stat(g_w)}   replayed from a graph {E._stat(g_g)}",
            f"      ungrouped call      call + synchronise {E._stat(p_w)}   replayed from a graph {E._stat(p_g)}"
            f"   (grouped / ungrouped = {_ratio(g_g, p_g):.3f}x replayed; the sweep alone, by the library's launch timer: "
            f"{sweep(g_t):.1f} us against {sweep(p_t):.1f} us)",
            f"      torch ops, grouped  call + synchronise {E._stat(r_w)}   replayed from a graph {E._stat(r_g)}"
            f"   (torch / HIP = {_ratio(r_w, g_w):.2f}x eager, {_ratio(r_g, g_g):.2f}x replayed: {verdict}; the torch formulation "
            f"holds {2 * N * N * 4 / 1e6:.0f} MB of [N, N] matrices)",
            f"      {same}"]


def _majority_lines(reps, windows):
    from spcl_amd import functional as F_hip
    g = torch.Generator(device=DEV).manual_seed(7)
    coarse = torch.randint(0, C, (SLICES, 1, 14, 14), device=DEV, generator=g).float()
    maps = torch.nn.functional.interpolate(coarse, size=(224, 224), mode="nearest")[:, 0].to(torch.uint8).contiguous()

    def hip():
        return F_hip.cell_majority(maps, C, GRID, purity=True)

    def ref():
        share = torch.nn.functional.adaptive_avg_pool2d(
            torch.nn.functional.one_hot(maps.long(), C).permute(0, 3, 1, 2).float(), GRID)
        purity, label = share.max(1)
        return label, purity

    (label, purity), (want_label, want_purity) = hip(), ref()
    same = (f"labels equal at {float((label == want_label).float().mean()) * 100:.3f} % of the cells (the f32 averages may "
            f"order near-ties otherwise), largest purity difference {float((purity - want_purity).abs().max()):.2e}")
    h_w, h_g = E._wall(hip, reps, windows), E._replayed(hip, reps, windows)
    r_w, r_g = E._wall(ref, reps, windows), E._replayed(ref, reps, windows)
    verdict = "the HIP call wins" if _ratio(r_g, h_g) > 1.0 else "the HIP call LOSES"
    return [f"(c)  cell_majority, {SLICES} label maps of 224 x 224 (uint8, {C} classes), grid {GRID[0]} x {GRID[1]}: "
            f"{maps.numel() / 1e6:.1f} MB read",
            f"      cell_majority       call + synchronise {E._stat(h_w)}   replayed from a graph {E._stat(h_g)}"
            f"   ({maps.numel() / statistics.median(h_g) / 1e6:.1f} GB/s of label bytes)",
            f"      one-hot, pool, max  call + synchronise {E._stat(r_w)}   replayed from a graph {E._stat(r_g)}"
            f"   (torch / HIP = {_ratio(r_w, h_w):.2f}x eager, {_ratio(r_g, h_g):.2f}x replayed: {verdict})",
            f"      {same}"]


def _run_lines(rounds, steps):
    from spcl_amd import stepgraph
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.data.dataset import synthetic_slice_store
    from spcl_amd.semi_seg.data.loader import ContrastiveDeviceLoader
    from spcl_amd.semi_seg.data.rearr import ContrastBatchSampler
    from spcl_amd.semi_seg.hooks import create_infonce_hooks
    from spcl_amd.semi_seg.trainers import PretrainDecoderTrainer
    lines = []
    store = synthetic_slice_store(scans=60, slices_per_scan=(8, 11), size=256, device=DEV, seed=1)
    store.targets = (store.images * 4.0).clamp_(0, 3).to(torch.uint8)
    blocks = ["Up5", "Up_conv5", "Up4", "Up_conv4", "Up3", "Up_conv3", "Up2", "Up_conv2"]
    for feature in ("Up_conv3", "Up_conv2"):
        torch.manual_seed(3)
        net = UNet(input_dim=1, num_classes=4, max_channel=256).to(DEV)
        net.set_compute_dtype(torch.bfloat16)
        for p in net.parameters():
            p.requires_grad_(False)
        for name in blocks[:blocks.index(feature) + 1]:
            getattr(net, "_" + name).requires_grad_(True)
        sampler = ContrastBatchSampler(store, scan_sample_num=6, partition_sample_num=1)
        batch = len(next(iter(sampler)))
        loader = ContrastiveDeviceLoader(store, batch_sampler=sampler, out_hw=(224, 224))
        tr = PretrainDecoderTrainer(model=net, chain_dataloader=loader, max_epoch=4, num_batches=steps, device=DEV, lr=1e-6,
                                    save_dir=None, dense_monitor={"k": K})
        tr.register_hooks(create_infonce_hooks(model=net, feature_names=[feature], weights=1.0, contrast_ons="partition",
                                               data_name="acdc", sync_checks=False))
        tr.forward_until = feature
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.init()
        torch.cuda.synchronize()
        built = (time.perf_counter() - t0) * 1e3
        monitor = tr._dense_monitor
        epochs = []
        try:
            for epoch in (1, 2, 3):  # (epoch 1 captures the step and is not counted)
                tr._cur_epoch = epoch
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.run_tra_epoch()
                torch.cuda.synchronize()
                if epoch > 1:
                    epochs.append((time.perf_counter() - t0) * 1e3)
        finally:
            stepgraph.gc_release()
        times = []
        for r in range(rounds + 1):  # (round 0 warms every shape up and is not counted)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            result = monitor.run(net, tr.__hooks__)
            torch.cuda.synchronize()
            if r:
                times.append((time.perf_counter() - t0) * 1e3)
        rows = len(monitor.indices) * GRID[0] * GRID[1]
        per_200 = statistics.median(epochs) * 200.0 / steps
        lines += [f"(d)  DenseEmbeddingMonitor, one dense hook on {feature} ({net.get_channel_dim(feature)} channels), synthetic "
                  f"ACDC-like store with label maps ({len(store)} slices of 256 x 256), {len(monitor.indices)} slices as val views "
                  f"of 224 x 224 ({rows} rows), UNet (max_channel 256, bf16):",
                  f"      init() with the monitor (views, label maps, optimizer): {built:.1f} ms, once",
                  f"      one run, forwards in eval mode included, two embedding_monitor calls, one read-back: "
                  f"{E._stat(times, 'ms', 1.0)} over {rounds} runs",
                  f"      200 decoder pre-train steps of this trainer (batch {batch} slices in two views, "
                  f"measured over {steps} steps, median of two epochs): {per_200:.0f} ms -- one run is "
                  f"{statistics.median(times) / per_200 * 100:.1f} % of them",
                  "      " + ", ".join(f"{key} {value:.4f}" for key, value in sorted(result.items()) if key != "skipped")]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dense_monitor_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dense_monitor_time.py measures on the GPU: no device found")
    import spcl_amd  # noqa: F401
    lines = _call_lines(args.reps, args.windows) + _majority_lines(args.reps, args.windows)
    lines += _run_lines(args.rounds, args.steps)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    kept = ""
    if os.path.exists(args.out):  # the section this tool does not measure stays in the file (see the docstring)
        old = open(args.out).read()
        kept = old[old.index(AB_MARKER):] if AB_MARKER in old else ""
    with open(args.out, "w") as f:
        f.write(text + kept)


if __name__ == "__main__":
    main()
