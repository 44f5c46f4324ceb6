"""Time the pre-training monitor:

* ``functional.embedding_monitor`` (four launches + one memset, no [N, N] matrix) against the plain torch formulation of the
  same outputs on the same device -- normalise, ``mm``, masks, ``topk``, label gathers, a vectorised vote, ``exp``, sums --,
  both eagerly (call + synchronise) and replayed from a captured graph (device time between events), at
  (N, d, k) = (1024, 256, 20), (4096, 128, 20) and (8192, 256, 32), three label kinds, the two-view pair layout;
* the library's kernels alone, by its own launch timer;
* one ``EmbeddingMonitor.run`` on a synthetic ACDC-like store (512 slices in two views of 224 x 224, UNet in bf16, two hooks
  on ``Conv5``), forwards included.

Every figure is the median over ``--windows`` windows of ``--reps`` calls each (smallest and largest window beside it), after
a warm-up of every shape; the two formulations' results are compared first (they may differ at near-ties: the torch
formulation breaks them as ``topk`` does).  The lines are printed and written to ``--out``.  No pass / fail bar.

    python tools/diag/embed_monitor_time.py [--reps 20] [--windows 7] [--out profiles/embed_monitor_time.txt]"""
import argparse
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
DEV = "cuda:0"
SHAPES = ((1024, 256, 20), (4096, 128, 20), (8192, 256, 32))


def _torch_monitor(z, labels, pair, k):
    """the torch formulation (ties as ``topk`` / ``>`` leave them) -> (knn_idx, knn_sim, pred, correct, pair_rank, scalars)"""
    N = z.shape[0]
    zh = torch.nn.functional.normalize(z, dim=1)
    s = zh @ zh.T
    sp = s.gather(1, pair[:, None])
    e = torch.exp(-4.0 * (1.0 - s))
    uniform = ((e.sum(dtype=torch.float64) - e.diagonal().sum(dtype=torch.float64)) / (N * (N - 1))).log()
    align = (2.0 - 2.0 * sp).mean(dtype=torch.float64)
    masked = s.clone().fill_diagonal_(-float("inf")).scatter_(1, pair[:, None], -float("inf"))
    rank = (masked > sp).sum(1)
    sim, idx = masked.topk(k, dim=1)
    preds = []
    for lab in labels:
        nl = lab[idx]  # [N, k]
        eq = nl[:, :, None] == nl[:, None, :]
        score = eq.sum(2) * (k + 1) - eq.float().argmax(2)  # the count, then the rank of the label's first neighbour
        preds.append(nl.gather(1, score.argmax(1, keepdim=True))[:, 0])
    pred = torch.stack(preds)
    correct = (pred == labels).sum(1)
    scalars = torch.stack([align, uniform, align.new_full((), float(N)),
                           z.norm(dim=1).min().double()])
    return idx, sim, pred, correct, rank, scalars


def _stat(samples, unit="us", scale=1e3):
    s = sorted(samples)
    return f"{statistics.median(s) * scale:.1f} {unit} ({s[0] * scale:.1f} - {s[-1] * scale:.1f})"


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
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
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


def _kernel_table(fn, reps):
    """{kernel symbol: mean microseconds per call of ``fn``} from the library's launch timer (``spcl_profile_*``)"""
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
    table = {}
    for i in range(n.call("spcl_profile_count")):
        n.call("spcl_profile_get", i, name, 256, ctypes.byref(us), ctypes.byref(by), ctypes.byref(fl))
        key = name.value.decode()
        table[key] = table.get(key, 0.0) + us.value / reps
    n.call("spcl_profile_enable", 0)
    return table


def _inputs(N, d, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    M = N // 2
    which = torch.randint(0, 24, (M,), device=DEV, generator=g)
    centres = torch.randn(24, d, device=DEV, generator=g)
    half = centres[which] + 0.5 * torch.randn(M, d, device=DEV, generator=g)
    z = torch.cat([half, half + 0.2 * torch.randn(M, d, device=DEV, generator=g)])
    labels = torch.stack([which % 3, which, which % 2]).repeat(1, 2).to(torch.int32)
    pair = ((torch.arange(N, device=DEV) + M) % N).to(torch.int32)
    return z, labels, pair


def _call_lines(reps, windows):
    from spcl_amd import functional as F_hip
    lines = []
    for N, d, k in SHAPES:
        z, labels, pair = _inputs(N, d, seed=N + d)
        lab64, pair64 = labels.long(), pair.long()
        got, want = F_hip.embedding_monitor(z, labels, pair, k=k), _torch_monitor(z, lab64, pair64, k)
        same = (f"neighbour tables equal at {float((got.knn_idx == want[0]).float().mean()) * 100:.3f} % of the entries, "
                f"correct {got.correct.tolist()} / {want[3].tolist()}, pair_rank equal at "
                f"{float((got.pair_rank == want[4]).float().mean()) * 100:.3f} % of the rows, alignment "
                f"{float(got.scalars[0]):.6f} / {float(want[5][0]):.6f}, uniformity {float(got.scalars[1]):.6f} / "
                f"{float(want[5][1]):.6f}")

        def hip():
            return F_hip.embedding_monitor(z, labels, pair, k=k)

        def ref():
            return _torch_monitor(z, lab64, pair64, k)

        hip_w, hip_g = _wall(hip, reps, windows), _replayed(hip, reps, windows)
        ref_w, ref_g = _wall(ref, reps, windows), _replayed(ref, reps, windows)
        table = _kernel_table(hip, reps)
        kernels = ", ".join(f"{name.split('(')[0].split('::')[-1]} {us:.1f}" for name, us in table.items())
        flops = 2.0 * N * N * d
        sweep = next((us for name, us in table.items() if "sweep" in name), float("nan"))
        lines.append(f"  N = {N}, d = {d}, k = {k}, L = 3, paired")
        lines.append(f"      embedding_monitor   call + synchronise {_stat(hip_w)}   replayed from a graph {_stat(hip_g)}")
        lines.append(f"      torch ops           call + synchronise {_stat(ref_w)}   replayed from a graph {_stat(ref_g)}"
                     f"   (torch / HIP = {statistics.median(ref_w) / statistics.median(hip_w):.2f}x eager, "
                     f"{statistics.median(ref_g) / statistics.median(hip_g):.2f}x replayed)")
        lines.append(f"      kernels alone, us: {kernels}   (the sweep: {flops / sweep / 1e6:.1f} TFLOP/s of exact-f32 products; "
                     f"the torch formulation holds {3 * N * N * 4 / 1e6:.0f} MB of [N, N] f32 matrices)")
        lines.append(f"      {same}")
    return lines


def _run_lines(rounds):
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.data.dataset import synthetic_slice_store
    from spcl_amd.semi_seg.epochers import EmbeddingMonitor
    from spcl_amd.semi_seg.hooks import create_sp_infonce_hooks
    torch.manual_seed(3)
    net = UNet(input_dim=1, num_classes=4, max_channel=256).to(DEV)
    net.set_compute_dtype(torch.bfloat16)
    store = synthetic_slice_store(scans=60, slices_per_scan=(8, 11), size=256, device=DEV, seed=1)
    hooks = create_sp_infonce_hooks(model=net, feature_names=["Conv5"] * 2, weights=[1.0, 1.0],
                                    contrast_ons=["partition", "patient"], begin_values=5.0, end_values=50.0, mode="soft",
                                    max_epoch=10, p=0.5, correct_grad=True, data_name="acdc", sync_checks=False).to(DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    monitor = EmbeddingMonitor(store, max_slices=512, k=20)
    torch.cuda.synchronize()
    built = (time.perf_counter() - t0) * 1e3
    net.train()
    times = []
    for r in range(rounds + 1):  # (round 0 warms every shape up and is not counted)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result = monitor.run(net, [hooks])
        torch.cuda.synchronize()
        if r:
            times.append((time.perf_counter() - t0) * 1e3)
    n_calls = len({key.rsplit("/", 1)[0] for key in result if key != "skipped"})
    return [f"EmbeddingMonitor on a synthetic ACDC-like store ({len(store)} slices of 256 x 256), {len(monitor.indices)} slices in "
            f"two views of 224 x 224 ({monitor.images.shape[0]} rows), UNet (max_channel 256, bf16, untrained), two hooks on Conv5:",
            f"  construction (both views drawn and kept on the device): {built:.1f} ms, once",
            f"  one run, forwards in eval mode included, {n_calls} embedding_monitor calls (N = {monitor.images.shape[0]}, "
            f"d = 256), one read-back: {_stat(times, 'ms', 1.0)} over {rounds} runs",
            "  keys: " + ", ".join(sorted(key for key in result if key != "skipped"))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "embed_monitor_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("embed_monitor_time.py measures on the GPU: no device found")
    import spcl_amd  # noqa: F401
    lines = [f"functional.embedding_monitor against the torch formulation (normalize, mm, masks, topk, gathers, vote, exp, sums) "
             f"on clustered rows of uneven cluster size, f32; median of {args.windows} windows of {args.reps} calls (smallest - "
             f"largest window)"]
    lines += _call_lines(args.reps, args.windows)
    lines += _run_lines(args.rounds)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
