"""Time test-time augmentation at the inference pass's size (one scan of 10 slices of 224 x 224, C = 4):

* the merge alone: ``functional.tta_merge`` (one launch + the ticket's memset) against the torch formulation of the same four
  outputs on the same device -- un-flip / un-swap every view's logits, softmax, stack, mean, arg-max, entropy, mean --, both
  eagerly (call + synchronise) and replayed from a captured graph (device time between events, the host's launch rate out of
  the picture).  V = 4 ("flips") and V = 8 ("dihedral"); to price the axis swap, whose reads walk a column of the view (stride
  W C floats), also four and eight views that are all flipped only and four and eight that are all swapped.
* a whole ``InferenceEpocher`` pass (the UNet in bf16, PNG writes included) over synthetic scans -- the smooth-blob label maps
  of tests/_lcc_oracle.py, the image carrying the labels plus noise -- with ``tta=None``, ``"flips"`` and ``"dihedral"``,
  alternating.

Every figure is the median over ``--windows`` windows of ``--reps`` calls each (smallest and largest window beside it), after
a warm-up of every shape; the two formulations' results are compared first.  The lines are printed and written to ``--out``.
No pass / fail bar.

    python tools/diag/tta_time.py [--reps 50] [--windows 9] [--out profiles/tta_time.txt]"""
import argparse
import math
import os
import statistics
import sys
import tempfile
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
DEV = "cuda:0"
N, C, H, W = 10, 4, 224, 224
OP_SETS = (("V = 4, flips (ops 0 1 2 3)", (0, 1, 2, 3)), ("V = 4, all swapped (ops 4 5 6 7)", (4, 5, 6, 7)),
           ("V = 8, dihedral (ops 0 .. 7)", tuple(range(8))), ("V = 8, flipped only (ops 0 1 2 3 0 1 2 3)", (0, 1, 2, 3) * 2),
           ("V = 8, all swapped (ops 4 5 6 7 4 5 6 7)", (4, 5, 6, 7) * 2))


def _torch_merge(view_logits, ops, eps=1e-16):
    """the torch formulation: logical [N, C, H, W] maps in their views' frames -> (prob, pred, entropy, mean entropy)"""
    rows = []
    for t, op in zip(view_logits, ops):
        if op & 4:
            t = t.transpose(-1, -2)
        dims = [d for d, bit in ((-1, 2), (-2, 1)) if op & bit]
        if dims:
            t = torch.flip(t, dims=dims)
        rows.append(torch.softmax(t, dim=1))
    prob = torch.stack(rows).mean(0)
    pred = prob.argmax(1)
    entropy = -(prob * torch.log(prob + eps)).sum(1) / math.log(prob.shape[1])
    return prob, pred, entropy, entropy.mean()


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


def _kernel_us(fn, reps):
    """mean microseconds per call of the library's kernels inside ``fn`` (its own launch timer, ``spcl_profile_*``: events
    around every launch, so the memset and the gaps between launches are not in it)"""
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
    total = 0.0
    for i in range(n.call("spcl_profile_count")):
        n.call("spcl_profile_get", i, name, 256, ctypes.byref(us), ctypes.byref(by), ctypes.byref(fl))
        total += us.value
    n.call("spcl_profile_enable", 0)
    return total / reps


def _merge_lines(reps, windows):
    from spcl_amd import functional as F_hip
    g = torch.Generator(device=DEV).manual_seed(5)
    maps = [(3 * torch.randn((N, H, W, C), device=DEV, generator=g)).permute(0, 3, 1, 2) for _ in range(8)]
    lines = []
    for name, ops in OP_SETS:
        views = maps[:len(ops)]
        got, want = F_hip.tta_merge(views, ops), _torch_merge(views, ops)
        same = (f"arg-max equal at {float((got[1] == want[1]).float().mean()) * 100:.4f} % of the pixels, largest probability "
                f"difference {float((got[0] - want[0]).abs().max()):.1e}, mean entropy {float(got[3]):.7f} / {float(want[3]):.7f}")

        def hip():
            return F_hip.tta_merge(views, ops)

        def ref():
            return _torch_merge(views, ops)

        hip_w, hip_g = _wall(hip, reps, windows), _replayed(hip, reps, windows)
        ref_w, ref_g = _wall(ref, reps, windows), _replayed(ref, reps, windows)
        kernel = _kernel_us(hip, reps)
        moved = (len(ops) + 1) * N * H * W * C * 4 + 12 * N * H * W
        lines.append(f"  {name}")
        lines.append(f"      tta_merge   call + synchronise {_stat(hip_w)}   replayed from a graph {_stat(hip_g)}"
                     f"   the kernel alone {kernel:.1f} us ({moved / 1e6:.1f} MB moved: {moved / kernel / 1e6:.2f} TB/s)")
        lines.append(f"      torch ops   call + synchronise {_stat(ref_w)}   replayed from a graph {_stat(ref_g)}"
                     f"   (torch / HIP = {statistics.median(ref_w) / statistics.median(hip_w):.1f}x eager, "
                     f"{statistics.median(ref_g) / statistics.median(hip_g):.1f}x replayed)")
        lines.append(f"      {same}")
    return lines


class _Scans:
    def __init__(self, n_scans):
        from tests import _lcc_oracle as O
        g = torch.Generator(device=DEV).manual_seed(9)
        self.items = []
        for i in range(n_scans):
            tgt = torch.from_numpy(O.smooth_blobs((1, N, H, W), C, seed=11 + i)[0]).to(DEV).unsqueeze(1)
            img = (tgt.float() / 4 + 0.1 + 0.05 * torch.randn(tgt.shape, device=DEV, generator=g)).clamp(0, 1)
            names = [f"scan{i:02d}_{k:02d}" for k in range(N)]
            self.items.append(((img, tgt), names, ([0] * N, [f"scan{i:02d}"] * N)))

    def __len__(self):
        return len(self.items)

    def __iter__(self):
        return iter(self.items)


def _pass_lines(n_scans, rounds):
    from spcl_amd import functional as F_hip
    from spcl_amd.contrastyou.losses.kl import KL_div
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.epochers import InferenceEpocher
    torch.manual_seed(3)
    model = UNet(input_dim=1, num_classes=C, max_channel=256).to(DEV).eval()
    model.set_compute_dtype(torch.bfloat16)
    loader = _Scans(n_scans)
    times, stats = {None: [], "flips": [], "dihedral": []}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(rounds + 1):  # (round 0 warms every shape up and is not counted)
            for mode in times:
                ep = InferenceEpocher(model=model, loader=loader, sup_criterion=KL_div(verbose=False), device=DEV, tta=mode)
                ep.init(save_dir=os.path.join(tmp, str(mode)))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                stats[mode] = ep.run()["eval"]
                torch.cuda.synchronize()
                if r:
                    times[mode].append((time.perf_counter() - t0) / n_scans * 1e3)
    base = statistics.median(times[None])
    lines = [f"whole InferenceEpocher pass, UNet (max_channel 256, bf16, untrained), {n_scans} scans of {N} x {H} x {W}, PNG writes "
             f"included, ms per scan, median of {rounds} alternating rounds (smallest - largest):"]
    for mode, t in times.items():
        extra = ""
        if mode is not None:
            extra = (f"   (+{statistics.median(t) - base:.1f} ms for {len(F_hip.TTA_MODES[mode]) - 1} more forwards, the merge, its "
                     f"meters and two more PNG folders; tta_changed {stats[mode]['tta_changed']['mean']:.4f}, tta_entropy "
                     f"{stats[mode]['tta_entropy']['mean']:.4f})")
        lines.append(f"  tta={mode!r}: {_stat(t, 'ms', 1.0)}{extra}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--scans", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tta_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tta_time.py measures on the GPU: no device found")
    import spcl_amd  # noqa: F401
    lines = [f"functional.tta_merge against the torch formulation (un-flip, softmax, stack, mean, arg-max, entropy, mean) on one "
             f"scan of {N} x {H} x {W}, C = {C}, f32 channels-last logits; median of {args.windows} windows of {args.reps} calls "
             f"(smallest - largest window)"]
    lines += _merge_lines(args.reps, args.windows)
    lines += _pass_lines(args.scans, args.rounds)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
