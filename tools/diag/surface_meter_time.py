"""Time the Hausdorff meter at the inference pass's batch shape (16 slices of 224 x 224, C = 4, the three foreground classes
reported) on two inputs -- smooth blobs (a trained network's output: a few hundred border pixels per class) and per-pixel
uniform random labels (an untrained network's speckle: nearly every pixel is a border pixel, the worst case) --:

* ``SurfaceMeter.add`` + ``summary()`` on the device (``functional.surface_distances``: four launches, one read-back in
  ``summary()``), the device time of ``add`` alone between events and, in the first round, of each of its kernels (the
  library's launch timer);
* the reference's formulation in the same process (contrastyou/meters/surface_meter.py:109-128 and what medpy does under
  it): copy both maps to the host, then per (slice, class) scipy's ``binary_erosion`` for the two borders and two
  ``distance_transform_edt``, the gather, the maximum -- the baseline: no earlier version of this project computes this
  metric.

The cost of the HIP path must not depend on the number of border pixels beyond what they cost in the row pass and the
reductions: random / blobs for the HIP lines is the figure to read (an all-pairs search would be ~10^3 x).  Every shape is
warmed up first; each figure is the mean of ``--reps`` repetitions, the whole measurement is repeated ``--rounds`` times in
one process so that the spread shows.  The lines are printed and written to ``--out``.

    python tools/diag/surface_meter_time.py [--reps 10] [--rounds 3] [--out profiles/surface_meter_time.txt]"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
DEV = "cuda:0"
B, H, W, C, REPORT = 16, 224, 224, 4, [1, 2, 3]


def _blobs(seed):
    from scipy import ndimage
    rng = np.random.RandomState(seed)
    fields = np.stack([[ndimage.gaussian_filter(rng.randn(H, W), sigma=H / 8.0, mode="nearest") for _ in range(C)]
                       for _ in range(B)])
    return torch.from_numpy(fields.argmax(1).astype(np.int64))


def _random(seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, C, size=(B, H, W)).astype(np.int64))


def _host_reference(pred, target):
    """the reference's ``SurfaceMeter._evalue`` with ``hausdorff_distance``: device -> host, then per (slice, class)"""
    from scipy import ndimage
    cross = ndimage.generate_binary_structure(2, 1)
    p, t = pred.cpu().numpy(), target.cpu().numpy()
    out, borders = np.full((B, len(REPORT)), np.nan), 0
    for b in range(B):
        for r, c in enumerate(REPORT):
            a, g = p[b] == c, t[b] == c
            if not a.any() or not g.any():
                continue
            ba, bg = a & ~ndimage.binary_erosion(a, structure=cross), g & ~ndimage.binary_erosion(g, structure=cross)
            out[b, r] = max(ndimage.distance_transform_edt(~bg)[ba].max(), ndimage.distance_transform_edt(~ba)[bg].max())
            borders += int(ba.sum()) + int(bg.sum())
    return out, borders


def _wall(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def _device(fn, reps, warmup=2):
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
    """mean microseconds per call of every kernel symbol (the library's own launch timer, ``spcl_profile_*``)"""
    from spcl_amd import native as n
    fn()
    torch.cuda.synchronize()
    n.call("spcl_profile_enable", 1)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    name = ctypes.create_string_buffer(256)
    us, by, fl = ctypes.c_float(), ctypes.c_double(), ctypes.c_double()
    acc = {}
    for i in range(n.call("spcl_profile_count")):
        n.call("spcl_profile_get", i, name, 256, ctypes.byref(us), ctypes.byref(by), ctypes.byref(fl))
        acc[name.value.decode()] = acc.get(name.value.decode(), 0.0) + us.value
    n.call("spcl_profile_enable", 0)
    return sorted(((k, v / reps) for k, v in acc.items()), key=lambda r: -r[1])


def _times(name, pred, target, reps, table):
    from spcl_amd.contrastyou.meters import SurfaceMeter
    meter = SurfaceMeter(C=C, report_axises=REPORT, metername="hausdorff")

    def hip():
        meter.reset()
        meter.add(pred, target)
        return meter.summary()

    def hip_add():
        meter.reset()
        meter.add(pred, target)

    got = hip()
    ref, border = _host_reference(pred, target)
    same = all(got[f"HD{c}"] == ref.mean(0)[r] for r, c in enumerate(REPORT)) if not np.isnan(ref).any() else None
    t_hip, t_add, t_host = _wall(hip, reps), _device(hip_add, reps), _wall(lambda: _host_reference(pred, target), max(1, reps // 5), 1)
    return (f"{name}: SurfaceMeter add + summary {t_hip:.3f} ms (add alone, device time {t_add:.3f} ms), host scipy per "
            f"(slice, class) {t_host:.1f} ms (host / HIP = {t_host / t_hip:.0f}x; HD equal to the host's: {same}; "
            f"{border} border pixels in the {B * len(REPORT)} pairs)"), t_hip, t_add, _kernel_table(hip_add, reps) if table else []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "surface_meter_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("surface_meter_time.py measures on the GPU: no device found")
    import spcl_amd  # noqa: F401
    inputs = {"smooth blobs": (_blobs(1).to(DEV), _blobs(2).to(DEV)), "random labels": (_random(3).to(DEV), _random(4).to(DEV))}
    lines = [f"SurfaceMeter(hausdorff) on {B} x {H} x {W} class-coded maps, C = {C}, classes {REPORT} reported; {args.reps} reps "
             f"per figure (host reference: {max(1, args.reps // 5)})"]
    for r in range(args.rounds):
        res = {name: _times(name, p, t, args.reps, table=r == 0) for name, (p, t) in inputs.items()}
        lines.append(f"round {r}")
        for v in res.values():
            lines.append("  " + v[0])
            lines.extend(f"      {us:8.1f} us  {k}" for k, us in v[3])
        lines.append(f"  random labels / smooth blobs on the HIP path: add + summary {res['random labels'][1] / res['smooth blobs'][1]:.2f}x, "
                     f"add alone {res['random labels'][2] / res['smooth blobs'][2]:.2f}x")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
