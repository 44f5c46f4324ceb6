"""Time the per-scan surface distances at one scan of the inference pass (10 slices of 224 x 224, C = 4, the three foreground
classes reported), at unit spacing (the integer path) and at (5.0, 1.25, 1.25) (the float64 path), on two inputs -- smooth
blobs (a trained network's output) and per-pixel uniform random labels (nearly every voxel is a border voxel, the worst
case) --:

* ``functional.surface_distances_3d`` on the device (five launches, nothing read back): wall time of call + synchronise,
  device time between events and, in the first round, of each of its kernels (the library's launch timer);
* the scipy formulation of the same metric on the host in the same process, which is what medpy runs
  (contrastyou/meters/surface_distance.py:9-29 on a volume): copy both maps to the host, then per class the 3-D
  ``binary_erosion`` for the two borders, two ``distance_transform_edt(sampling=...)``, the gathers, maximum / percentile /
  means -- the baseline: no earlier version of this project computes this metric.

Every shape is warmed up first; each figure is the mean of ``--reps`` repetitions, the whole measurement is repeated
``--rounds`` times in one process so that the spread shows.  The lines are printed and written to ``--out``.

    python tools/diag/surface3d_meter_time.py [--reps 10] [--rounds 3] [--out profiles/surface3d_meter_time.txt]"""
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
D, H, W, C, REPORT = 10, 224, 224, 4, [1, 2, 3]
SPACINGS = {"unit spacing": None, "spacing (5.0, 1.25, 1.25)": (5.0, 1.25, 1.25)}


def _blobs(seed):
    from scipy import ndimage
    rng = np.random.RandomState(seed)
    fields = np.stack([ndimage.gaussian_filter(rng.randn(D, H, W), sigma=(D / 8.0, H / 8.0, W / 8.0), mode="nearest")
                       for _ in range(C)])
    return torch.from_numpy(fields.argmax(0).astype(np.int64))


def _random(seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, C, size=(D, H, W)).astype(np.int64))


def _host_reference(pred, target, spacing):
    """device -> host, then per class what medpy's hd / hd95 / asd do on a volume -> ([3, n_report] values, border voxels)"""
    from scipy import ndimage
    cross = ndimage.generate_binary_structure(3, 1)
    sampling = (1.0, 1.0, 1.0) if spacing is None else spacing
    p, t = pred.cpu().numpy(), target.cpu().numpy()
    out, borders = np.full((3, len(REPORT)), np.nan), 0
    for r, c in enumerate(REPORT):
        a, g = p == c, t == c
        if not a.any() or not g.any():
            continue
        ba, bg = a & ~ndimage.binary_erosion(a, structure=cross), g & ~ndimage.binary_erosion(g, structure=cross)
        d_ag = ndimage.distance_transform_edt(~bg, sampling=sampling)[ba]
        d_ga = ndimage.distance_transform_edt(~ba, sampling=sampling)[bg]
        out[:, r] = (max(d_ag.max(), d_ga.max()), max(np.percentile(d_ag, 95), np.percentile(d_ga, 95)),
                     (d_ag.mean() + d_ga.mean()) / 2.0)
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


def _times(name, pred, target, spacing, reps, table):
    from spcl_amd import functional as F_hip

    def hip():
        return F_hip.surface_distances_3d(pred, target, C, REPORT, spacing, 95.0)

    got = torch.stack(hip()[:3]).squeeze(1).cpu().numpy()
    ref, border = _host_reference(pred, target, spacing)
    scale = np.maximum(np.abs(ref), np.finfo(np.float64).tiny)
    worst = float(np.nanmax(np.abs(got - ref) / scale)) if np.isfinite(ref).any() else float("nan")
    t_hip, t_dev = _wall(hip, reps), _device(hip, reps)
    t_host = _wall(lambda: _host_reference(pred, target, spacing), max(1, reps // 5), 1)
    return (f"{name}: device call + synchronise {t_hip:.3f} ms (device time {t_dev:.3f} ms), host scipy per class {t_host:.1f} ms "
            f"(host / HIP = {t_host / t_hip:.1f}x; largest relative difference to the host's values {worst:.1e}; "
            f"{border} border voxels in the {len(REPORT)} pairs)"), t_hip, t_dev, _kernel_table(hip, reps) if table else []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "surface3d_meter_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("surface3d_meter_time.py measures on the GPU: no device found")
    import spcl_amd  # noqa: F401
    inputs = {"smooth blobs": (_blobs(1).to(DEV), _blobs(2).to(DEV)), "random labels": (_random(3).to(DEV), _random(4).to(DEV))}
    lines = [f"functional.surface_distances_3d on one scan of {D} x {H} x {W} class-coded voxels, C = {C}, classes {REPORT} reported; "
             f"{args.reps} reps per figure (host reference: {max(1, args.reps // 5)})"]
    for r in range(args.rounds):
        lines.append(f"round {r}")
        for sname, spacing in SPACINGS.items():
            res = {name: _times(f"{name}, {sname}", p, t, spacing, args.reps, table=r == 0) for name, (p, t) in inputs.items()}
            for v in res.values():
                lines.append("  " + v[0])
                lines.extend(f"      {us:8.1f} us  {k}" for k, us in v[3])
            lines.append(f"  random labels / smooth blobs on the HIP path, {sname}: call + synchronise "
                         f"{res['random labels'][1] / res['smooth blobs'][1]:.2f}x, device time "
                         f"{res['random labels'][2] / res['smooth blobs'][2]:.2f}x")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
