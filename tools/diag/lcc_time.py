"""Time the largest-connected-component step at one scan of the inference pass (10 slices of 224 x 224, C = 4, the three
foreground classes processed, 6-neighbour) on three inputs -- smooth blobs with sprinkled islands (a trained network's output),
per-voxel uniform random labels (hundreds of thousands of components of a few voxels) and the serpentine (one-voxel-wide
snakes through every row of every slice: the longest union chains) --:

* ``functional.largest_components`` on the device (five launches, nothing read back): wall time of call + synchronise, device
  time between events over many calls and, in the first round, of each of its kernels (the library's launch timer);
* the host formulation a user would otherwise write, in the same process: copy the map to the host, ``scipy.ndimage.label``
  per class, ``bincount``, rebuild the map, copy it back (tests/_lcc_oracle.py between the two copies).

Every input is warmed up first and the device result is compared with the host's (it must be equal); each figure is the mean of
``--reps`` repetitions, the whole measurement is repeated ``--rounds`` times in one process so that the spread shows.  The lines
are printed and written to ``--out``.

    python tools/diag/lcc_time.py [--reps 50] [--rounds 3] [--out profiles/lcc_time.txt]"""
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
D, H, W, C = 10, 224, 224, 4


def _inputs():
    from tests import _lcc_oracle as O
    snake = np.concatenate([O.serpentine(H, W) for _ in range(D)], axis=1)  # (the slices join along z at every voxel)
    return {"smooth blobs": O.smooth_blobs((1, D, H, W), C, seed=11), "random labels": O.random_labels((1, D, H, W), C, seed=3),
            "serpentine": snake}


def _host(t):
    """device -> host, label / bincount / rebuild per class, host -> device"""
    from tests import _lcc_oracle as O
    out, kept, ncomp = O.largest_components(t.cpu().numpy(), C)
    return torch.from_numpy(out).to(t.device), kept, ncomp


def _wall(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def _device(fn, reps, warmup=3):
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


def _times(name, t, reps, table):
    from spcl_amd import functional as F_hip
    extras = []
    got = F_hip.largest_components(t, C, out=extras)
    want, kept, ncomp = _host(t)
    equal = (torch.equal(got, want) and np.array_equal(extras[0].cpu().numpy(), kept)
             and np.array_equal(extras[1].cpu().numpy(), ncomp))

    def hip():
        return F_hip.largest_components(t, C)

    t_hip, t_dev = _wall(hip, reps), _device(hip, reps)
    t_host = _wall(lambda: _host(t), max(2, reps // 10), 1)
    line = (f"{name}: device call + synchronise {t_hip * 1e3:.1f} us (device time {t_dev * 1e3:.1f} us), host scipy per class "
            f"{t_host:.2f} ms (host / HIP = {t_host / t_hip:.1f}x); equal to the host's result: {equal}; components per class "
            f"{ncomp[0].tolist()}, kept {kept[0].tolist()}")
    return line, _kernel_table(hip, reps) if table else []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lcc_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lcc_time.py measures on the GPU: no device found")
    import spcl_amd  # noqa: F401
    inputs = {k: torch.from_numpy(v).to(DEV) for k, v in _inputs().items()}
    lines = [f"functional.largest_components on one scan of {D} x {H} x {W} class-coded voxels, C = {C}, classes "
             f"{list(range(1, C))} processed, 6-neighbour; {args.reps} reps per figure (host formulation: {max(2, args.reps // 10)})"]
    for r in range(args.rounds):
        lines.append(f"round {r}")
        for name, t in inputs.items():
            line, table = _times(name, t, args.reps, table=r == 0)
            lines.append("  " + line)
            lines.extend(f"      {us:8.1f} us  {k}" for k, us in table)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
