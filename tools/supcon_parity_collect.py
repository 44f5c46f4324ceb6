"""Measure the table of docs/supcon_parity.md: for every case of tests/_supcon_cases.py (one per schedule of csrc/supcon.hip),
each temperature and both self-paced rules, the largest gradient error of the HIP kernels against the oracle in float64,
divided by max|grad| -- and beside it the same figure for the oracle in float32 (torch on the CPU), i.e. what float32
arithmetic in another summation order costs on the same inputs.  Prints the markdown table.

    python tools/supcon_parity_collect.py [--out FILE]        (needs the GPU)"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

from oracle import spcl_oracle as O  # noqa: E402
from tests import _supcon_cases as C  # noqa: E402


def kernel_grads(z1, z2, labels, t, mode, gamma):
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses.contrast_loss3 import SelfPacedSupConLoss
    crit = SelfPacedSupConLoss(temperature=t, weight_update=mode, correct_grad=mode == "soft")
    crit.set_gamma(gamma)
    x, y = z1.cuda().requires_grad_(True), z2.cuda().requires_grad_(True)
    crit(x, y, target=list(labels)).backward()
    return np.concatenate([x.grad.cpu().numpy(), y.grad.cpu().numpy()])


def oracle32_grads(z1, z2, labels, t, mode, gamma):
    a, b = z1.clone().requires_grad_(True), z2.clone().requires_grad_(True)
    O.supcon_loss(a, b, list(labels), t=t, gamma=gamma, mode=mode, correct_grad=mode == "soft")["loss"].backward()
    return np.concatenate([a.grad.numpy(), b.grad.numpy()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = ["| (n, d) | schedule | t | rule | kernel err / max\\|grad\\| | float32 oracle err / max\\|grad\\| | ratio |",
            "|---|---|---|---|---|---|---|"]
    for (n, d), name in C.SCHEDULES.items():
        z1, z2, labels = C.clustered(n, d)
        for t in C.TEMPERATURES:
            for mode in ("hard", "soft"):
                ref, gamma, _ = C.reference("clustered", n, d, t, mode)
                g64 = np.concatenate([ref["dz1"], ref["dz2"]])
                scale = np.abs(g64).max()
                ek = np.abs(kernel_grads(z1, z2, labels, t, mode, gamma) - g64).max() / scale
                e32 = np.abs(oracle32_grads(z1, z2, labels, t, mode, gamma) - g64).max() / scale
                rows.append(f"| ({n}, {d}) | {name.split(' (')[0]} | {t} | {mode} | {ek:.1e} | {e32:.1e} | {ek / e32:.1f} |")
                print(rows[-1], flush=True)
    text = "\n".join(rows) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
