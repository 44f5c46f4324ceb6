#!/usr/bin/env python3
"""Write tests/golden/g13_pica.npz from the REFERENCE's contrastyou/losses/pica_loss.py.

    python tools/gen_golden_pica.py --reference <checkout of the reference>

The reference file imports ``simplex`` from ``deepclustering2.utils`` (un-vendored third party).  It is loaded by path with
that module stubbed by the two-line check the name stands for; the class bodies -- plain torch -- are what runs.

Only data is written: per case of tests/_pica_oracle.GOLDEN_CASES the seeded probabilities ``x`` / ``y``, the reference's
float32 loss and gradients w.r.t. both, and the reference's OWN float32-against-float64 relative gap (the same class run on the
inputs cast to float64) of the loss and of the gradient w.r.t. ``y`` -- the yardstick tests/test_gpu_pica_hooks.py derives its
bars from.  (The gradient w.r.t. ``x`` of the dense criterion is not given a gap: in float32 the balance term adds rounding
noise to it.)  No test reads the reference; they read this file."""
import argparse
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import _pica_oracle as O  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "g13_pica.npz")


def load_reference(root):
    def simplex(t, axis=1):
        s = t.sum(axis)
        return bool(torch.allclose(s, torch.ones_like(s)))

    top = sys.modules.setdefault("deepclustering2", types.ModuleType("deepclustering2"))
    utils = types.ModuleType("deepclustering2.utils")
    utils.simplex = simplex
    top.utils = utils
    sys.modules["deepclustering2.utils"] = utils
    path = os.path.join(root, "contrastyou", "losses", "pica_loss.py")
    spec = importlib.util.spec_from_file_location("_reference_pica_loss", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def run(ref, kind, x, y, pad, lamda, dtype):
    crit = ref.PUILoss(lamda=lamda) if kind == "pui" else ref.PUISegLoss(lamda=lamda, padding=pad)
    a, b = x.detach().clone().to(dtype).requires_grad_(True), y.detach().clone().to(dtype).requires_grad_(True)
    loss = crit(a.flatten(1), b.flatten(1)) if kind == "pui" else crit(a, b)
    ga, gb = torch.autograd.grad(loss, (a, b))
    return loss.detach(), ga, gb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    ref = load_reference(args.reference)
    out, cases = {}, []
    for idx, case in enumerate(O.GOLDEN_CASES):
        kind, N, K, H, W, pad, lamda = case
        key = O.case_key(*case)
        cases.append(key)
        x, y = O.make_probabilities(N, K, H, W, seed=130 + idx)
        l32, gx32, gy32 = run(ref, kind, x, y, pad, lamda, torch.float32)
        l64, gx64, gy64 = run(ref, kind, x, y, pad, lamda, torch.float64)
        out[key + "/x"], out[key + "/y"] = x.numpy(), y.numpy()
        out[key + "/loss"] = l32.numpy()
        out[key + "/gx"], out[key + "/gy"] = gx32.numpy(), gy32.numpy()
        out[key + "/gap_loss"] = np.float64(O.rel(l32, l64))
        out[key + "/gap_gy"] = np.float64(O.rel_l2(gy32, gy64))
        want = O.run_case(x, y, kind, pad, lamda, torch.float64)
        print(f"{key}: loss {float(l32):.9g}, reference f32 vs f64: loss {O.rel(l32, l64):.2e}, gy {O.rel_l2(gy32, gy64):.2e}, "
              f"gx {O.rel_l2(gx32, gx64):.2e}; restatement vs reference in f64: loss {O.rel(want[0], l64):.2e}, "
              f"gy {O.rel_l2(want[3], gy64):.2e}")
    out["cases"] = np.array(cases)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(cases)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
