#!/usr/bin/env python3
"""Write tests/golden/g11_weighted_supcon.npz from the REFERENCE's contrastyou/losses/contrast_loss.py.

    python tools/gen_golden_weighted_supcon.py --reference <checkout of the reference>

The reference file is loaded by path with ``deepclustering2.writer`` stubbed (it is imported for a type annotation only).
Only data is written: the seeded inputs of tests/_weighted_supcon_oracle.make_inputs and, per case, the reference's loss,
dz1 and dz2 (float32, the reference's own precision).  Cases: (n, d) in {(3, 5), (6, 32), (33, 128)} x the six sources of
``SOURCES`` x both modes.  No test reads the reference; they read this file."""
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
from tests import _weighted_supcon_oracle as O  # noqa: E402

SHAPES = [(3, 5), (6, 32), (33, 128)]
OUT = os.path.join(REPO, "tests", "golden", "g11_weighted_supcon.npz")


def load_reference(root):
    top = sys.modules.setdefault("deepclustering2", types.ModuleType("deepclustering2"))
    writer = types.ModuleType("deepclustering2.writer")
    writer.SummaryWriter = object
    top.writer = writer
    sys.modules["deepclustering2.writer"] = writer
    path = os.path.join(root, "contrastyou", "losses", "contrast_loss.py")
    spec = importlib.util.spec_from_file_location("_reference_contrast_loss", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    ref = load_reference(args.reference)
    out, cases, worst = {}, [], 0.0
    for n, d in SHAPES:
        inp = O.make_inputs(n, d)
        for k, v in inp.items():
            out[f"n{n}_d{d}/{k}"] = v.numpy()
        for source in O.SOURCES:
            for out_mode in (True, False):
                a = inp["z1"].clone().requires_grad_(True)
                b = inp["z2"].clone().requires_grad_(True)
                _, loss = O.call_of(source, dict(inp, z1_arg=a, z2_arg=b), ref, out_mode)
                loss.backward()
                key = f"n{n}_d{d}/{source}/{'out' if out_mode else 'in'}"
                cases.append(key)
                out[key + "/loss"] = loss.detach().numpy()
                out[key + "/dz1"] = a.grad.numpy()
                out[key + "/dz2"] = b.grad.numpy()
                want, _, _ = O.loss_and_grads(inp["z1"], inp["z2"], *O.pe_of(source, inp), out_mode=out_mode)
                # (in units of the tests' bar, rtol 1e-4 / atol 1e-5: the reference itself is float32)
                worst = max(worst, abs(float(loss.detach()) - float(want)) / (1e-5 + 1e-4 * abs(float(want))))
    out["cases"] = np.array(cases)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(cases)} cases, {os.path.getsize(OUT)} bytes; restatement vs reference loss, worst difference "
          f"{worst:.2e} of the bar rtol 1e-4 / atol 1e-5")


if __name__ == "__main__":
    main()
