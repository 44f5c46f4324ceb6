#!/usr/bin/env python3
"""Write tests/golden/g12_mine.npz from the REFERENCE's semi_seg/mi_estimator/mineestimator.py.

    python tools/gen_golden_mine.py --reference <checkout of the reference>

The reference file does not import as shipped: ``contrastyou.arch.unet`` does not exist and no ``UNet`` of the reference has a
``dimension_dict``.  It is loaded by path with that module stubbed (``UNet.dimension_dict`` supplies the channel count of the
case) and with ``.base`` stubbed (``SingleEstimator`` / ``EstimatorList`` are bare ``nn.Module``s there; the real file imports
the whole segmentation package for two lists of names).  The class body -- plain torch -- is what runs.

Only data is written: per case (n, C, H, W) of tests/_mine_oracle.SHAPES the seeded feature and flip flags, the initial state
dict, and the reference's float32 loss, feature gradient (both halves), parameter gradients and running statistics after one
call.  The call is the epocher's (semi_seg/epochers/_mixins.py:79-86): ``estimator(feature[n:], flip(feature[:n]))``.  No
test reads the reference; they read this file."""
import argparse
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import _mine_oracle as O  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "g12_mine.npz")
LAYER = "Conv5"


def load_reference(root):
    class UNet:
        dimension_dict = {}

    for name in ("contrastyou", "contrastyou.arch", "contrastyou.arch.unet"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["contrastyou.arch.unet"].UNet = UNet
    pkg = types.ModuleType("_reference_mi_estimator")
    pkg.__path__ = []
    base = types.ModuleType("_reference_mi_estimator.base")

    class SingleEstimator(nn.Module):
        pass

    class EstimatorList(nn.Module):
        def __init__(self):
            super().__init__()
            self._estimator_dictionary = nn.ModuleDict()

    base.SingleEstimator, base.EstimatorList = SingleEstimator, EstimatorList
    sys.modules["_reference_mi_estimator"] = pkg
    sys.modules["_reference_mi_estimator.base"] = base
    path = os.path.join(root, "semi_seg", "mi_estimator", "mineestimator.py")
    spec = importlib.util.spec_from_file_location("_reference_mi_estimator.mineestimator", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod, UNet


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    ref, UNet = load_reference(args.reference)
    out, cases, worst = {}, [], 0.0
    for idx, (n, C, H, W) in enumerate(O.SHAPES):
        key = f"n{n}_c{C}_h{H}_w{W}"
        cases.append(key)
        feat, flags = O.make_inputs(n, C, H, W, seed=120 + idx)
        sd0 = O.init_state(C, seed=220 + idx)
        UNet.dimension_dict[LAYER] = C
        est = ref.MineEstimator(layer_name=LAYER)
        est._projector.load_state_dict(sd0, strict=True)
        est.train()
        x = feat.clone().requires_grad_(True)
        loss = est(x[n:], O.flip(x[:n], flags))
        loss.backward()
        out[key + "/feat"] = feat.numpy()
        out[key + "/flags"] = np.array(flags, dtype=np.uint8)
        for k, v in sd0.items():
            out[key + "/init/" + k] = v.numpy()
        out[key + "/loss"] = loss.detach().numpy()
        out[key + "/dfeat"] = x.grad.numpy()
        for k, p in est._projector.named_parameters():
            out[key + "/grad/" + k] = p.grad.numpy()
        for k, v in est._projector.state_dict().items():
            if "running" in k or "num_batches" in k:
                out[key + "/after/" + k] = v.numpy()
        want = O.run(feat, flags, sd0, torch.float32)
        worst = max(worst, abs(float(loss.detach()) - float(want["loss"])) / (1e-6 + 1e-4 * abs(float(want["loss"]))))
    out["cases"] = np.array(cases)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(cases)} cases, {os.path.getsize(OUT)} bytes; restatement vs reference loss, worst difference "
          f"{worst:.2e} of the bar rtol 1e-4 / atol 1e-6")


if __name__ == "__main__":
    main()
