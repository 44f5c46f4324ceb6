"""Measure the tables of docs/eval_parity.md: the eval-mode UNet on the HIP path against the oracle in float64, on the cases of
tests/_eval_oracle.py (weights whose running statistics are real).

  float32   per shape, f32 product mode and stage: max|device - f64| / max|f64|, beside the same figure for the oracle run in
            float32 on the CPU (what float32 arithmetic in another summation order costs on these numbers), and their ratio
  bf16      per shape and stage, every stage fed the DEVICE's outputs of the stages before it: relative L2 against the
            bf16-emulating oracle in float64 arithmetic, beside the same emulation in float32 arithmetic on the same inputs
  gradients per shape and module: the eval-mode parameter gradients of the fine-tune loss (float32, default product mode)

Prints the markdown tables.  No assertion is derived from them.

    python tools/eval_parity_collect.py [--out FILE]        (needs the GPU)"""
import argparse
import os
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

from oracle import spcl_oracle as O  # noqa: E402
from tests import _eval_oracle as E  # noqa: E402

F32_SHAPES = [(3, 48, 32, 128), (2, 64, 64, 256), (1, 112, 80, 128), (2, 16, 16, 128), (2, 224, 224, 256)]
BF16_SHAPES = [(3, 48, 32, 128), (2, 64, 64, 256), (2, 224, 224, 256)]
GRAD_SHAPES = [(3, 48, 32, 128), (2, 64, 64, 256)]


def device_stages(model, x):
    outs = {}
    with torch.no_grad():
        for s in E.STAGES:
            outs[s] = model(x, until=E.until_of(s)).detach().double().cpu()
    return outs


def float32_table(rows):
    import spcl_amd  # noqa: F401
    from spcl_amd import native
    rows += ["| (N, H, W, max_channel) | f32 products | stage | device err / max | float32 oracle err / max | ratio |",
             "|---|---|---|---|---|---|"]
    for shape in F32_SHAPES:
        c = E.case(*shape)
        model = E.load_unet(c["sd"], shape[3], torch.float32)
        for mode in ("exact", "split"):
            native.call("spcl_conv_set_f32_split", 1 if mode == "split" else 0)
            try:
                dev = device_stages(model, c["x"].float().cuda())
            finally:
                native.call("spcl_conv_set_f32_split", 1)
            for s in E.STAGES:
                e, b = E.relmax(dev[s], c["f64"][s]), c["f32_err"][s]
                rows.append(f"| {shape} | {mode} | {s} | {e:.1e} | {b:.1e} | {e / b:.1f} |")
                print(rows[-1], flush=True)


def bf16_table(rows):
    rows += ["", "| (N, H, W, max_channel) | stage | device rel. L2 | float32-arithmetic emulation rel. L2 | ratio |",
             "|---|---|---|---|---|"]
    for shape in BF16_SHAPES:
        c = E.case(*shape)
        model = E.load_unet(c["sd"], shape[3], torch.bfloat16)
        dev = device_stages(model, c["x"].float().cuda())
        sd32 = E.as_dtype(c["sd"], torch.float32)
        for s in E.STAGES:
            inputs = E.stage_inputs(s, c["x"], dev)
            with torch.no_grad():
                ref = E.stage_oracle(s, inputs, c["sd"], q=O.BF16Emulation)
                emu = E.stage_oracle(s, tuple(t.float() for t in inputs), sd32, q=O.BF16Emulation)
            e, b = E.rel_l2(dev[s], ref), E.rel_l2(emu, ref)
            rows.append(f"| {shape} | {s} | {e:.1e} | {b:.1e} | {e / b:.1f} |" if b > 0 else
                        f"| {shape} | {s} | {e:.1e} | {b:.1e} | - |")
            print(rows[-1], flush=True)
        whole = E.rel_l2(dev["Deconv_1x1"], E.chain(c["x"], c["sd"], q=O.BF16Emulation)["Deconv_1x1"])
        rows.append(f"| {shape} | logits from x (no teacher forcing) | {whole:.1e} | | |")
        print(rows[-1], flush=True)


def gradient_table(rows):
    from spcl_amd import functional as F
    rows += ["", "| (N, H, W, max_channel) | module | tensors | worst device err / max | its float32 oracle err / max | worst ratio |",
             "|---|---|---|---|---|---|"]
    for shape in GRAD_SHAPES:
        gc = E.grad_case(*shape)
        model = E.load_unet(gc["case"]["sd"], shape[3], torch.float32)
        loss = F.kl_div(F.softmax_classes(model(gc["case"]["x"].float().cuda())), F.one_hot_classes(gc["labels"].cuda(), 4))
        loss.backward()
        by_module = {}
        for k, p in model.named_parameters():
            by_module.setdefault(k.split(".")[0], []).append((E.relmax(p.grad, gc["grads"][k]), gc["f32_err"][k], k))
        for m, items in by_module.items():
            e, b, k = max(items)
            ratio = max(x[0] / x[1] for x in items)
            rows.append(f"| {shape} | {m} | {len(items)} | {e:.1e} ({k.split('.', 1)[1]}) | {b:.1e} | {ratio:.1f} |")
            print(rows[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = []
    float32_table(rows)
    bf16_table(rows)
    gradient_table(rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(rows) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
