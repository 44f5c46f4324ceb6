"""Time the dense IIC criterion (csrc/iic.hip: joint, loss, backward) at the UDA-IIC reference sizes (5 unlabelled
images, 5 subheads x 20 clusters; Up_conv3 112^2, Up_conv2 224^2) for paddings 0, 1, 3, against the same math in torch ops
on the device (F.conv2d joint of the reference's IIDSegmentationLoss, f32).

    python tools/diag/iic_kernel_time.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def _time(fn, reps=10):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    from tests import _iic_oracle as R
    dev = "cuda:0"
    n, S, K = 5, 5, 20
    flags = torch.tensor([1, 0, 3, 2, 1], dtype=torch.uint8, device=dev)
    for name, hw in (("Up_conv3", 112), ("Up_conv2", 224)):
        lx = torch.randn(n, S * K, hw, hw, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        ly = torch.randn(n, S * K, hw, hw, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        for pad in (0, 1, 3):
            def hip():
                loss = F_hip.iic_loss(lx, ly, num_subheads=S, num_clusters=K, padding=pad, dense=True, scale=1.0 / S,
                                      flags=flags)
                loss.backward()

            def torch_ops():
                px = R.grouped_softmax(R.flip(lx, flags.tolist()), S, K)
                py = R.grouped_softmax(ly, S, K)
                loss = sum(R.iid_segmentation_loss(a, b, pad) for a, b in zip(px, py)) / S
                loss.backward()

            th = _time(hip)
            # the torch formulation's F.conv2d with an image-sized kernel runs for minutes beyond these two cases
            tt = _time(torch_ops, reps=3) if (hw == 112 or pad == 0) else float("nan")
            gf = 3 * 2.0 * (2 * pad + 1) ** 2 * n * hw * hw * S * K * K / 1e9
            print(f"{name} p={pad}: HIP fwd+loss+bwd {th:.3f} ms ({gf / th:.1f} TFLOP/s useful), torch ops {tt:.3f} ms")


if __name__ == "__main__":
    main()
