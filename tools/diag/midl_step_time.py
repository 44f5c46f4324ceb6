"""Time the MIDL baseline's patch-wise IIC criterion at the reference's batch shape (10 x 4 x 224 x 224 class maps, padding 1)
for ``patch_size`` 32 (13 x 13 = 169 patches), 64 (6 x 6 = 36) and 1024 (the default: one patch):

* the HIP call -- ``functional.iic_patch_loss`` and its backward (two launches and one) --;
* the same arithmetic in torch ops on the same device tensors, written from the formula of
  ``IIDSegmentationSmallPathLoss`` (contrastyou/losses/iic_loss.py:103-162): per patch the crops of the two probability
  maps, the displacement joint, the min-shift, the per-displacement normalisation, the symmetrisation, the marginals and the
  loss; then the mean and autograd's backward.  Two forms of the joint: ``conv`` (one ``F.conv2d`` with the batch as the
  contraction, as the reference writes it) and ``shift`` (one ``einsum`` per displacement); a form that the device's
  convolution library refuses at a shape is reported as such;
* for ``patch_size`` 1024 also the existing dense criterion ``functional.iic_loss(dense=True)`` with one subhead on the same
  maps: the same arithmetic up to which map is read through the flips -- recorded for whoever tunes the kernels next.

Every variant starts from the same logits and ends with the gradient of the student's logits; the torch forms are handed the
already flipped copy (as the reference's epocher hands it over), the HIP calls the flags.  Device events around replayed
calls; every shape is warmed up first; each figure is the mean of its repetitions and the whole measurement is repeated
``--rounds`` times in one process so that the spread shows.  The lines are printed as they come and written to ``--out`` at
the end.

    python tools/diag/midl_step_time.py [--reps 100] [--torch-reps 3] [--rounds 3] [--out profiles/midl_step_time.txt]"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
DEV = "cuda:0"
SHAPE, PAD, PATCHES = (10, 4, 224, 224), 1, (32, 64, 1024)
FLAGS = [3, 0, 1, 2, 0, 3, 1, 2, 0, 3]


def _time(fn, reps, warmup=2):
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


def _starts(h, patch):
    return list(range(0, h - patch, patch // 2)) + [max(h - patch, 0)]


def _joint_conv(x, y, pad):
    """[T, T, k, k]: the batch is the contraction of one convolution"""
    return F.conv2d(x.transpose(0, 1), weight=y.transpose(0, 1), padding=(pad, pad)).permute(2, 3, 0, 1)


def _joint_shift(x, y, pad):
    """[T, T, k, k]: one product per displacement, X zero outside the patch"""
    h, w = x.shape[2:]
    xp = F.pad(x, (pad, pad, pad, pad))
    T = 2 * pad + 1
    return torch.stack([torch.stack([torch.einsum("nihw,njhw->ij", xp[:, :, dy:dy + h, dx:dx + w], y) for dx in range(T)])
                        for dy in range(T)])


def _criterion(j):
    """the loss of one patch from its raw joint [T, T, k, k] (lamda = 1)"""
    T = j.shape[0]
    p = j - j.min().detach() + 1e-16
    p = p / p.sum(dim=(2, 3), keepdim=True)
    p = (p + p.transpose(2, 3)) / 2.0
    pi, pj = p.sum(dim=2, keepdim=True), p.sum(dim=3, keepdim=True)
    return (-p * (torch.log(p + 1e-16) - torch.log(pi + 1e-16) - torch.log(pj + 1e-16))).sum() / (T * T)


def _torch_loss(lx, ly_tf, pad, patch, joint):
    px, py = lx.softmax(1), ly_tf.softmax(1).detach()
    H, W = px.shape[2:]
    losses = [_criterion(joint(px[:, :, a:min(a + patch, H), b:min(b + patch, W)],
                               py[:, :, a:min(a + patch, H), b:min(b + patch, W)], pad))
              for a in _starts(H, patch) for b in _starts(W, patch)]
    return sum(losses) / len(losses)


def _measure(patch, reps, torch_reps, say):
    from spcl_amd import functional as F_hip
    g = torch.Generator().manual_seed(2)

    def cl(x):
        return x.to(DEV).contiguous(memory_format=torch.channels_last)

    student, other = cl(torch.randn(*SHAPE, generator=g)), cl(torch.randn(*SHAPE, generator=g))
    flags = torch.tensor(FLAGS, dtype=torch.uint8, device=DEV)
    other_tf = F_hip.flip_batch(other, flags)
    unit = F_hip.register_unit_gradient(torch.ones((), device=DEV))
    grads = {}

    def hip():
        x = student.detach().requires_grad_(True)
        loss = F_hip.iic_patch_loss(x, other, padding=PAD, patch_size=patch, flags=flags)
        loss.backward(gradient=unit)
        grads["hip"] = x.grad
        return loss

    def dense():  # X is the map read through the flips there: the roles of the two maps are swapped, the work is the same
        y = student.detach().requires_grad_(True)
        loss = F_hip.iic_loss(other, y, num_subheads=1, num_clusters=SHAPE[1], padding=PAD, dense=True, flags=flags)
        loss.backward(gradient=unit)
        return loss

    def torch_ops(joint, name):
        def run():
            x = student.detach().requires_grad_(True)
            loss = _torch_loss(x, other_tf, PAD, patch, joint)
            loss.backward()
            grads[name] = x.grad
            return loss
        return run

    n_patches = len(_starts(SHAPE[2], patch)) * len(_starts(SHAPE[3], patch))
    t_hip = _time(hip, reps)
    line = f"patch_size {patch} ({n_patches} patches): HIP call + backward {t_hip * 1e3:.1f} us (loss {float(hip()):.6g})"
    ratios = []
    for name, joint in (("shift", _joint_shift), ("conv", _joint_conv)):
        run = torch_ops(joint, name)
        try:
            t = _time(run, torch_reps, warmup=1)
        except RuntimeError as e:  # the convolution library has no kernel for this shape
            line += f"; torch {name}: refused ({str(e).splitlines()[0][:80]})"
            continue
        err = float((grads["hip"] - grads[name]).norm() / grads[name].norm())
        ratios.append(t / t_hip)
        line += f"; torch {name} {t:.2f} ms = {t / t_hip:.0f}x (loss {float(run()):.6g}, gradients differ by {err:.1e} rel L2)"
    if patch >= max(SHAPE[2:]):
        t_dense = _time(dense, reps)
        line += f"; existing dense criterion (iic_loss, one subhead) {t_dense * 1e3:.1f} us = {t_dense / t_hip:.2f}x the HIP call"
    say(line)
    return ratios


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "midl_step_time.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("midl_step_time.py measures on the GPU: no device found")
    import spcl_amd  # noqa: F401
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"class maps {' x '.join(map(str, SHAPE))} f32 channels-last, padding {PAD}; {args.reps} reps per HIP figure, "
        f"{args.torch_reps} per torch figure")
    slowest = {}
    for r in range(args.rounds):
        say(f"round {r}")
        for patch in PATCHES:
            ratios = _measure(patch, args.reps, args.torch_reps, say)
            if ratios:
                slowest[patch] = min([slowest.get(patch, float("inf"))] + ratios)
    say("smallest torch / HIP ratio seen per patch size: " + ", ".join(f"{p}: {v:.0f}x" for p, v in slowest.items()))
    with open(args.out, "w") as out:  # (written once, at the end: a run that fails midway leaves no truncated file)
        out.write("\n".join(lines) + "\n")
    if any(v <= 1.0 for v in slowest.values()) or len(slowest) != len(PATCHES):
        raise SystemExit("the HIP call is not faster than the torch formulation at every patch size")


if __name__ == "__main__":
    main()
