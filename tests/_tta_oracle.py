"""Float64 restatement of the test-time-augmentation pieces (``functional.tta_views`` / ``functional.tta_merge`` /
``spcl_tta_merge``) with ``torch.flip`` and ``transpose`` on the CPU, and the seeded inputs the GPU kernel tests use.

The op byte of a view: bit 0 its input was flipped along H, bit 1 along W, bit 2 its H and W axes were swapped AFTER the flips.
A map the network returned for a view lies in that view's frame; ``unview`` carries it back: swap first, then the flips (each
its own inverse)."""
import math

import torch

MODES = {"flips": (0, 1, 2, 3), "dihedral": (0, 1, 2, 3, 4, 5, 6, 7)}


def view(x, op):
    """x [..., H, W] -> view ``op`` of it"""
    if op & 1:
        x = torch.flip(x, dims=(-2,))
    if op & 2:
        x = torch.flip(x, dims=(-1,))
    if op & 4:
        x = x.transpose(-1, -2)
    return x.contiguous()


def unview(x, op):
    """a map in the frame of view ``op`` -> the original frame (the inverse of ``view``)"""
    if op & 4:
        x = x.transpose(-1, -2)
    if op & 2:
        x = torch.flip(x, dims=(-1,))
    if op & 1:
        x = torch.flip(x, dims=(-2,))
    return x.contiguous()


def views(image, mode):
    ops = MODES[mode]
    if any(op & 4 for op in ops) and image.shape[-1] != image.shape[-2]:
        raise ValueError(f"{mode} needs a square image, given {tuple(image.shape[-2:])}")
    return [(view(image, op), op) for op in ops]


def merge(view_logits, ops, eps=1e-16):
    """[N, C, H, W] logits per view (each in its view's frame) -> (prob [N,C,H,W], pred [N,H,W], entropy [N,H,W],
    mean_entropy, gap): float64 throughout; ``pred`` the first maximal class; ``gap`` the smallest difference between the top
    two mean probabilities over all pixels"""
    assert len(view_logits) == len(ops)
    rows = [torch.softmax(unview(t.detach().cpu().double(), op), dim=1) for t, op in zip(view_logits, ops)]
    prob = torch.stack(rows).sum(0) / len(rows)
    C = prob.shape[1]
    pred = torch.from_numpy(prob.numpy().argmax(axis=1))  # (numpy: the first maximum)
    entropy = -(prob * torch.log(prob + eps)).sum(1) / math.log(C)
    top = prob.topk(2, dim=1).values
    gap = float((top[:, 0] - top[:, 1]).min())
    return prob, pred, entropy, float(entropy.mean()), gap


# ---- the inputs of tests/test_gpu_tta_kernels.py; tests/test_tta_host.py asserts their top-two gap on the CPU
SHAPES = ((2, 4, 6, 10), (3, 4, 9, 11), (1, 16, 5, 7), (2, 2, 7, 3), (2, 4, 8, 8), (2, 5, 12, 12))  # (N, C, H, W)
SQUARE = tuple(s for s in SHAPES if s[2] == s[3])
GAP = 1e-4


# seeds picked on the CPU (float64 oracle) so that the smallest top-two gap of every case is >= 1e-3, ten times the asserted bar
_FLIPS_SEEDS = (1100, 9101, 1102, 103, 104, 9105)
_DIHEDRAL_SEEDS = (200, 6201)


def _cases():
    out = [(f"flips-{'x'.join(map(str, s))}", s, MODES["flips"], seed) for s, seed in zip(SHAPES, _FLIPS_SEEDS)]
    out += [(f"dihedral-{'x'.join(map(str, s))}", s, MODES["dihedral"], seed) for s, seed in zip(SQUARE, _DIHEDRAL_SEEDS)]
    out += [("one-view", SHAPES[1], (0,), 300), ("two-views-0-2", SHAPES[0], (0, 2), 1301),
            ("two-views-swap", SHAPES[5], (5, 6), 5302), ("offset-4-bytes", SHAPES[0], MODES["flips"], 303)]
    return out


CASES = _cases()  # (name, shape, ops, seed)


def case_logits(case):
    """independent ``3 * randn`` logits for every view of the case, f32 [N, C, H, W] on the CPU"""
    _, shape, ops, seed = case
    g = torch.Generator().manual_seed(seed)
    return [3 * torch.randn(shape, generator=g) for _ in ops]
