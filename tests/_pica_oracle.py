"""CPU restatement of the PICA criteria (contrastyou/losses/pica_loss.py: PUILoss :9-38, PUISegLoss :41-84), written as the
reference writes them -- including the ``mean(0)`` of the already permuted map in PUISegLoss's balance term -- in whatever
dtype the inputs have (the tests use float64), for the tests of csrc/pica.hip.  ``flip`` and ``grouped_softmax`` are
tests/_iic_oracle.py's."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests._iic_oracle import flip, grouped_softmax

# (kind, N, K, H, W, padding, lamda) of tests/golden/g13_pica.npz, written by tools/gen_golden_pica.py
GOLDEN_CASES = [
    ("pui", 5, 20, 1, 1, 0, 2.0),
    ("pui", 3, 10, 1, 1, 0, 2.0),
    ("pui", 40, 7, 1, 1, 0, 0.5),
    ("seg", 2, 20, 9, 11, 1, 2.0),
    ("seg", 1, 10, 13, 7, 3, 2.0),
    ("seg", 2, 5, 8, 8, 0, 1.0),
]


def case_key(kind, N, K, H, W, pad, lamda):
    return f"{kind}_n{N}_k{K}_h{H}_w{W}_p{pad}"


def make_probabilities(N, K, H, W, seed):
    """two seeded f32 maps on the simplex, [N, K, H, W]"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, K, H, W, generator=g) * 2.0).softmax(1)
    y = (torch.randn(N, K, H, W, generator=g) * 2.0).softmax(1)
    return x.float(), y.float()


def pui_ce(x, y):
    """the cross-entropy part of PUILoss (pica_loss.py:31-32)"""
    pui = torch.mm(F.normalize(x.t(), p=2, dim=1), F.normalize(y, p=2, dim=0))
    return F.cross_entropy(pui, torch.arange(pui.size(0), device=pui.device))


def pui_loss(x, y, lamda=2.0):
    """PUILoss.forward (pica_loss.py:17-38) without the simplex asserts -> (loss, ce, ne)"""
    ce = pui_ce(x, y)
    p = x.mean(0).view(-1)
    ne = math.log(p.size(0)) + (p * p.log()).sum()
    return ce + lamda * ne, ce, ne


def seg_ce_from_joint(j):
    """pica_loss.py:63-73,81-84 from the raw joint [T, T, K, K] (displacements first)"""
    p = j - j.min().detach() + 1e-16
    p = p / p.sum(dim=3, keepdim=True).sum(dim=2, keepdim=True)
    p = (p + p.permute(0, 1, 3, 2)) / 2.0
    p = p.mean(dim=[0, 1])
    eye = torch.eye(p.size(0), dtype=p.dtype, device=p.device)
    return (-eye * torch.log(p + 1e-16)).mean()


def pui_seg_loss(x_out, x_tf_out, padding, lamda=2.0):
    """PUISegLoss.forward (pica_loss.py:47-79) -> (loss, ce, ne)"""
    x_out = x_out.permute(1, 0, 2, 3).contiguous()
    x_tf_out = x_tf_out.permute(1, 0, 2, 3).contiguous()
    p_i_j = F.conv2d(x_out, weight=x_tf_out, padding=(padding, padding))
    ce = seg_ce_from_joint(p_i_j.permute(2, 3, 0, 1))
    p = x_out.mean(0).view(-1)  # (over the CLASSES: the map is [K, N, H, W] here)
    ne = math.log(p.size(0)) + (p * p.log()).sum()
    return ce + lamda * ne, ce, ne


def balance_constant(M, K):
    """what ``ne`` of pui_seg_loss is on the simplex"""
    return math.log(M) - (M / K) * math.log(K)


def pica_hook_loss(lx, ly, S, K, padding, dense, flags=None, lamda=2.0):
    """mean over subheads of the criterion on softmax(flip(lx)) / softmax(ly), as the hook calls it -> (loss, ce)"""
    px = grouped_softmax(flip(lx, flags) if dense else lx, S, K)
    py = grouped_softmax(ly, S, K)
    if dense:
        terms = [pui_seg_loss(a, b, padding, lamda) for a, b in zip(px, py)]
    else:
        terms = [pui_loss(a.flatten(1), b.flatten(1), lamda) for a, b in zip(px, py)]
    return sum(t[0] for t in terms) / S, sum(t[1] for t in terms) / S


def rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def run_case(x, y, kind, padding, lamda, dtype):
    """the restated class on ``x`` / ``y`` cast to ``dtype`` -> loss, ce, gradients w.r.t. both"""
    a, b = x.detach().clone().to(dtype).requires_grad_(True), y.detach().clone().to(dtype).requires_grad_(True)
    if kind == "pui":
        loss, ce, _ = pui_loss(a.flatten(1), b.flatten(1), lamda)
    else:
        loss, ce, _ = pui_seg_loss(a, b, padding, lamda)
    ga, gb = torch.autograd.grad(loss, (a, b))
    return loss.detach(), ce.detach(), ga, gb


def load_golden(path):
    z = np.load(path)
    return [str(c) for c in z["cases"]], {k: torch.from_numpy(z[k]) for k in z.files if k != "cases"}
