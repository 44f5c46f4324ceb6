"""Inputs and float64 references for the structured self-paced SupCon tests (test_supcon_cases_host.py checks the inputs
on the CPU, test_gpu_supcon_structured.py runs the kernels on them).  Plain helpers: no GPU code, no fixtures.

Why structured inputs.  For isotropic unit rows at t = 0.07 every positive pair has -ell_ij ~ log(2n) +- 1.3, so a fixed
age parameter leaves the self-paced weights on ONE side of their threshold.  Here the age parameter is derived from the
inputs (float64 oracle) so that about half of the positive pairs are kept and half are dropped / clipped, and -- hard mode --
so that no pair lies closer to the threshold than the kernels' own worst-case error of ell (``ell_bound``): the weights of
a correct kernel are then exactly the oracle's, and one flipped pair is an error, not noise."""
import functools
import math

import numpy as np
import torch

from oracle import spcl_oracle as O

# (n, d) -> the schedule of csrc/supcon.hip the case is meant to hit (supcon_layout / supcon_use_small / _big / _fused)
SCHEDULES = {
    (17, 40): "one-workgroup",
    (32, 128): "one-workgroup",
    (33, 100): "exact sweeps",
    (100, 128): "exact sweeps",
    (40, 300): "wide",
    (513, 128): "logits v1 + scalar row pass",
    (520, 64): "logits v1 + vector row pass",
    (520, 200): "DP = 256 + vector row pass",
    (577, 128): "fused, 126 padded rows (last 64-row tile all padding, the one before it 2 valid rows)",
    (608, 64): "fused, exactly one whole padded tile",
    (639, 100): "fused, 2 padded rows, d % 8 != 0",
    (640, 37): "fused, no padding, d % 4 != 0",
}
CASES = tuple(SCHEDULES)
TEMPERATURES = (0.07, 0.5)
# labels=None (SimCLR positives) at the large sizes, hard rule: (kind, n, d, t).  The paired clusters of (577, 128) at
# t = 0.07 are left out of the hard rule: their positives are so close that -ell ~ 0.05 for all of them and the widest gap is
# 0.6 x the bound (measured by test_supcon_cases_host.py's conditions) -- that input runs as supcon1 only.
LABEL_FREE_SHAPES = ((577, 128), (640, 37))
LABEL_FREE_HARD = tuple((kind, n, d, t) for n, d in LABEL_FREE_SHAPES for kind in ("isotropic", "paired")
                        for t in TEMPERATURES if (kind, n, d, t) != ("paired", 577, 128, 0.07))


def split_bf16(n, d, mask=False):
    """does the label path of (n, d) run the split-bf16 large-batch schedules (else exact f32)?  SUPCON_BIG_N2 = 1024"""
    return 2 * n >= 1024 and d <= 256 and not mask


@functools.lru_cache(maxsize=None)
def isotropic(n, d, seed=None):
    """two views of n unit rows, float32 -- the recipe of test_gpu_loss.py (seed n * 7 + d)"""
    g = torch.Generator().manual_seed(n * 7 + d if seed is None else seed)
    z1 = torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1)
    z2 = torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=1)
    return z1, z2


@functools.lru_cache(maxsize=None)
def clustered(n, d, nlab=None, seed=None, spread=0.6):
    """-> (z1, z2, labels): ``nlab`` unit centres (float64); row i of each view is
    normalize(float32(centre[i % nlab] + spread * randn / sqrt(d))), its label i % nlab.  Default nlab = ceil(n / 2): three
    positives per row; nlab = n: the paired (SimCLR) variant."""
    nlab = (n + 1) // 2 if nlab is None else nlab
    g = torch.Generator().manual_seed(n * 7 + d if seed is None else seed)
    centres = torch.nn.functional.normalize(torch.randn(nlab, d, generator=g, dtype=torch.float64), dim=1)
    idx = torch.arange(n) % nlab
    views = []
    for _ in range(2):
        x = centres[idx] + spread * torch.randn(n, d, generator=g, dtype=torch.float64) / math.sqrt(d)
        views.append(torch.nn.functional.normalize(x.float(), dim=1))
    return views[0], views[1], tuple(int(i) for i in idx)


def label_mask(labels):
    """the n x n label-equality matrix (float32 0 / 1), the ``mask=`` argument that states the same positives"""
    y = torch.tensor(labels)
    return (y[:, None] == y[None, :]).float()


def oracle64(z1, z2, labels=None, mask=None, *, t, gamma=None, mode="hard", correct_grad=False):
    """the oracle in float64 on the float32 inputs cast up, with its own autograd gradients
    -> dict(loss, rho, dz1, dz2, w, pos, sim_logits) of float64 numpy arrays / floats"""
    a = z1.double().clone().requires_grad_(True)
    b = z2.double().clone().requires_grad_(True)
    r = O.supcon_loss(a, b, None if labels is None else list(labels), mask, t=t, gamma=gamma, mode=mode,
                      correct_grad=correct_grad)
    r["loss"].backward()
    return {"loss": float(r["loss"].detach()), "rho": float(r["rho"]), "dz1": a.grad.numpy(), "dz2": b.grad.numpy(),
            "w": r["sp_mask"].numpy() if "sp_mask" in r else None, "pos": r["pos_mask"].numpy(),
            "sim_logits": r["sim_logits"].detach().numpy()}


def neg_ell64(z1, z2, labels=None, mask=None, *, t):
    """-ell_ij of the positive pairs (1-D float64 array, row-major order), from the float64 oracle's own tensors"""
    with torch.no_grad():
        r = O.supcon_loss(z1.double(), z2.double(), None if labels is None else list(labels), mask, t=t)
        L, E, pos, neg = r["sim_logits"], r["sim_exp"], r["pos_mask"], r["neg_mask"]
        D = (E * pos).sum(1, keepdim=True) + (E * neg).sum(1, keepdim=True)
        ll = L - torch.log(D + 1e-16)
        assert bool((pos.sum(1) > 0).all()), "a row without a positive"
        return (-ll)[pos.bool()].numpy()


def hard_gamma(l):
    """the age parameter of the hard rule: the midpoint of the widest gap between neighbouring values of ``l`` within its
    30 % .. 70 % quantile range -> (gamma, half-width of that gap)"""
    s = np.sort(np.asarray(l, dtype=np.float64))
    lo, hi = int(math.floor(0.3 * (len(s) - 1))), int(math.ceil(0.7 * (len(s) - 1)))
    gaps = np.diff(s[lo:hi + 1])
    k = int(np.argmax(gaps))
    return float(0.5 * (s[lo + k] + s[lo + k + 1])), float(0.5 * gaps[k])


def soft_gamma(l):
    """the age parameter of the soft rule: the median of ``l`` -- about half of the positives clip to w = 0"""
    return float(np.median(np.asarray(l, dtype=np.float64)))


def ell_bound(t, split_bf16):
    """worst-case error of a kernel's ell_ij = L_ij - log D_i.
    split-bf16 schedules: a row is carried as hi + mid with a residual <= 2^-18 relative and the mid * mid product is
    dropped; rows have unit norm, so a dot product is off by <= 3 * 2^-18, L_ij by that / t, and log D_i (a weighted mean
    of such errors) by the same: 6 * 2^-18 / t.  Exact-f32 schedules: the same count with the f32 unit roundoff."""
    return 6.0 * 2.0 ** (-18 if split_bf16 else -22) / t


@functools.lru_cache(maxsize=None)
def gammas(kind, n, d, t, labelled=True, use_mask=False):
    """(hard gamma, half-gap, soft gamma) of the inputs ``kind`` in ('clustered', 'paired', 'isotropic'):
    'clustered' has labels i % ceil(n / 2); 'paired' is clustered(nlab=n); 'isotropic' without labels is SimCLR"""
    z1, z2, labels = inputs(kind, n, d)
    if not labelled:
        labels = None
    mask = label_mask(labels) if use_mask else None
    l = neg_ell64(z1, z2, None if use_mask else labels, mask, t=t)
    g, half = hard_gamma(l)
    g32 = float(np.float32(g))  # the kernels take the age parameter as a float32: the oracle gets the same number
    return g32, half - abs(g32 - g), float(np.float32(soft_gamma(l)))


def inputs(kind, n, d):
    """-> (z1, z2, labels or None)"""
    if kind == "clustered":
        return clustered(n, d)
    if kind == "paired":
        return clustered(n, d, nlab=n)
    if kind == "isotropic":
        return isotropic(n, d) + (None,)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def reference(kind, n, d, t, mode, labelled=True, use_mask=False, nlab_iso=None):
    """the float64 reference of one case, computed once and shared (do not modify the arrays).
    mode: 'supcon1', 'hard' (at hard_gamma), 'soft' (at soft_gamma, correct_grad) or 'soft_12_cg'.
    ``nlab_iso``: labels i % nlab_iso for isotropic inputs.  -> (reference dict, gamma, correct_grad)"""
    z1, z2, labels = inputs(kind, n, d)
    if nlab_iso is not None:
        labels = tuple(i % nlab_iso for i in range(n))
    if not labelled:
        labels = None
    mask = label_mask(labels) if use_mask else None
    if use_mask:
        labels = None
    if mode == "supcon1":
        return oracle64(z1, z2, labels, mask, t=t), None, False
    if mode == "soft_12_cg":
        return oracle64(z1, z2, labels, mask, t=t, gamma=12.0, mode="soft", correct_grad=True), 12.0, True
    assert nlab_iso is None
    g_hard, _, g_soft = gammas(kind, n, d, t, labelled, use_mask)
    if mode == "hard":
        return oracle64(z1, z2, labels, mask, t=t, gamma=g_hard, mode="hard"), g_hard, False
    assert mode == "soft", mode
    return oracle64(z1, z2, labels, mask, t=t, gamma=g_soft, mode="soft", correct_grad=True), g_soft, True
