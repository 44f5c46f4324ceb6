"""Integer and float64 CPU restatements of the label-guided pixel contrast (csrc/pixel_contrast.hip), for its tests: the
sampler's key and selection rule in exact integers, the criterion in float64 with autograd, and a brute-force double loop of
the criterion's definition."""
import math

import numpy as np
import torch

_M32 = 0xFFFFFFFF


def fmix32(h):
    """MurmurHash3's finaliser on uint64 arrays that hold 32-bit words"""
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(_M32)
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(_M32)
    return h ^ (h >> np.uint64(16))


def keys(n, seed):
    """key(i) = fmix32((((i + 1) * 0x9E3779B1) mod 2^32) ^ seed) for i = 0 .. n - 1, as uint64 values below 2^32"""
    i = np.arange(n, dtype=np.uint64)
    h = (((i + np.uint64(1)) & np.uint64(_M32)) * np.uint64(0x9E3779B1)) & np.uint64(_M32)
    return fmix32(h ^ np.uint64(int(seed) & _M32))


def sample(cell_label, C, K, seed):
    """-> (idx int32 [C, K], count int32 [C]): per class the min(K, n_c) cells of that label with the smallest keys, in
    ascending index order, -1 behind them"""
    lab = np.asarray(cell_label).reshape(-1)
    k = keys(lab.size, seed)
    idx = np.full((C, K), -1, dtype=np.int32)
    count = np.zeros(C, dtype=np.int32)
    for c in range(C):
        cells = np.nonzero(lab == c)[0]
        chosen = np.sort(cells[np.argsort(k[cells], kind="stable")[:K]])
        idx[c, :chosen.size] = chosen
        count[c] = chosen.size
    return idx, count


def slots(count, K):
    """(valid bool [M], cls int64 [M]) of the slots m = c K + j: valid iff j < count[c]"""
    count = [int(v) for v in count]
    C = len(count)
    cls = torch.arange(C).repeat_interleave(K)
    j = torch.arange(K).repeat(C)
    return j < torch.tensor(count)[cls], cls


def supcon(z, count, K, t):
    """the criterion in the dtype of ``z`` ([C K, d], may require grad): invalid rows are SELECTED away (they may hold NaN)"""
    valid, cls = slots(count, K)
    zz = torch.where(valid[:, None], z, torch.zeros_like(z))
    M = zz.shape[0]
    a_mask = valid[:, None] & valid[None, :] & ~torch.eye(M, dtype=torch.bool)
    p_mask = a_mask & (cls[:, None] == cls[None, :])
    npos = p_mask.sum(1)
    anchors = torch.nonzero(valid & (npos >= 1)).reshape(-1)
    if anchors.numel() == 0:
        return (zz * 0.0).sum()
    s = (zz[anchors] @ zz.t()) / t
    am, pm = a_mask[anchors], p_mask[anchors]
    lse = torch.logsumexp(torch.where(am, s, torch.full_like(s, -math.inf)), dim=1)
    pos = torch.where(pm, s, torch.zeros_like(s)).sum(1)
    li = lse - pos / npos[anchors].to(s.dtype)
    return li.mean()


def anchors(count):
    """|I|: the valid rows whose class has a second sample"""
    return sum(int(v) for v in count if int(v) >= 2)


def supcon_bruteforce(z, count, K, t):
    """the definition, term by term, in Python floats (float64)"""
    z = np.asarray(z, dtype=np.float64)
    C = len(count)
    valid = [(c, c * K + j) for c in range(C) for j in range(int(count[c]))]
    total, n = 0.0, 0
    for ci, i in valid:
        A = [(c, a) for c, a in valid if a != i]
        P = [a for c, a in A if c == ci]
        if not P:
            continue
        log_den = math.log(sum(math.exp(float(z[i] @ z[a]) / t) for _, a in A))
        total += -sum(float(z[i] @ z[p]) / t - log_den for p in P) / len(P)
        n += 1
    return total / n if n else 0.0
