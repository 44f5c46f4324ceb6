"""Integer and float64 CPU restatements of CutMix for cross pseudo supervision (csrc/cutmix.hip), for its tests: the box rule
in Python integers, the ``src`` index maps of a mix, and the mixed criterion through torch autograd with the teachers gathered
by ``src``.  All maps are logical [N, C, H, W]."""
import torch

from tests import _cps_oracle as CO

M32 = 0xFFFFFFFF


def key(i, seed):
    """``pxs_key`` of csrc/pixel_contrast.hip: fmix32(((i + 1) * 0x9E3779B1 mod 2^32) ^ seed)"""
    h = (((i + 1) * 0x9E3779B1) & M32) ^ (seed & M32)
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def share16(p):
    """an area share in units of 1 / 65536, as the binding forms it"""
    return int(round(float(p) * 65536))


def box(n, seed, H, W, lo16, hi16):
    """box ``n`` of a batch: (y0, x0, bh, bw), rows [y0, y0 + bh), columns [x0, x0 + bw)"""
    r = [key(4 * n + j, seed) for j in range(4)]
    u = [v >> 8 for v in r]
    P = lo16 + (((hi16 - lo16) * u[0]) >> 24)
    S = P + (((65536 - P) * u[1]) >> 24)
    T = (P * 65536) // S
    sh, sw = (S, T) if r[1] & 1 else (T, S)
    bh = min(H, max(1, (H * sh + 32768) >> 16))
    bw = min(W, max(1, (W * sw + 32768) >> 16))
    y0 = ((H - bh + 1) * u[2]) >> 24
    x0 = ((W - bw + 1) * u[3]) >> 24
    return y0, x0, bh, bw


def boxes(seed, N, H, W, prop_range=(0.25, 0.5)):
    """int32 [N, 4]"""
    lo16, hi16 = share16(prop_range[0]), share16(prop_range[1])
    assert 1 <= lo16 <= hi16 <= 65536
    return torch.tensor([box(n, seed, H, W, lo16, hi16) for n in range(N)], dtype=torch.int32).reshape(N, 4)


def inside(bx, H, W):
    """bool [N, H, W]: the pixels inside their sample's box"""
    bx = bx.long().cpu()
    ys, xs = torch.arange(H).view(1, H, 1), torch.arange(W).view(1, 1, W)
    y0, x0, bh, bw = (bx[:, k].view(-1, 1, 1) for k in range(4))
    return (ys >= y0) & (ys < y0 + bh) & (xs >= x0) & (xs < x0 + bw)


def src(bx, N, H, W, roll=1):
    """int64 [N, H, W]: the sample a pixel is read from -- (n + roll) mod N inside box n, n elsewhere; no boxes: n"""
    own = torch.arange(N).view(N, 1, 1).expand(N, H, W)
    if bx is None:
        return own.clone()
    return torch.where(inside(bx, H, W), (own + roll) % N, own)


def gather(t, m):
    """``t[m[n, h, w], :, h, w]`` of a logical [N, C, H, W] map"""
    N, C, H, W = t.shape
    idx = m.view(N, 1, H, W).expand(N, C, H, W)
    return torch.gather(t, 0, idx)


def mix_images(x, bx, roll=1):
    """the image mix through ``torch.where``"""
    N, _, H, W = x.shape
    return torch.where(inside(bx, H, W).view(N, 1, H, W).to(x.device), x.roll(-roll, 0), x)


def teachers(t_a, t_b, bx, roll=1):
    """(confA, yA, confB, yB) of the teachers gathered through the boxes: float64 confidences and arg-max labels [N, H, W]"""
    N, _, H, W = t_a.shape
    m = src(bx, N, H, W, roll)
    confA, yA = CO.conf_and_label(gather(t_a, m))
    confB, yB = CO.conf_and_label(gather(t_b, m))
    return confA, yA, confB, yB


def parts(sa64, sb64, yA, yB, keepA, keepB, weight=1.0):
    """the two directions of the mixed criterion: the students' cross-entropies towards the gathered teachers' labels"""
    return CO.parts(sa64, sb64, yA, yB, keepA, keepB, weight)


def loss(sa64, sb64, yA, yB, keepA, keepB, weight=1.0):
    return CO.loss(sa64, sb64, yA, yB, keepA, keepB, weight)


def hist(yA, yB, keepA, keepB, C, bx=None):
    """int64 [4 C + 2]: ``_cps_oracle.hist`` and the number of pixels inside a box"""
    N, H, W = yA.shape
    n_in = int(inside(bx, H, W).sum()) if bx is not None else 0
    return torch.cat([CO.hist(yA, yB, keepA, keepB, C), torch.tensor([n_in])])
