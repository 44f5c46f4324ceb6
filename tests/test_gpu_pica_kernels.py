"""GPU: the PICA criteria (csrc/pica.hip; the dense one between iic.hip's joint launches) against the float64 restatement of
the reference's classes (tests/_pica_oracle.py).  Bars are those of tests/test_gpu_iic_kernels.py: loss and ce 1e-5 relative,
dJ and d(logits) 1e-5 relative L2, a second call bitwise equal.  One exception: a dense case's gradient bar is
max(1e-5, 4 x the miss of the float32 torch formulation of the ce term on the CPU against float64 at that case), computed here
from torch (never from the kernel) and printed -- at the 33 x 140 case that formulation itself misses float64 by 1.2e-5.

The dense total is ``f32(ce + lamda * ne)`` with ``ne = log M - (M / K) log K`` a large negative constant: it is checked
to 2 ulp of float32, ``ce`` (handed out separately) to 1e-5.  The dense gradient w.r.t. ``x`` is compared with float64 only:
the reference's float32 value carries the rounding noise of the balance term."""
import numpy as np
import pytest
import torch

from tests import _iic_oracle as R
from tests import _pica_oracle as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAMDA = 2.0


def _logits(N, C, H, W, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, C, H, W, generator=g) * scale).float()


def _hip(lx, ly, S, K, pad, dense, flags, scale, upstream=None):
    from spcl_amd import functional as F_hip
    x = lx.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ly.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    fl = None if flags is None else torch.tensor(flags, dtype=torch.uint8, device=DEV)
    out = []
    loss = F_hip.pica_loss(x, y, num_subheads=S, num_clusters=K, padding=pad, dense=dense, lamda=LAMDA, scale=scale, flags=fl,
                           out=out)
    (loss if upstream is None else loss * upstream).backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), out[0].cpu(), None if out[1] is None else out[1].cpu(), x.grad.cpu(), y.grad.cpu()


# ------------------------------------------------------------------------------------------ criterion from a fixed joint
JOINTS = [  # (S, K, pad, near-uniform?)
    (2, 20, 0, True), (2, 20, 1, True), (2, 20, 3, True), (2, 2, 7, False), (2, 32, 1, False),
]


@pytest.mark.parametrize("S,K,pad,uniform", JOINTS)
def test_criterion_from_fixed_f32_joint(S, K, pad, uniform):
    from spcl_amd import functional as F_hip
    T = 2 * pad + 1
    g = torch.Generator().manual_seed(11 + pad + K)
    r = torch.rand(S, T, T, K, K, generator=g)
    J = (500.0 + 20.0 * r).float() if uniform else (40.0 * r + 0.5).float()  # near-uniform: the min-shift's regime
    ne, scale = -37.25, 0.5
    loss, ce, dj = F_hip.pica_seg_loss_from_joint(J.to(DEV), lamda=LAMDA, ne=ne, scale=scale)
    torch.cuda.synchronize()
    j64 = J.double().requires_grad_(True)
    ref = sum(P.seg_ce_from_joint(j64[s]) for s in range(S)) * scale
    ref.backward()
    ref_total = float(ref.detach()) + scale * S * LAMDA * ne
    print(f"ce {float(ce):.9g} vs {float(ref.detach()):.9g}; loss {float(loss):.9g} vs {ref_total:.9g}; "
          f"dJ {P.rel_l2(dj, j64.grad):.2e}")
    assert P.rel(ce, ref.detach()) <= 1e-5, (float(ce), float(ref))
    assert P.rel(loss, ref_total) <= 1e-5, (float(loss), ref_total)
    assert P.rel_l2(dj, j64.grad) <= 1e-5, P.rel_l2(dj, j64.grad)
    # loss - ce is the constant, to the rounding of the two float32 results
    const = scale * S * LAMDA * ne
    slack = float(np.spacing(np.float32(abs(float(loss))))) + float(np.spacing(np.float32(abs(float(ce)))))
    assert abs((float(loss) - float(ce)) - const) <= slack, (float(loss) - float(ce), const, slack)
    loss2, ce2, dj2 = F_hip.pica_seg_loss_from_joint(J.to(DEV), lamda=LAMDA, ne=ne, scale=scale)
    assert torch.equal(loss, loss2) and torch.equal(ce, ce2) and torch.equal(dj, dj2)


# ------------------------------------------------------------------------------------------------------ dense end to end
DENSE = [  # (N, S, K, H, W, pad, flags)
    (2, 5, 20, 9, 11, 0, [1, 2]),
    (2, 5, 20, 9, 11, 1, [3, 0]),
    (1, 5, 20, 13, 7, 3, [2]),
    (1, 1, 10, 17, 15, 7, [1]),
    (3, 1, 10, 11, 9, 3, None),
    (2, 2, 20, 33, 140, 3, [0, 3]),  # more than one 128-column pass
    (1, 1, 2, 5, 6, 1, [3]),
]


def _ce_gradients(lx, ly, S, K, pad, flags, dtype):
    """d(sum_s ce_s) / d(logits) of the plain torch formulation in ``dtype`` on the CPU"""
    x, y = lx.detach().clone().to(dtype).requires_grad_(True), ly.detach().clone().to(dtype).requires_grad_(True)
    px, py = R.grouped_softmax(R.flip(x, flags), S, K), R.grouped_softmax(y, S, K)
    ce = sum(P.pui_seg_loss(a, b, pad, LAMDA)[1] for a, b in zip(px, py))
    return torch.autograd.grad(ce, (x, y))


@pytest.mark.parametrize("N,S,K,H,W,pad,flags", DENSE)
def test_dense_loss_and_gradients_vs_float64(N, S, K, H, W, pad, flags):
    lx, ly = _logits(N, S * K, H, W, 1), _logits(N, S * K, H, W, 2)
    weight = 0.05
    loss, ce, J, gx, gy = _hip(lx, ly, S, K, pad, True, flags, weight / S)
    x64, y64 = lx.double().requires_grad_(True), ly.double().requires_grad_(True)
    ref, ref_ce = P.pica_hook_loss(x64, y64, S, K, pad, True, flags, LAMDA)
    (ref * weight).backward()
    ref, ref_ce = float(ref.detach()) * weight, float(ref_ce.detach()) * weight
    g32, g64 = _ce_gradients(lx, ly, S, K, pad, flags, torch.float32), _ce_gradients(lx, ly, S, K, pad, flags, torch.float64)
    miss = max(P.rel_l2(a, b) for a, b in zip(g32, g64))
    bar = max(1e-5, 4.0 * miss)
    ex, ey = P.rel_l2(gx, x64.grad), P.rel_l2(gy, y64.grad)
    print(f"float32 torch ce gradient on the CPU misses float64 by {miss:.2e}: bar {bar:.2e}; kernel dx {ex:.2e}, dy {ey:.2e}; "
          f"ce {float(ce):.9g} vs {ref_ce:.9g}; loss {float(loss):.9g} vs {ref:.9g}")
    Jr = torch.stack([R.joint_dense(a, b, pad) for a, b in
                      zip(R.grouped_softmax(R.flip(lx.double(), flags), S, K), R.grouped_softmax(ly.double(), S, K))])
    assert float(((J.double() - Jr).abs() / Jr.abs().clamp_min(1e-30)).max()) <= 2e-6
    assert P.rel(ce, ref_ce) <= 1e-5, (float(ce), ref_ce)
    assert abs(float(loss) - ref) <= 2.0 * float(np.spacing(np.float32(abs(ref)))), (float(loss), ref)
    assert ex <= bar and ey <= bar, (ex, ey, bar)
    loss2, ce2, J2, gx2, gy2 = _hip(lx, ly, S, K, pad, True, flags, weight / S)
    assert torch.equal(loss, loss2) and torch.equal(ce, ce2) and torch.equal(J, J2)
    assert torch.equal(gx, gx2) and torch.equal(gy, gy2)


# ---------------------------------------------------------------------------------------------------------------- global
GLOBAL = [  # (N, S, K, upstream gradient)
    (5, 5, 20, None), (3, 1, 10, 3.0), (1, 1, 2, None), (70, 2, 32, None), (300, 1, 20, None),  # 300: more rows than one pass
]


@pytest.mark.parametrize("N,S,K,upstream", GLOBAL)
def test_global_loss_and_gradients_vs_float64(N, S, K, upstream):
    lx, ly = _logits(N, S * K, 1, 1, 3, 2.0), _logits(N, S * K, 1, 1, 4, 2.0)
    weight = 0.1
    loss, ce, J, gx, gy = _hip(lx, ly, S, K, 0, False, None, weight / S, upstream)
    assert J is None
    x64, y64 = lx.double().requires_grad_(True), ly.double().requires_grad_(True)
    ref, ref_ce = P.pica_hook_loss(x64, y64, S, K, 0, False, None, LAMDA)
    (ref * weight * (upstream or 1.0)).backward()
    ref, ref_ce = float(ref.detach()) * weight, float(ref_ce.detach()) * weight
    # A gradient that vanishes identically (one row: every cosine is 1, so d ce = 0 and y gets nothing) is rounding on both
    # sides; its error is measured against the other map's gradient, 1e-9 of it at the least.
    floor = 1e-9 * float(max(x64.grad.norm(), y64.grad.norm()))
    ex = float((gx.double() - x64.grad).norm() / x64.grad.norm().clamp_min(floor))
    ey = float((gy.double() - y64.grad).norm() / y64.grad.norm().clamp_min(floor))
    print(f"loss {float(loss):.9g} vs {ref:.9g}; ce {float(ce):.9g} vs {ref_ce:.9g}; dx {ex:.2e}, dy {ey:.2e}")
    assert P.rel(loss, ref) <= 1e-5, (float(loss), ref)
    assert P.rel(ce, ref_ce) <= 1e-5, (float(ce), ref_ce)
    assert ex <= 1e-5 and ey <= 1e-5, (ex, ey)
    loss2, ce2, _, gx2, gy2 = _hip(lx, ly, S, K, 0, False, None, weight / S, upstream)
    assert torch.equal(loss, loss2) and torch.equal(ce, ce2) and torch.equal(gx, gx2) and torch.equal(gy, gy2)
