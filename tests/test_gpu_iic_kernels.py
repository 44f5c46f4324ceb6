"""GPU: the IIC and consistency kernels (csrc/iic.hip) against the float64 restatement of the reference's criteria
(tests/_iic_oracle.py).  Bars (f32 accumulation): J per entry 2e-6 relative; loss 1e-5 relative; dJ, d(logits) and the
consistency gradient 1e-5 relative L2.  A second call gives bitwise the same results."""
import pytest
import torch

from tests import _iic_oracle as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _logits(N, C, H, W, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, C, H, W, generator=g) * scale).float()


def _hip(lx, ly, S, K, pad, dense, flags, scale=1.0):
    from spcl_amd import functional as F_hip
    x = lx.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ly.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    fl = None if flags is None else torch.tensor(flags, dtype=torch.uint8, device=DEV)
    out = []
    loss = F_hip.iic_loss(x, y, num_subheads=S, num_clusters=K, padding=pad, dense=dense, scale=scale, flags=fl, out=out)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), out[0].cpu(), out[1].cpu(), x.grad.cpu(), y.grad.cpu()


# The logits' gradient carries the pointwise mutual information of J, a small difference of logarithms of nearly equal
# numbers; f32 softmax probabilities (1e-7 relative) bound how well it is known.  With one 17 x 15 image and 225
# displacements the bar is looser (the measured gradient error there is 1.2e-4 relative L2; the test prints
# max J / (J - min J) of its input).
CASES = [  # (N, S, K, H, W, pad, flags, gradient bar)
    (2, 5, 20, 9, 11, 0, [1, 2], 1e-5),
    (2, 5, 20, 9, 11, 1, [3, 0], 1e-5),
    (1, 5, 20, 13, 7, 3, [2], 1e-5),
    (1, 1, 10, 17, 15, 7, [1], 5e-4),
    (3, 1, 10, 11, 9, 3, None, 1e-5),
    (2, 5, 20, 33, 140, 3, [0, 3], 1e-5),  # more than one 128-column pass
]


@pytest.mark.parametrize("N,S,K,H,W,pad,flags,bar", CASES)
def test_dense_joint_loss_and_gradients_vs_float64(N, S, K, H, W, pad, flags, bar):
    lx, ly = _logits(N, S * K, H, W, 1), _logits(N, S * K, H, W, 2)
    scale = 0.05 / S
    loss, J, flag, gx, gy = _hip(lx, ly, S, K, pad, True, flags, scale)
    x64, y64 = lx.double().requires_grad_(True), ly.double().requires_grad_(True)
    px = R.grouped_softmax(R.flip(x64, flags), S, K)
    py = R.grouped_softmax(y64, S, K)
    Jr = torch.stack([R.joint_dense(a, b, pad) for a, b in zip(px, py)]).detach()
    err = ((J.double() - Jr).abs() / Jr.abs().clamp_min(1e-30)).max()
    assert float(err) <= 2e-6, float(err)
    ref = sum(R.iid_segmentation_loss(a, b, pad) for a, b in zip(px, py)) * scale
    ref.backward()
    assert abs(float(loss) - float(ref.detach())) <= 1e-5 * abs(float(ref)), (float(loss), float(ref))
    assert int(flag[0]) == 0
    d = Jr - Jr.amin(dim=(1, 2, 3, 4), keepdim=True)
    d[d == 0] = float("inf")
    print(f"max J / (J - min J) over the entries above the min: {float((Jr / d).amax()):.3g}")
    assert _rel_l2(gx, x64.grad) <= bar, _rel_l2(gx, x64.grad)
    assert _rel_l2(gy, y64.grad) <= bar, _rel_l2(gy, y64.grad)
    # bitwise deterministic
    loss2, J2, _, gx2, gy2 = _hip(lx, ly, S, K, pad, True, flags, scale)
    assert torch.equal(loss, loss2) and torch.equal(J, J2) and torch.equal(gx, gx2) and torch.equal(gy, gy2)


def test_global_iid_loss_vs_float64():
    N, S, K = 5, 5, 20
    lx, ly = _logits(N, S * K, 1, 1, 3, 2.0), _logits(N, S * K, 1, 1, 4, 2.0)
    loss, J, _, gx, gy = _hip(lx, ly, S, K, 0, False, None, 0.1 / S)
    x64, y64 = lx.double().requires_grad_(True), ly.double().requires_grad_(True)
    ref = R.iic_hook_loss(x64, y64, S, K, 0, False) * 0.1
    ref.backward()
    assert abs(float(loss) - float(ref.detach())) <= 1e-5 * abs(float(ref)), (float(loss), float(ref))
    assert _rel_l2(gx, x64.grad) <= 1e-5 and _rel_l2(gy, y64.grad) <= 1e-5, (_rel_l2(gx, x64.grad), _rel_l2(gy, y64.grad))


@pytest.mark.parametrize("pad", [0, 1, 3])
def test_loss_from_fixed_f32_joint(pad):
    from spcl_amd import functional as F_hip
    T, S, K = 2 * pad + 1, 2, 20
    g = torch.Generator().manual_seed(7 + pad)
    J = (500.0 + 20.0 * torch.rand(S, T, T, K, K, generator=g)).float()  # near-uniform: the min-shift's regime
    loss, dj, flag = F_hip.iic_loss_from_joint(J.to(DEV), dense=True, scale=1.0)
    torch.cuda.synchronize()
    j64 = J.double().requires_grad_(True)
    ref = sum(R.dense_loss_from_joint(j64[s]) for s in range(S))
    ref.backward()
    assert abs(float(loss) - float(ref.detach())) <= 1e-5 * abs(float(ref)), (float(loss), float(ref))
    assert _rel_l2(dj.cpu(), j64.grad) <= 1e-5, _rel_l2(dj.cpu(), j64.grad)
    assert int(flag.cpu()[0]) == 0
    bad = J.clone()
    bad[0, 0, 0, 0, 0] = float("nan")
    _, _, flag = F_hip.iic_loss_from_joint(bad.to(DEV), dense=True)
    assert int(flag.cpu()[0]) == 1


@pytest.mark.parametrize("flags", [None, [0, 1, 2, 3]])
def test_consistency_vs_float64(flags):
    from spcl_amd import functional as F_hip
    N, C, H, W = 4, 4, 19, 23
    a, b = _logits(N, C, H, W, 5), _logits(N, C, H, W, 6)
    fl = None if flags is None else torch.tensor(flags, dtype=torch.uint8, device=DEV)
    ad = a.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    bd = b.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    loss = F_hip.consistency_softmax_mse(ad, bd, 1.0, fl)
    (loss * 3.0).backward()
    torch.cuda.synchronize()
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = R.consistency(a64, b64, 1.0, flags)
    (ref * 3.0).backward()
    assert abs(float(loss) - float(ref.detach())) <= 1e-5 * abs(float(ref))
    assert ad.grad is None or float(ad.grad.abs().max()) == 0.0
    assert _rel_l2(bd.grad.cpu(), b64.grad) <= 1e-5, _rel_l2(bd.grad.cpu(), b64.grad)
    loss2 = F_hip.consistency_softmax_mse(ad.detach(), bd.detach(), 1.0, fl)
    assert torch.equal(loss.detach().cpu(), loss2.cpu())
