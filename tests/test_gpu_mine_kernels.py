"""GPU: the kernels of csrc/mine.hip, one by one.

Pairs: ``mine_pairs`` forward and backward are ``torch.equal`` to ``torch.cat`` / ``torch.roll`` / ``flip_batch`` and their
autograd (a copy forward; backward one f32 addition rounded once, which is also what torch's bf16 addition is), for n in 1..3,
C in 8 (padded feature storage, element-wise path), 12 (padded output too), 16 and 32 (16-byte path), 5 x 7 and 14 x 14 maps,
every flag value, f32 and bf16.
Head: on a given stored activation the pooled maxima and their argmax are exactly those of CPU
``F.adaptive_max_pool2d(return_indices=True)`` -- with a constant map, two equal maxima and an all-zero channel (what an
all-non-positive channel is after the ReLU) --, the loss is the float64 value within ``bound`` (floor 1e-6: the head alone),
``dw`` / ``db`` likewise, the activation gradients are exactly zero off the argmax.  Two identical calls give the same bits."""
import pytest
import torch
import torch.nn.functional as F

from tests import _mine_oracle as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("size", [(5, 7), (14, 14)], ids=["5x7", "14x14"])
@pytest.mark.parametrize("C", [8, 12, 16, 32])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_pairs_equal_cat_roll_flip_and_their_autograd(n, C, size, dtype):
    from spcl_amd import functional as F_hip
    H, W = size
    g = torch.Generator().manual_seed(1000 * n + 10 * C + H)
    feat = torch.randn(2 * n, C, H, W, generator=g).to(dtype).to(DEV)
    gj = torch.randn(n, 2 * C, H, W, generator=g).to(dtype).to(DEV)
    gm = torch.randn(n, 2 * C, H, W, generator=g).to(dtype).to(DEV)
    for shift in (None, 0, 1, 2, 3):
        flags = None if shift is None else torch.tensor([(shift + i) % 4 for i in range(n)], dtype=torch.uint8, device=DEV)
        x = feat.clone().requires_grad_(True)
        joint, marg = F_hip.mine_pairs(x, flags, dtype)
        (dx,) = torch.autograd.grad([joint, marg], x, [gj, gm])
        y = feat.clone().requires_grad_(True)
        feat1 = y[n:]
        feat2 = F_hip.flip_batch(y[:n], flags) if flags is not None else y[:n]
        want_j = torch.cat([feat1, feat2], 1)
        want_m = torch.cat([feat1, torch.roll(feat2, -1, 0)], 1)
        (dy,) = torch.autograd.grad([want_j, want_m], y, [gj, gm])
        assert joint.dtype == dtype and tuple(joint.shape) == (n, 2 * C, H, W)
        assert torch.equal(joint, want_j) and torch.equal(marg, want_m), shift
        assert dx.dtype == dtype and torch.equal(dx, dy), shift
        for t in (joint, marg):  # pad channels of the storage are zero
            st, cs = F_hip.as_nhwc(t)
            assert cs == (2 * C + 15) // 16 * 16 and bool((st[..., 2 * C:] == 0).all())


def _activation(n, CH, H, W, dtype, seed):
    """a stored ReLU output with the crafted channels (sample 0): 0 constant, 1 two equal maxima, 2 all zero"""
    g = torch.Generator().manual_seed(seed)
    a = torch.relu(torch.randn(n, CH, H, W, generator=g))
    a[0, 0] = 0.5
    if H * W > 1:
        flat = a[0, 1].reshape(-1)
        flat[H * W - 1] = flat[(H * W) // 2] = float(flat.max()) + 1.0
    a[0, 2] = 0.0
    return a.to(dtype)


# (23 x 29 and 56 x 56: more than one 256-pixel slab per sample, the last one short; the crafted ties then span slabs)
HEAD_SHAPES = [(1, 4, 5, 7), (3, 8, 5, 7), (2, 48, 14, 14), (3, 128, 14, 14), (2, 256, 3, 3), (2, 16, 1, 1), (2, 16, 23, 29),
               (1, 32, 56, 56)]


def _head(n, CH, H, W, dtype, seed=0):
    from spcl_amd import functional as F_hip
    g = torch.Generator().manual_seed(77 + seed)
    acts = [_activation(n, CH, H, W, dtype, 500 + 2 * seed + k) for k in range(2)]
    lw = torch.randn(1, CH, generator=g) / CH ** 0.5
    lb = torch.randn(1, generator=g)
    dev = [a.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True) for a in acts]
    lwd, lbd = lw.to(DEV).requires_grad_(True), lb.to(DEV).requires_grad_(True)
    out = {}
    loss = F_hip.mine_head(dev[0], dev[1], lwd, lbd, dtype, out=out)
    (3.0 * loss).backward()
    torch.cuda.synchronize()
    return acts, lw, lb, dev, lwd, lbd, out, loss


def _head_reference(acts, lw, lb, dtype):
    a = [x.to(dtype).requires_grad_(True) for x in acts]
    w, b = lw.to(dtype).requires_grad_(True), lb.to(dtype).requires_grad_(True)
    sd = {"8.weight": w, "8.bias": b}
    loss = F.softplus(M.head(a[1], sd)).mean() + F.softplus(M.head(a[0], sd)).mean()
    (3.0 * loss).backward()
    return loss.detach(), w.grad, b.grad, [x.grad for x in a]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_head_forward_and_backward(shape, dtype):
    n, CH, H, W = shape
    acts, lw, lb, dev, lwd, lbd, out, loss = _head(n, CH, H, W, dtype)
    stored = [a.float() for a in acts]  # the values the kernel read, exactly
    for p in range(2):
        want, idx = F.adaptive_max_pool2d(stored[p], 1, return_indices=True)
        assert torch.equal(out["maxima"][p].cpu(), want.reshape(n, CH)), p
        assert torch.equal(out["argmax"][p].cpu().long(), idx.reshape(n, CH)), p
    assert float(out["maxima"][0][0, 0]) == 0.5 and int(out["argmax"][0][0, 0]) == 0      # a constant map: the first index
    if H * W > 1:
        assert int(out["argmax"][0][0, 1]) == (H * W) // 2                                  # two equal maxima: the first
    assert float(out["maxima"][0][0, 2]) == 0.0 and int(out["argmax"][0][0, 2]) == 0        # nothing positive
    l64, dw64, db64, da64 = _head_reference(stored, lw, lb, torch.float64)
    l32, dw32, db32, _ = _head_reference(stored, lw, lb, torch.float32)
    tol = M.bound(l32, l64, M.FLOOR_HEAD)
    print(f"loss {float(loss.detach()):.9g} vs {float(l64):.9g} (bound {tol:.1e}); t {out['t'].flatten().tolist()}")
    assert abs(float(loss.detach()) - float(l64)) <= tol * abs(float(l64))
    assert M.rel_l2(lwd.grad, dw64) <= M.bound(dw32, dw64, M.FLOOR_HEAD)
    assert M.rel_l2(lbd.grad, db64) <= M.bound(db32, db64, M.FLOOR_HEAD)
    # activation gradients: exactly zero off the argmax, w_c dt at it (one rounding to the storage type)
    ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -23
    for p in range(2):
        got = dev[p].grad.float().cpu()
        assert got.shape == da64[p].shape
        hit = torch.zeros(n, CH, H * W, dtype=torch.bool)
        hit.scatter_(2, out["argmax"][p].cpu().long().unsqueeze(2), True)
        hit = hit.reshape(n, CH, H, W)
        assert bool((got[~hit] == 0).all()), p
        assert bool((da64[p][~hit] == 0).all()), p
        want = da64[p][hit]
        assert bool(((got[hit].double() - want).abs() <= (ulp + 4e-6) * want.abs() + 1e-30).all()), p


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_two_identical_calls_give_the_same_bits(dtype):
    a = _head(3, 128, 14, 14, dtype, seed=1)
    b = _head(3, 128, 14, 14, dtype, seed=1)
    assert torch.equal(a[7], b[7])
    for k in ("t", "maxima", "argmax"):
        assert torch.equal(a[6][k], b[6][k]), k
    assert torch.equal(a[4].grad, b[4].grad) and torch.equal(a[5].grad, b[5].grad)
    for x, y in zip(a[3], b[3]):
        assert torch.equal(x.grad, y.grad)
