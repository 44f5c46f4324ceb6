"""GPU: ``spcl_ucmt_softmax_mse`` (csrc/semi_reg.hip) through ``functional.ucmt_softmax_mse`` against the float64 restatement
of tests/_ucmt_oracle.py; two runs give the same bits.

The mask is a threshold compare of an f32 entropy: it cannot agree with float64 at pixels whose entropy sits on the
threshold.  So, as the project does elsewhere for f32 ties (a capped tie slack plus tie-independent checks):

(a) the kernel's mask equals the oracle's at every pixel with |u64 - threshold| > BAND = 2e-6 (f32 against f64 entropy was
    seen to differ by at most 2.4e-7 on these inputs on the CPU: about 8x room for ``expf`` / ``logf``);
(b) the pixels inside the band number at most max(1, 0.2 % of M) -- asserted on the oracle alone, before the kernel is looked
    at; the seed is pinned so that this holds (with a band five times wider the CPU saw at most 1 pixel of 1440 at the small
    shapes and 4.8e-5 of the pixels at 10 x 4 x 224 x 224);
(c) ``kept`` equals the sum of the kernel's own mask;
(d) with the KERNEL's mask given to the oracle, loss within 1e-5 relative and gradient within 1e-5 relative L2 -- the bars of
    ``test_mt_softmax_mse_vs_float64`` and ``test_entropy_softmax_vs_float64``.

The noisy maps are 3 * randn each: the average of K = 8 has about unit scale, and the two thresholds keep roughly a third to
three quarters of the pixels.  Shapes: C = 4 with and without flags (the 16-byte path), C = 2 at odd sizes below one
workgroup, C = 16 (the maximum), and the reference's batch."""
import functools

import pytest
import torch

from tests import _ucmt_oracle as UO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 11
BAND = 2e-6
BIG_FLAGS = (3, 0, 1, 2, 0, 3, 1, 2, 0, 3)
SMALL = [((3, 4, 20, 24), (3, 0, 1)), ((3, 4, 20, 24), None), ((2, 2, 5, 7), (2, 1)), ((1, 16, 9, 33), (3,))]
CASES = [(shape, flags, K, th) for shape, flags in SMALL for K in (1, 8) for th in (0.75, 0.9)] + \
        [((10, 4, 224, 224), BIG_FLAGS, 8, 0.75)]


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _cl(x):
    return x.to(DEV).contiguous(memory_format=torch.channels_last)


@functools.lru_cache(maxsize=2)
def _inputs(shape, flags, K):
    """(teacher, student, noisy maps, float64 entropy): drawn and restated once per (shape, flags, K), never modified"""
    g = torch.Generator().manual_seed(SEED)
    t, s = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
    noisy = tuple(3.0 * torch.randn(*shape, generator=g) for _ in range(K))
    return t, s, noisy, UO.entropy(noisy, flags)


def _run(t, noisy, s, th, weight, flags, upstream=None):
    from spcl_amd import functional as F_hip
    fl = None if flags is None else torch.tensor(flags, dtype=torch.uint8, device=DEV)
    td, nd = _cl(t).requires_grad_(True), [_cl(x).requires_grad_(True) for x in noisy]
    sd = _cl(s).requires_grad_(True)
    out = []
    loss = F_hip.ucmt_softmax_mse(td, nd, sd, th, weight, fl, out=out)
    (loss if upstream is None else upstream * loss).backward()
    assert td.grad is None and all(x.grad is None for x in nd)
    kept, mask = out
    assert kept.is_cuda and mask.shape == (s.shape[0], s.shape[2], s.shape[3]) and mask.dtype == torch.uint8
    return loss.detach().clone(), sd.grad.clone(), kept.clone(), mask.clone()


@pytest.mark.parametrize("shape,flags,K,th", CASES)
def test_ucmt_softmax_mse_vs_float64(shape, flags, K, th):
    t, s, noisy, u64 = _inputs(shape, flags, K)
    M = u64.numel()
    weight = 1.0 if flags is None else 2.5
    in_band = (u64 - th).abs() <= BAND
    assert int(in_band.sum()) <= max(1, int(0.002 * M)), int(in_band.sum())  # (b): the oracle alone
    runs = [_run(t, noisy, s, th, weight, flags) for _ in range(2)]
    loss, grad, kept, mask = runs[0]
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    mask = mask.cpu()
    ref_mask = (u64 <= th)
    wrong = (mask.bool() != ref_mask) & ~in_band
    assert int(wrong.sum()) == 0, int(wrong.sum())  # (a)
    assert int(kept) == int(mask.sum())  # (c)
    s64 = s.double().requires_grad_(True)
    ref = UO.loss(t, s64, mask, weight, flags)  # (d): the kernel's own mask
    ref.backward()
    lerr = abs(float(loss) - float(ref.detach())) / float(ref.detach())
    gerr = _rel_l2(grad, s64.grad)
    print(f"ucmt {shape} flags={flags is not None} K={K} th={th}: kept {int(kept)} of {M}, in band {int(in_band.sum())}, "
          f"mask differs at {int((mask.bool() != ref_mask).sum())}, loss rel {lerr:.2e}, grad rel L2 {gerr:.2e}")
    assert 0 < int(kept) <= M  # (the reference loss is not zero; C = 16 with K = 1 at 0.9 keeps every pixel)
    assert lerr <= 1e-5 and gerr <= 1e-5, (lerr, gerr)
    # pixels outside the mask carry exact zeros
    dropped = (mask == 0)[:, None].expand_as(grad.cpu())
    assert not bool(grad.cpu()[dropped].any())


def test_a_threshold_below_every_entropy_keeps_nothing():
    shape, flags = SMALL[0]
    t, s, noisy, _ = _inputs(shape, flags, 8)
    loss, grad, kept, mask = _run(t, noisy, s, -1.0, 2.5, flags)
    assert float(loss) == 0.0 and int(kept) == 0 and not bool(mask.any())
    assert not bool(grad.any())


def test_a_threshold_above_every_entropy_is_the_plain_criterion():
    shape, flags = SMALL[0]
    t, s, noisy, u64 = _inputs(shape, flags, 8)
    loss, grad, kept, mask = _run(t, noisy, s, 2.0, 2.5, flags)
    assert int(kept) == u64.numel() and bool(mask.all())
    s64 = s.double().requires_grad_(True)
    ref = UO.unmasked_mse(t, s64, 2.5, flags)
    ref.backward()
    assert abs(float(loss) - float(ref.detach())) <= 1e-5 * float(ref.detach())
    assert _rel_l2(grad, s64.grad) <= 1e-5


def test_a_non_unit_upstream_gradient_is_scaled():
    shape, flags = SMALL[0]
    t, s, noisy, _ = _inputs(shape, flags, 8)
    _, g1, _, m1 = _run(t, noisy, s, 0.9, 1.0, flags)
    _, g3, _, m3 = _run(t, noisy, s, 0.9, 1.0, flags, upstream=3.0)
    assert torch.equal(m1, m3)
    s64 = s.double().requires_grad_(True)
    (3.0 * UO.loss(t, s64, m3.cpu(), 1.0, flags)).backward()
    assert _rel_l2(g3, s64.grad) <= 1e-5
    assert _rel_l2(g3, 3.0 * g1) <= 1e-6


def test_bad_arguments_are_refused_with_an_error():
    from spcl_amd import functional as F_hip
    t = torch.zeros(1, 4, 8, 8, device=DEV)
    with pytest.raises((ValueError, RuntimeError)):
        F_hip.ucmt_softmax_mse(t, [], t, 0.75)  # K = 0
    with pytest.raises((ValueError, RuntimeError)):
        F_hip.ucmt_softmax_mse(t, [t] * 17, t, 0.75)  # K = 17
    t17 = torch.zeros(1, 17, 8, 8, device=DEV)
    with pytest.raises(RuntimeError, match="C <= 16"):
        F_hip.ucmt_softmax_mse(t17, [t17], t17, 0.75)  # C = 17
    with pytest.raises(RuntimeError):
        F_hip.ucmt_softmax_mse(t.cpu(), [t.cpu()], t.cpu(), 0.75)  # no CPU path
    torch.cuda.synchronize()
