"""GPU: the kernels of the label-guided pixel contrast (csrc/pixel_contrast.hip) through their functional wrappers.

Sampler: ``idx`` and ``count`` equal the integer restatement of tests/_pixel_contrast_oracle.py exactly.  Gather: bit-equal to
torch indexing / ``index_put``.  Criterion: against float64 autograd of the restatement at the bars tests/test_gpu_loss.py and
tests/test_gpu_weighted_supcon.py hold the f32 contrastive criteria to -- loss rtol 1e-4 / atol 1e-5, gradient rtol 1e-3 /
atol 1e-5 -- with the observed errors printed."""
import numpy as np
import pytest
import torch

from tests import _pixel_contrast_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _F():
    import spcl_amd  # noqa: F401
    from spcl_amd import functional
    return functional


# ------------------------------------------------------------------------------------------------ sampler
def _label_map(B, h, w, C, seed, ineligible=0.2):
    g = np.random.default_rng(seed)
    lab = g.integers(0, C, size=(B, h, w)).astype(np.int32)
    lab[g.random((B, h, w)) < ineligible] = -1
    return lab


def _small_map(absent=False):
    """2 x 8 x 8, C = 3, K = 4: class 0 has far more than K cells, class 1 exactly K, class 2 fewer (or none)"""
    lab = np.full(128, -1, dtype=np.int32)
    g = np.random.default_rng(3)
    cells = g.permutation(128)
    lab[cells[:60]] = 0
    lab[cells[60:64]] = 1
    if not absent:
        lab[cells[64:66]] = 2
    return lab.reshape(2, 8, 8)


def _check_sample(lab, C, K, seed):
    F = _F()
    idx, count = F.pixel_sample(torch.from_numpy(lab).to(DEV), C, K, seed)
    want_idx, want_count = O.sample(lab, C, K, seed)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (C, K) and tuple(count.shape) == (C,)
    assert np.array_equal(count.cpu().numpy(), want_count), (count.tolist(), want_count.tolist())
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    return idx, count


@pytest.mark.parametrize("absent", [False, True], ids=["all-classes", "class-absent"])
def test_sampler_small_map_around_K(absent):
    lab = _small_map(absent)
    _, count = _check_sample(lab, 3, 4, 0)
    assert count.tolist() == [4, 4, 0 if absent else 2]


@pytest.mark.parametrize("B,h,w,C,K", [(3, 37, 53, 4, 64), (5, 112, 112, 4, 256), (1, 224, 224, 16, 256)],
                         ids=["odd", "many-workgroups", "C16-M4096"])
def test_sampler_equals_the_integer_oracle(B, h, w, C, K):
    _check_sample(_label_map(B, h, w, C, 11), C, K, 5)


def test_sampler_all_ineligible_and_K_above_every_class():
    idx, count = _check_sample(np.full((2, 9, 7), -1, dtype=np.int32), 3, 8, 1)
    assert count.tolist() == [0, 0, 0] and bool((idx == -1).all())
    lab = _label_map(2, 9, 7, 3, 2)
    idx, count = _check_sample(lab, 3, 128, 1)  # K larger than every class: every eligible cell, in index order
    assert count.tolist() == [int((lab == c).sum()) for c in range(3)]
    lab[0, 0, :3] = [3, 100, -7]  # values outside [0, C) are ineligible, whatever they are
    _check_sample(lab, 3, 5, 1)


@pytest.mark.parametrize("seed", [0, 1, 0x80000000, 0xFFFFFFFF])
def test_sampler_seeds_int_and_tensor(seed):
    F = _F()
    lab = _label_map(3, 37, 53, 4, 12)
    idx, count = _check_sample(lab, 4, 64, seed)
    word = torch.tensor([seed - 2 ** 32 if seed >= 2 ** 31 else seed], dtype=torch.int32, device=DEV)
    idx_t, count_t = F.pixel_sample(torch.from_numpy(lab).to(DEV), 4, 64, word)
    assert torch.equal(idx_t, idx) and torch.equal(count_t, count)


def test_sampler_repeats_its_bits_and_seeds_differ():
    F = _F()
    lab = torch.from_numpy(_label_map(5, 112, 112, 4, 13)).to(DEV)  # n_c ~ 12500 >= 8 K
    a, b = F.pixel_sample(lab, 4, 256, 7), F.pixel_sample(lab, 4, 256, 7)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = F.pixel_sample(lab, 4, 256, 8)
    assert torch.equal(c[1], a[1])
    for k in range(4):
        assert not torch.equal(c[0][k], a[0][k])


def test_sampler_capture_and_replay_reads_the_seed_word():
    F = _F()
    lab_np = _label_map(3, 37, 53, 4, 14)
    lab = torch.from_numpy(lab_np).to(DEV)
    word = torch.tensor([3], dtype=torch.int32, device=DEV)
    F.pixel_sample(lab, 4, 64, word)  # (warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        idx, count = F.pixel_sample(lab, 4, 64, word)
    for seed in (3, 4, 0xFFFFFFFF):
        word.fill_(seed - 2 ** 32 if seed >= 2 ** 31 else seed)
        graph.replay()
        torch.cuda.synchronize()
        want_idx, want_count = O.sample(lab_np, 4, 64, seed)
        assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(count.cpu().numpy(), want_count)


# ------------------------------------------------------------------------------------------------ gather
def _feature(B, Cf, h, w, dtype, padded):
    g = torch.Generator().manual_seed(Cf + 7 * B)
    cs = Cf + 16 if padded else Cf
    store = torch.randn(B, h, w, cs, generator=g).to(dtype).to(DEV)
    return store.permute(0, 3, 1, 2)[:, :Cf], store, cs


@pytest.mark.parametrize("padded", [False, True], ids=["dense", "padded-pitch"])
@pytest.mark.parametrize("Cf", [6, 16, 32, 256])  # (6: no 16-byte path, one element per thread)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_gather_rows_and_its_gradient_are_bit_equal_to_indexing(dtype, Cf, padded):
    F = _F()
    B, h, w = 2, 9, 11
    feat, store, cs = _feature(B, Cf, h, w, dtype, padded)
    g = torch.Generator().manual_seed(1)
    chosen = torch.randperm(B * h * w, generator=g)[:21].to(torch.int32)
    idx = torch.cat([chosen[:10], torch.tensor([-1, -1], dtype=torch.int32), chosen[10:], torch.tensor([-1], dtype=torch.int32)])
    idx = idx.to(DEV)
    leaf = feat.detach().requires_grad_(True)
    rows = F.gather_rows(leaf, idx.view(2, 12))
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (24, Cf)
    flat = store.reshape(B * h * w, cs)[:, :Cf].float()
    real = idx >= 0
    want = torch.zeros(24, Cf, device=DEV)
    want[real] = flat[idx[real].long()]
    assert torch.equal(rows.detach(), want)
    assert bool((rows.detach()[~real] == 0).all())
    up = torch.randn(24, Cf, generator=g).to(DEV)
    rows.backward(up)
    grad = leaf.grad
    assert grad.dtype == dtype and grad.shape == feat.shape
    want_g = torch.zeros(B * h * w, Cf, dtype=dtype, device=DEV)
    want_g.index_put_((idx[real].long(),), up[real].to(dtype))
    got_g = grad.permute(0, 2, 3, 1).reshape(B * h * w, Cf)
    assert torch.equal(got_g, want_g)
    untouched = torch.ones(B * h * w, dtype=torch.bool, device=DEV)
    untouched[idx[real].long()] = False
    assert bool((got_g[untouched] == 0).all())


# ------------------------------------------------------------------------------------------------ criterion
def _mixed(C, K, seed):
    g = np.random.default_rng(seed)
    count = [int(v) for v in g.integers(0, K + 1, size=C)]
    count[0], count[-1] = K, 1
    return count


SHAPES = [
    (3, 4, 8, [4, 2, 0]),
    (3, 4, 8, [4, 1, 3]),
    (4, 16, 32, [16, 16, 16, 16]),
    (4, 17, 32, [17, 16, 1, 9]),
    (5, 64, 128, _mixed(5, 64, 1)),
    (4, 256, 256, [256, 100, 0, 7]),
    (16, 256, 64, _mixed(16, 256, 2)),
]
_REFERENCE = {}


def _rows(C, K, d, seed=0):
    g = torch.Generator().manual_seed(1000 * C + K + d + seed)
    return torch.nn.functional.normalize(torch.randn(C * K, d, generator=g), dim=1)


def _reference(C, K, d, count, t):
    """float64 loss and gradient of the restatement, computed once per case"""
    key = (C, K, d, tuple(count), t)
    if key not in _REFERENCE:
        z = _rows(C, K, d).double().requires_grad_(True)
        loss = O.supcon(z, count, K, t)
        loss.backward()
        _REFERENCE[key] = (float(loss.detach()), z.grad.clone())
    return _REFERENCE[key]


def _run(z, count, K, t, upstream=None):
    F = _F()
    leaf = z.to(DEV).requires_grad_(True)
    cnt = torch.tensor(count, dtype=torch.int32, device=DEV)
    loss = F.pixel_supcon(leaf, cnt, K, t)
    if upstream is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(upstream, device=DEV))
    return loss.detach(), leaf.grad


def _close(got, want, rtol, what):
    g, w = got.detach().double().cpu().numpy(), np.asarray(want, dtype=np.float64)
    print(f"{what}: max |diff| {np.abs(g - w).max():.3e} (max |want| {np.abs(w).max():.3e})")
    np.testing.assert_allclose(g, w, rtol=rtol, atol=1e-5, err_msg=what)


@pytest.mark.parametrize("t", [0.07, 0.1, 1.0])
@pytest.mark.parametrize("C,K,d,count", SHAPES, ids=[f"C{c}_K{k}_d{d}" + "_" + "-".join(map(str, n[:4])) for c, k, d, n in SHAPES])
def test_criterion_matches_float64_autograd(C, K, d, count, t):
    want_loss, want_grad = _reference(C, K, d, count, t)
    loss, grad = _run(_rows(C, K, d), count, K, t)
    what = f"C{C}_K{K}_d{d}_t{t}"
    _close(loss, want_loss, 1e-4, what + " loss")
    _close(grad, want_grad.numpy(), 1e-3, what + " dz")
    valid, _ = O.slots(count, K)
    assert bool((grad.cpu()[~valid] == 0).all())


def test_criterion_without_positives_is_exactly_zero():
    loss, grad = _run(_rows(2, 1, 4), [1, 1], 1, 0.1)
    assert float(loss) == 0.0 and bool((grad == 0).all())


def test_criterion_never_reads_invalid_rows():
    C, K, d, count = 4, 17, 32, [17, 16, 1, 9]
    valid, _ = O.slots(count, K)
    z = _rows(C, K, d)
    zeros, nans = z.clone(), z.clone()
    zeros[~valid] = 0.0
    nans[~valid] = float("nan")
    la, ga = _run(zeros, count, K, 0.1)
    lb, gb = _run(nans, count, K, 0.1)
    assert bool(torch.isfinite(lb)) and bool(torch.isfinite(gb).all())
    assert torch.equal(la, lb) and torch.equal(ga, gb)
    assert bool((gb.cpu()[~valid] == 0).all())


def test_criterion_upstream_gradient_scales():
    C, K, d, count = 3, 4, 8, [4, 1, 3]
    _, want_grad = _reference(C, K, d, count, 0.1)
    _, grad = _run(_rows(C, K, d), count, K, 0.1, upstream=2.5)
    _close(grad, 2.5 * want_grad.numpy(), 1e-3, "upstream 2.5 dz")


def test_criterion_repeats_its_bits_and_replays_from_a_graph():
    F = _F()
    C, K, d, count = 5, 64, 128, _mixed(5, 64, 1)
    z = _rows(C, K, d)
    la, ga = _run(z, count, K, 0.1)
    lb, gb = _run(z, count, K, 0.1)
    assert torch.equal(la, lb) and torch.equal(ga, gb)
    zd = z.to(DEV)
    cnt = torch.tensor(count, dtype=torch.int32, device=DEV)
    one = torch.ones((), device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # (warm-up on a side stream, as torch asks before a capture with autograd)
        leaf = zd.clone().requires_grad_(True)
        F.pixel_supcon(leaf, cnt, K, 0.1).backward(one)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    leaf = zd.clone().requires_grad_(True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = F.pixel_supcon(leaf, cnt, K, 0.1)
        (grad,) = torch.autograd.grad(loss, leaf, one)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, la) and torch.equal(grad, ga)


def test_criterion_is_invariant_to_the_order_inside_a_class():
    C, K, d, count = 4, 17, 32, [17, 16, 1, 9]
    z = _rows(C, K, d)
    want_loss, _ = _reference(C, K, d, count, 0.1)
    perm = torch.arange(C * K)
    g = torch.Generator().manual_seed(9)
    perm[K:K + 16] = K + torch.randperm(16, generator=g)  # the 16 valid rows of class 1
    loss, _ = _run(z[perm], count, K, 0.1)
    _close(loss, want_loss, 1e-4, "permuted class 1 loss")
