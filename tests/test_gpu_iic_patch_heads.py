"""GPU: the patch-wise IIC criterion over S subheads (csrc/iic_patch.hip ``spcl_iic_patch_heads_*``,
functional.iic_patch_heads_loss) against the float64 restatement of the decoder branch of ``IICEstimator``
(tests/_iic_estimator_oracle.py), scale = 0.1.

Bars (those of tests/test_gpu_midl_kernels.py).  Each loss_{s,P}: 1e-5 relative, 1e-9 absolute where |loss| < 1e-4.  Total
loss: 1e-5 relative.  Gradients: relative L2 within ``max(1e-5, e32)`` where ``e32`` is the error of the SAME oracle evaluated
in float32 on the CPU against its float64 evaluation; each test prints ``e32`` next to the kernel's error.  The references of a
case are computed once and shared by its tests.  The maps carry ``ld`` channels; those beyond S*K hold logits that no subhead
reads and must get no gradient."""
import ctypes
import functools

import pytest
import torch

from tests import _iic_estimator_oracle as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = 0.1
SENTINEL = -77.0

CASES = [  # (N, S, K, H, W, pad, patch, flags, ld)
    (2, 1, 4, 20, 24, 1, 8, [1, 2], 4),           # must agree with the single-subhead entry
    (2, 3, 5, 21, 27, 1, 8, [3, 0], 16),          # pitch wider than S*K; K not a multiple of 4; irregular last starts
    (2, 5, 20, 12, 12, 1, 1024, [0, 3], 100),     # the config default: K = 20, one clipped patch
    (1, 2, 32, 12, 12, 0, 6, None, 64),           # the maximum K, pad 0
    (2, 2, 17, 9, 7, 2, 16, [2, 1], 34),          # K not a multiple of 4 (KP = 20); patch larger than the map; pad 2
    (2, 5, 10, 40, 56, 3, 16, [1, 0], 50),        # pad = 3: 7 * 9 = 63 tiles a displacement row
    (2, 5, 20, 56, 56, 1, 32, [3, 0], 100),       # nine patches a subhead
]
IDS = [f"case{k + 1}" for k in range(len(CASES))]


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _logits(N, ld, H, W):
    g = torch.Generator().manual_seed(1)
    lx = torch.randn(N, ld, H, W, generator=g)
    ly = torch.randn(N, ld, H, W, generator=g)
    return lx.float(), ly.float()


@functools.lru_cache(maxsize=None)
def _reference(case):
    """(loss, losses [S, nP], gx, gy, e32x, e32y): the float64 oracle and the float32 oracle's gradient errors against it"""
    N, S, K, H, W, pad, patch, flags, ld = CASES[case]
    lx, ly = _logits(N, ld, H, W)
    loss, per, gx, gy = E.patch_heads_evaluate(lx, ly, S, K, pad, patch, flags, SCALE, torch.float64)
    _, _, gx32, gy32 = E.patch_heads_evaluate(lx, ly, S, K, pad, patch, flags, SCALE, torch.float32)
    return loss, per, gx, gy, _rel_l2(gx32, gx), _rel_l2(gy32, gy)


@functools.lru_cache(maxsize=None)
def _hip(case, ly_grad=False, upstream=None):
    from spcl_amd import functional as F_hip
    N, S, K, H, W, pad, patch, flags, ld = CASES[case]
    lx, ly = _logits(N, ld, H, W)
    x = lx.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ly.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(ly_grad)
    fl = None if flags is None else torch.tensor(flags, dtype=torch.uint8, device=DEV)
    out = []
    loss = F_hip.iic_patch_heads_loss(x, y, num_subheads=S, num_clusters=K, padding=pad, patch_size=patch, scale=SCALE,
                                      flags=fl, out=out)
    (loss if upstream is None else upstream * loss).backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), out[0].cpu(), out[1].cpu(), x.grad.cpu(), None if y.grad is None else y.grad.cpu()


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_losses_and_lx_gradient_vs_float64(case):
    N, S, K, H, W, pad, patch, flags, ld = CASES[case]
    ref_loss, ref_per, ref_gx, _, e32x, _ = _reference(case)
    loss, per, flag, gx, gy = _hip(case)
    assert per.shape == ref_per.shape and per.shape[0] == S
    err = (per.double() - ref_per).abs()
    small = ref_per.abs() < 1e-4
    rel = err / ref_per.abs().clamp_min(1e-300)
    lerr = abs(float(loss) - float(ref_loss)) / abs(float(ref_loss))
    gerr = _rel_l2(gx, ref_gx)
    print(f"{S} x {per.shape[1]} losses ({int(small.sum())} below 1e-4), {float(ref_per.min()):.3g} .. "
          f"{float(ref_per.max()):.3g}: worst rel {float(rel[~small].max()) if bool((~small).any()) else 0.0:.2e}, "
          f"worst abs among the small {float(err[small].max()) if bool(small.any()) else 0.0:.2e}; loss rel {lerr:.2e}; "
          f"d lx rel L2 {gerr:.2e} (float32 oracle: {e32x:.2e})")
    assert bool(((rel <= 1e-5) | (small & (err <= 1e-9))).all()), (float(rel.max()), float(err.max()))
    assert lerr <= 1e-5, (float(loss), float(ref_loss))
    assert gerr <= max(1e-5, e32x), (gerr, e32x)
    assert int(flag[0]) == 0
    assert gy is None  # ly did not require grad: d ly is written only when asked for
    assert bool((gx[:, S * K:] == 0).all())  # channels no subhead reads


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_ly_gradient_vs_float64_and_lx_gradient_unchanged(case):
    N, S, K = CASES[case][:3]
    _, _, _, ref_gy, _, e32y = _reference(case)
    loss0, per0, _, gx0, _ = _hip(case)
    loss, per, flag, gx, gy = _hip(case, ly_grad=True)
    gerr = _rel_l2(gy, ref_gy)
    print(f"d ly rel L2 {gerr:.2e} (float32 oracle: {e32y:.2e})")
    assert gerr <= max(1e-5, e32y), (gerr, e32y)
    assert torch.equal(gx, gx0) and torch.equal(loss, loss0) and torch.equal(per, per0)
    assert bool((gy[:, S * K:] == 0).all())
    assert int(flag[0]) == 0


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_a_second_call_gives_the_same_bits(case):
    a = _hip(case, ly_grad=True)
    b = _hip.__wrapped__(case, ly_grad=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("case", [1, 2, 3], ids=["case2", "case3", "case4"])
def test_non_unit_upstream_gradient(case):
    _, _, _, gx, gy = _hip(case, ly_grad=True)
    _, _, _, gx3, gy3 = _hip(case, ly_grad=True, upstream=3.0)
    assert _rel_l2(gx3, 3.0 * gx) <= 1e-6 and _rel_l2(gy3, 3.0 * gy) <= 1e-6, (_rel_l2(gx3, 3.0 * gx), _rel_l2(gy3, 3.0 * gy))


def test_one_subhead_agrees_with_the_single_subhead_entry():
    from spcl_amd import functional as F_hip
    N, S, K, H, W, pad, patch, flags, ld = CASES[0]
    assert S == 1 and ld == K
    loss, per, _, gx, gy = _hip(0, ly_grad=True)
    lx, ly = _logits(N, ld, H, W)
    x = lx.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ly.to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    out = []
    want = F_hip.iic_patch_loss(x, y, padding=pad, patch_size=patch, scale=SCALE,
                                flags=torch.tensor(flags, dtype=torch.uint8, device=DEV), out=out)
    want.backward()
    lerr = abs(float(loss) - float(want.detach())) / abs(float(want.detach()))
    ex, ey = _rel_l2(gx, x.grad), _rel_l2(gy, y.grad)
    print(f"loss rel {lerr:.2e}; d lx {ex:.2e}; d ly {ey:.2e}")
    assert lerr <= 1e-6 and ex <= 1e-6 and ey <= 1e-6, (lerr, ex, ey)
    assert _rel_l2(per[0], out[0]) <= 1e-6


def test_backward_leaves_the_columns_beyond_the_subheads_alone():
    """the library call itself on gradient buffers prefilled with a sentinel: columns >= S*K = 15 of the 16-wide rows keep it,
    every column below is written"""
    from spcl_amd import native as _n
    N, S, K, H, W, pad, patch, flags, ld = CASES[1]
    lx, ly = _logits(N, ld, H, W)
    xs = lx.to(DEV).permute(0, 2, 3, 1).contiguous()
    ys = ly.to(DEV).permute(0, 2, 3, 1).contiguous()
    fl = torch.tensor(flags, dtype=torch.uint8, device=DEV)
    nP, wsb, dje = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    _n.call("spcl_iic_patch_heads_plan", N, S, K, ld, H, W, pad, patch, ctypes.byref(nP), ctypes.byref(wsb), ctypes.byref(dje))
    ws = torch.empty(wsb.value, dtype=torch.uint8, device=DEV)
    dj = torch.empty(dje.value, dtype=torch.float32, device=DEV)
    loss = torch.empty((), dtype=torch.float32, device=DEV)
    flag = torch.empty(1, dtype=torch.int32, device=DEV)
    _n.call("spcl_iic_patch_heads_forward", _n.ptr(xs), _n.ptr(ys), ld, N, H, W, S, K, pad, patch, _n.ptr(fl),
            ctypes.c_float(SCALE), _n.ptr(loss), None, _n.ptr(flag), _n.ptr(dj), _n.ptr(ws), ws.numel(), _n.stream())
    dlx = torch.full_like(xs, SENTINEL)
    dly = torch.full_like(ys, SENTINEL)
    _n.call("spcl_iic_patch_heads_backward", _n.ptr(xs), _n.ptr(ys), ld, N, H, W, S, K, pad, patch, _n.ptr(fl), _n.ptr(dj),
            None, _n.ptr(dlx), _n.ptr(dly), _n.stream())
    torch.cuda.synchronize()
    for g in (dlx, dly):
        assert bool((g[..., S * K:] == SENTINEL).all())
        assert not bool((g[..., :S * K] == SENTINEL).any())
    _, _, _, gx, gy = _hip(1, ly_grad=True)
    assert torch.equal(dlx[..., :S * K].cpu(), gx.permute(0, 2, 3, 1)[..., :S * K])
    assert torch.equal(dly[..., :S * K].cpu(), gy.permute(0, 2, 3, 1)[..., :S * K])
    assert abs(float(loss) - float(_hip(1)[0])) == 0.0


@pytest.mark.parametrize("S,K,pad,patch,ld,word", [(1, 33, 1, 8, 33, "K = 33"), (1, 4, 8, 8, 4, "padding 8"),
                                                   (1, 4, 1, 1, 4, "patch size 1"), (3, 5, 1, 8, 14, "ld = 14")])
def test_argument_errors_carry_the_librarys_message(S, K, pad, patch, ld, word):
    from spcl_amd import native as _n
    x = torch.zeros(1, ld, 8, 8, device=DEV)
    with pytest.raises(RuntimeError, match=word):
        _n.call("spcl_iic_patch_heads_plan", 1, S, K, ld, 8, 8, pad, patch, None, None, None)
    from spcl_amd import functional as F_hip
    with pytest.raises(RuntimeError, match=word):
        F_hip.iic_patch_heads_loss(x, x, num_subheads=S, num_clusters=K, padding=pad, patch_size=patch)
