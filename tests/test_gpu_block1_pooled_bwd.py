"""The image block's backward without the gradient tensor behind Conv1.b's BatchNorm + ReLU + max-pool (reference
semi_seg/arch/unet.py:75-77, 118-121 and autograd): the one-pass backward of Conv1.b (csrc/conv16_bwd.hip, POOLDY) forms that
gradient per tile in its loader from Conv1.b's raw output and the pooled gradient, with the expression sequence of the
BatchNorm apply pass (csrc/pool_dy.hpp).  spcl_conv16_bwd_fused_image_pooled replaces spcl_bnrelu_backward_rows_acc -> dy
followed by spcl_conv16_bwd_fused_image; nothing is approximated, so every comparison is bit for bit on integer views (a NaN
compares by its bits too).

Shapes (N, H, W), the whole-tile shapes of tests/test_gpu_block1_recompute.py: 3 x 14 x 14 one tile whose whole halo is
padding (72 of its 81 windows lie outside the image), three images = a ragged walk; 2 x 28 x 28 every tile touches a border;
1 x 42 x 56 an interior tile and all four edges.  Inputs follow tests/test_gpu_poolmax.py: y = multiples of 1/8 in [-4, 4]
(tied maxima in most windows), BatchNorm coefficients with negative-scale channels, a zero-scale channel and a channel that
is non-positive after BN, a NaN in y at window position (1, 0) and one at (0, 1).  A padding pixel formed as A 0 + B instead
of 0 would move every border tile's weight gradient: the gradient is non-zero on the border in every channel but the
zero-scale one here (checked)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import spcl_oracle as O
from tests.test_gpu_poolmax import _coefficients, _eighths

BF16 = torch.bfloat16
SHAPES = [(3, 14, 14), (2, 28, 28), (1, 42, 56)]
_CACHE = {}


def _mods():
    import spcl_amd  # noqa
    from spcl_amd import functional as F_, native as _n
    return F_, _n


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _inputs(N, H, W):
    F_, _n = _mods()
    dtc = _n.dtype_code(BF16)
    g = torch.Generator().manual_seed(300 + N + H + W)
    img = (torch.rand(N, H, W, generator=g) + 0.25).cuda()
    gamma = torch.randn(16, generator=g)
    gamma[::2], gamma[1::2] = gamma[::2].abs() + 0.1, -gamma[1::2].abs() - 0.1
    x = dict(img=img, wa=(torch.randn(16, 1, 3, 3, generator=g) * 0.3).cuda(), ga=gamma.cuda(),
             ba=torch.full((16,), 3.0).cuda(), wb=(torch.randn(16, 16, 3, 3, generator=g) * 0.1).cuda())
    # Conv1.a's statistics and autocorrelation rows from the statistics-only image kernel (nothing stored), then its BatchNorm
    nt = N * (H // 14) * (W // 14)
    x["wpa"], x["wpb_t"] = F_._pack(x["wa"], 0, dtc, BF16), F_._pack(x["wb"], 1, dtc, BF16)
    sa = torch.empty(_n.call("spcl_bn_stats_elems", nt, 16), dtype=torch.float32, device="cuda")
    x["acorr"] = torch.empty(nt, 64, dtype=torch.float32, device="cuda")
    _n.call("spcl_conv3x3_forward_image_acorr", _n.ptr(img), dtc, N, H, W, 1, 16, _n.ptr(x["wpa"]), None, _n.ptr(sa),
            _n.ptr(x["acorr"]), _n.stream())
    rm, rv, nbt = torch.zeros(16).cuda(), torch.ones(16).cuda(), torch.zeros((), dtype=torch.int64).cuda()
    x["sta"] = torch.empty(4, 16, dtype=torch.float32, device="cuda")
    sta = x["sta"]
    _n.call("spcl_bn_finalize", _n.ptr(sa), nt, 16, 16, _n.ptr(x["ga"]), _n.ptr(x["ba"]), ctypes.c_float(0.1),
            ctypes.c_float(1e-5), _n.ptr(rm), _n.ptr(rv), _n.ptr(nbt), _n.ptr(sta[0]), _n.ptr(sta[1]), _n.ptr(sta[2]),
            _n.ptr(sta[3]), _n.stream())
    # Conv1.b's side: its raw output, its BatchNorm's forward coefficients, the pooled gradient, per-tile rows of the sums
    y = _eighths((N, H, W, 16), g).to(BF16).cuda()
    y[0, 1, 0, 5] = float("nan")  # position (1, 0) of window (0, 0)
    y[0, 0, 1, 9] = float("nan")  # position (0, 1)
    x["y"], x["stb"] = y, _coefficients(16, g)
    x["dpool"] = torch.randn(N, H // 2, W // 2, 16, generator=g).to(BF16).cuda()
    x["nrows"] = 7
    x["rows"] = (torch.randn(x["nrows"], 2, 16, generator=g) * 40.0).cuda()
    return x


def _run(N, H, W, x, fused):
    """Conv1.b's backward on 14 x 14 tiles through the C ABI, per-tile rows and per-workgroup rows -> dict of what it leaves;
    ``fused``: the one call, else the two it replaces"""
    F_, _n = _mods()
    dtc = _n.dtype_code(BF16)
    dev = x["img"].device
    nt = N * (H // 14) * (W // 14)
    nsplit = _n.call("spcl_conv16_bwd_fused_splits", N, H, W)
    sta, stb = x["sta"], x["stb"]
    out = {}
    for wg in (False, True):
        acc = torch.zeros(_n.call("spcl_bn_acc_elems", 16), dtype=torch.int64, device=dev)
        dgamma, dbeta = torch.full((16,), 7.0, device=dev), torch.full((16,), 7.0, device=dev)
        rows11 = torch.full(((11 * 16 * nsplit) if wg else (nt * 11 * 16),), 7.0, dtype=torch.float32, device=dev)
        a16 = torch.full((16, 64), 7.0, dtype=torch.float32, device=dev)
        ws = torch.empty(nsplit * 9 * 256, dtype=torch.float32, device=dev)
        dwb = torch.full((16, 16, 3, 3), 7.0, dtype=torch.float32, device=dev)
        tail = (_n.ptr(x["wpb_t"]), _n.ptr(x["wpa"]), _n.ptr(sta[2]), _n.ptr(sta[3]), _n.ptr(sta[0]), _n.ptr(x["img"]),
                None if wg else _n.ptr(rows11), _n.ptr(ws), _n.ptr(dwb), 16, 16, _n.ptr(rows11) if wg else None,
                _n.ptr(x["acorr"]) if wg else None, nt if wg else 0, _n.ptr(a16) if wg else None, _n.stream())
        if fused:
            _n.call("spcl_conv16_bwd_fused_image_pooled", _n.ptr(x["y"]), _n.ptr(x["dpool"]), _n.ptr(x["rows"]), x["nrows"], dtc,
                    N, H, W, _n.ptr(stb), 1, _n.ptr(acc), _n.ptr(dgamma), _n.ptr(dbeta), *tail)
        else:
            dy = torch.empty(N, H, W, 16, dtype=BF16, device=dev)
            _n.call("spcl_bnrelu_backward_rows_acc", _n.ptr(x["y"]), None, _n.ptr(x["dpool"]), _n.ptr(x["rows"]), x["nrows"],
                    dtc, N, H, W, 16, 16, _n.ptr(stb), 1, _n.ptr(acc), _n.ptr(dgamma), _n.ptr(dbeta), _n.ptr(dy), _n.stream())
            _n.call("spcl_conv16_bwd_fused_image", _n.ptr(dy), dtc, N, H, W, *tail)
            out["dy"] = dy
        k = "wg_" if wg else "tile_"
        out[k + "rows"], out[k + "dwb"], out[k + "dgamma"], out[k + "dbeta"] = rows11, dwb, dgamma, dbeta
        if wg:
            out["acorr16"] = a16
    torch.cuda.synchronize()
    return out


def _pair(N, H, W):
    """the two calls and the one on the same inputs, computed once per shape and shared by the tests below"""
    if (N, H, W) not in _CACHE:
        x = _inputs(N, H, W)
        _CACHE[(N, H, W)] = (_run(N, H, W, x, False), _run(N, H, W, x, True), x)
    return _CACHE[(N, H, W)]


KEYS = [p + k for p in ("tile_", "wg_") for k in ("rows", "dwb", "dgamma", "dbeta")] + ["acorr16"]


def _same(a, b, keys):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        diff = _bits(a[k]) != _bits(b[k])
        print(k, "elements", a[k].numel(), "differing", int(diff.sum()))
        assert not bool(diff.any()), k
        assert float(torch.nan_to_num(a[k].float(), nan=0.0).abs().max()) > 0, k
        assert not bool((a[k].float() == 7.0).all()), k  # (written, not the fill)


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_one_call_against_the_two_it_replaces(N, H, W):
    """spcl_conv16_bwd_fused_image_pooled against spcl_bnrelu_backward_rows_acc -> dy -> spcl_conv16_bwd_fused_image: Conv1.b's
    weight gradient, rows11 / wg_rows, the folded autocorrelation rows, dgamma and dbeta of Conv1.b's BatchNorm"""
    _, _n = _mods()
    assert _n.call("spcl_conv16_bwd_fused_image_pooled_supported", _n.dtype_code(BF16), N, H, W, 16, 16, 1) == 1
    old, new, x = _pair(N, H, W)
    # the inputs bite: the materialised gradient carries the two NaNs and is non-zero on the image border in every channel
    # but the zero-scale one (channel 3: scale = 0 makes A = B = 0, its gradient is zero everywhere) -- a padding pixel formed
    # as A 0 + B would differ from the zero it must be
    dy = old["dy"].float()
    assert bool(torch.isnan(dy[0, 1, 0, 5])) and bool(torch.isnan(dy[0, 0, 1, 9]))
    assert int(torch.isnan(dy).sum()) == 2
    edge = torch.nan_to_num(dy[:, 0], nan=1.0).abs().amax(dim=(0, 1))
    assert float(edge[3]) == 0 and float(torch.cat([edge[:3], edge[4:]]).min()) > 0
    _same(old, new, KEYS)


def test_two_identical_calls_give_the_same_bits():
    N, H, W = SHAPES[2]
    _, new, x = _pair(N, H, W)
    again = _run(N, H, W, x, True)
    _same(new, again, KEYS)


def test_query_refuses_what_the_kernel_does_not_take():
    _, _n = _mods()
    bf, f32 = _n.dtype_code(BF16), _n.dtype_code(torch.float32)
    q = lambda *a: _n.call("spcl_conv16_bwd_fused_image_pooled_supported", *a)  # noqa: E731
    assert q(bf, 2, 126, 140, 16, 16, 1) == 1
    assert q(bf, 2, 126, 140, 16, 16, 0) == 0   # eval-mode BatchNorm
    assert q(f32, 2, 126, 140, 16, 16, 1) == 0  # f32 storage
    assert q(bf, 2, 126, 140, 32, 32, 1) == 0   # another width
    assert q(bf, 2, 30, 44, 16, 16, 1) == 0     # no multiple of 14


def _block_step(N, H, W, pooled, seed=7):
    """one forward / backward of the UNet's first two blocks through the module, dispatched like the 64 x 224^2 step (see
    test_block_through_the_switch_is_bit_identical) -> (Conv2's output, Conv1 gradients, the native calls made)"""
    F_, _n = _mods()
    from spcl_amd.semi_seg.arch import UNet
    keep, real = F_._BLOCK1_POOLED_BWD, _n.call
    calls = []

    def call(name, *a):
        # (the BatchNorm apply pass is told apart by its level: arguments 7, 8 are H, W)
        calls.append(f"{name}@{a[7]}x{a[8]}" if name == "spcl_bnrelu_backward_rows_acc" else name)
        if name in ("spcl_conv_bn_acc_supported", "spcl_conv_dgrad_poolstats_acc_supported",
                    "spcl_conv_dgrad_bnstats_acc_supported"):
            return 0
        return real(name, *a)

    F_._BLOCK1_POOLED_BWD, _n.call = pooled, call
    try:
        m = UNet(input_dim=1, num_classes=4, max_channel=256)
        sd = O.init_unet_state(1, 4, 256, seed=seed)
        g = torch.Generator().manual_seed(seed)
        gam = torch.randn(16, generator=g)
        gam[::2], gam[1::2] = gam[::2].abs() + 0.1, -gam[1::2].abs() - 0.1
        sd["_Conv1.conv.1.weight"], sd["_Conv1.conv.1.bias"] = gam, torch.full((16,), 3.0)
        m.load_state_dict(sd, strict=True)
        m.cuda().train()
        m.set_compute_dtype(BF16)
        x = torch.rand(N, 1, H, W, generator=g) + 0.25
        y = m(x.cuda(), until="Conv2")
        r = torch.randn(y.shape, generator=g)
        (y.float() * r.cuda()).sum().backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if n.startswith("_Conv1")}
        return y.detach().clone(), grads, calls
    finally:
        F_._BLOCK1_POOLED_BWD, _n.call = keep, real


def test_block_through_the_switch_is_bit_identical():
    """functional._BLOCK1_POOLED_BWD on / off at 2 x 126 x 140 (the shape of tests/test_gpu_block1_recompute.py's switch test),
    Conv1 -> pool -> Conv2 with a random gradient on Conv2's output: the output, every Conv1 gradient (both convolutions'
    weights, both BatchNorms' gamma / beta) identical; with the switch on the new entry ran and no
    spcl_bnrelu_backward_rows_acc was called for block 1.
    The block is dispatched as in the 64 x 224^2 step, where block 1 has 16 384 tiles: there the BatchNorm sums of blocks 1 and
    2 travel as per-tile rows (more tiles than an accumulator block takes adds from), which is what the recomputation and the
    pooled entry are offered for.  At this size the library would pick the accumulator-block forms, so the three queries
    that decide it answer 0 for the duration of the step."""
    N, H, W = 2, 126, 140
    y1, g1, c1 = _block_step(N, H, W, True)
    y0, g0, c0 = _block_step(N, H, W, False)
    assert c1.count("spcl_conv16_bwd_fused_image_pooled") == 1 and "spcl_conv16_bwd_fused_image" not in c1
    assert f"spcl_bnrelu_backward_rows_acc@{H}x{W}" not in c1
    assert c0.count(f"spcl_bnrelu_backward_rows_acc@{H}x{W}") == 1 and c0.count("spcl_conv16_bwd_fused_image") == 1
    assert "spcl_conv16_bwd_fused_image_pooled" not in c0
    assert torch.equal(_bits(y0), _bits(y1))
    assert sorted(g0) == sorted(g1) and len(g0) == 6
    for k in g0:
        assert torch.equal(_bits(g0[k]), _bits(g1[k])), k
        assert bool(torch.isfinite(g0[k]).all()) and float(g0[k].abs().max()) > 0, k


def test_a_size_that_is_no_multiple_of_14_keeps_the_old_calls():
    """2 x 30 x 44: the query says no; the block runs the launches it ran before (switch on) and never the new entry"""
    F_, _n = _mods()
    N, H, W = 2, 30, 44
    assert _n.call("spcl_conv16_bwd_fused_image_pooled_supported", _n.dtype_code(BF16), N, H, W, 16, 16, 1) == 0
    y1, g1, c1 = _block_step(N, H, W, True)
    y0, g0, c0 = _block_step(N, H, W, False)
    assert "spcl_conv16_bwd_fused_image_pooled" not in c1
    assert [c for c in c1 if not c.endswith("_supported")] == [c for c in c0 if not c.endswith("_supported")]
    assert torch.equal(_bits(y0), _bits(y1))
    for k in g0:
        assert torch.equal(_bits(g0[k]), _bits(g1[k])) and float(g0[k].abs().max()) > 0, k
