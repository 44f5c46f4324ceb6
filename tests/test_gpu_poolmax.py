"""The pooled boundary through the window-maximum tensor (reference semi_seg/arch/unet.py:74-77,118-121: BatchNorm + ReLU +
nn.MaxPool2d(2) between two encoder blocks, and autograd's backward through them).

The pooled forward leaves, per 2x2 window and channel, the raw convolution output ``y`` at the window's first maximum of
``fma(scale, y, shift)`` (spcl_bnrelu_pool_forward_ymax); the next block's input-gradient kernel reads that tensor instead of
the full-resolution ``y`` (spcl_conv3x3_dgrad_poolmax[_acc]).  Nothing is approximated: every comparison here is bit for bit."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_kernels import _n, nhwc, pack  # noqa: E402

BF16 = torch.bfloat16


def _eighths(shape, g):
    """values k / 8, |k| <= 32: exact in bf16, many equal neighbours (tied window maxima)"""
    return torch.randint(-32, 33, shape, generator=g).float() / 8.0


def _coefficients(C, g):
    """[4][C] (mean, invstd, scale, shift) with the cases the selection rule must get right: negative gamma (the arg-max is the
    raw minimum), a channel with scale == 0 (every position ties: the first wins), a channel that is non-positive everywhere"""
    st = torch.zeros(4, C)
    st[0] = torch.randn(C, generator=g) * 0.1 + 0.2
    st[1] = torch.rand(C, generator=g) + 0.5
    st[2] = st[1] * (torch.rand(C, generator=g) + 0.5)
    st[2][::5] *= -1.0
    st[3] = torch.randn(C, generator=g) * 0.2 - st[0] * st[2]
    st[2][3], st[3][3] = 0.0, 0.25     # scale == 0, positive everywhere
    st[3][7] = -100.0                  # all windows non-positive after BN
    return st.cuda()


def _first_max_reference(y, scale, shift):
    """[N][H/2][W/2][C]: y at the first maximum of fma(scale, y, shift) over each complete window, scan order (0,0) (0,1) (1,0)
    (1,1); a position takes over only when strictly larger (so a NaN behind the first position never does)"""
    N, H, W, C = y.shape
    OH, OW = H // 2, W // 2
    yw = y[:, :2 * OH, :2 * OW].reshape(N, OH, 2, OW, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(N, OH, OW, C, 4)
    yf = yw.float()
    z = torch.addcmul(shift.view(1, 1, 1, C, 1).expand_as(yf), yf, scale.view(1, 1, 1, C, 1).expand_as(yf))
    zb, yb = z[..., 0], yw[..., 0]
    for k in range(1, 4):
        m = z[..., k] > zb
        zb = torch.where(m, z[..., k], zb)
        yb = torch.where(m, yw[..., k], yb)
    return yb.contiguous()


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _pool_ymax(n, y, dtc, scale, shift, bn=None, act=None):
    N, H, W, C = y.shape
    pool = torch.full((N, H // 2, W // 2, C), 7.0, dtype=y.dtype, device="cuda")
    ymax = torch.full_like(pool, 7.0)
    n.call("spcl_bnrelu_pool_forward_ymax", n.ptr(y), dtc, N, H, W, C, n.ptr(scale), n.ptr(shift),
           ctypes.byref(bn) if bn is not None else None, n.ptr(act), n.ptr(pool), n.ptr(ymax), n.stream())
    return pool, ymax


# even sizes (the whole-window kernel), odd H, odd W, both odd (windows cut by the edge produce nothing), every channel-chunk count
FWD_SHAPES = [(2, 16, 28, 28, BF16), (1, 32, 9, 11, BF16), (2, 64, 6, 7, BF16), (1, 128, 7, 6, BF16), (1, 256, 4, 4, BF16),
              (1, 16, 6, 4, torch.float32), (1, 16, 5, 7, torch.float32)]


@pytest.mark.parametrize("N,C,H,W,dtype", FWD_SHAPES)
@pytest.mark.parametrize("with_act", [False, True])
def test_forward_side_output_is_the_first_maximum_and_changes_nothing_else(N, C, H, W, dtype, with_act):
    n = _n()
    dtc = n.dtype_code(dtype)
    g = torch.Generator().manual_seed(C + H + 3 * W)
    y = _eighths((N, H, W, C), g).to(dtype).cuda()
    y[0, 1, 0, 5] = float("nan")  # position (1, 0) of window (0, 0)
    y[0, 0, 1, 9] = float("nan")  # position (0, 1)
    st = _coefficients(C, g)
    act0 = torch.full((N, H, W, C), 7.0, dtype=dtype, device="cuda") if with_act else None
    act1 = act0.clone() if with_act else None
    pool0 = torch.full((N, H // 2, W // 2, C), 7.0, dtype=dtype, device="cuda")
    n.call("spcl_bnrelu_pool_forward", n.ptr(y), dtc, N, H, W, C, n.ptr(st[2]), n.ptr(st[3]), n.ptr(act0), n.ptr(pool0),
           n.stream())
    pool1, ymax = _pool_ymax(n, y, dtc, st[2], st[3], act=act1)
    assert torch.equal(_bits(pool1), _bits(pool0))
    if with_act:
        assert torch.equal(_bits(act1), _bits(act0))
    ref = _first_max_reference(y, st[2], st[3])
    assert not bool(torch.isnan(ref.float()).any())
    assert torch.equal(_bits(ymax), _bits(ref))


@pytest.mark.parametrize("view", [(1, 56, 56), (1, 49, 64), (1, 64, 49)])
def test_forward_side_output_with_coefficients_from_an_accumulator_block(view):
    """the same through the accumulator-block prologue (spcl_bn_acc): a convolution leaves y and its statistics block, the pooled
    forward derives scale / shift from it -- with and without the side output; the odd views re-read the same pixels as an
    image with an odd height / width (the statistics are those of all pixels either way)"""
    n = _n()
    dtc, ci, C = 1, 32, 64
    assert n.call("spcl_conv_bn_acc_supported", dtc, 1, 56, 56, ci, C, 0, 1)
    g = torch.Generator().manual_seed(11)
    xs = nhwc(torch.randn(1, ci, 56, 56, generator=g) + 0.3, BF16)
    wp = pack(n, torch.randn(C, ci, 3, 3, generator=g) / (3 * ci ** 0.5), 0, BF16)
    acc = torch.zeros(n.call("spcl_bn_acc_elems", C), dtype=torch.int64, device="cuda")
    y = torch.empty(1, 56, 56, C, dtype=BF16, device="cuda")
    n.call("spcl_conv3x3_forward_acc", n.ptr(xs), dtc, 1, 56, 56, ci, C, n.ptr(wp), None, None, None, n.ptr(y), n.ptr(acc), None,
           n.stream())
    N, H, W = view
    y = y.view(N, H, W, C)
    gamma = (torch.rand(C, generator=g) + 0.5).cuda()
    gamma[::5] *= -1.0
    beta = (torch.randn(C, generator=g) * 0.2).cuda()

    def desc(block, st):
        return n.BnAcc(block.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None, None, None, st.data_ptr(), 0.1, 1e-5,
                       float(N * H * W), C, C)

    st0, st1 = torch.zeros(4, C, device="cuda"), torch.zeros(4, C, device="cuda")
    a0, a1 = acc.clone(), acc.clone()
    pool0 = torch.full((N, H // 2, W // 2, C), 7.0, dtype=BF16, device="cuda")
    d0 = desc(a0, st0)
    n.call("spcl_bnrelu_pool_forward_acc", n.ptr(y), dtc, N, H, W, C, ctypes.byref(d0), None, n.ptr(pool0), n.stream())
    pool1, ymax = _pool_ymax(n, y, dtc, None, None, bn=desc(a1, st1))
    assert torch.equal(st1, st0)
    assert torch.equal(_bits(pool1), _bits(pool0))
    assert torch.equal(_bits(ymax), _bits(_first_max_reference(y, st1[2], st1[3])))


PAIRS = [(32, 16), (64, 32), (128, 64), (256, 128)]  # (channels of the incoming gradient, channels of the pooled block)


# pooled sizes: one tile row pair; several tiles; 21 x 21; a height that is no multiple of the 7-row tile (last tile row shifted
# back: the `keep` factor by rows); a width that is no multiple of the 14-column tile (the same by columns)
SIZES = [(14, 14), (28, 28), (21, 21), (20, 28), (35, 35)]


@pytest.mark.parametrize("co,ci", PAIRS)
@pytest.mark.parametrize("H,W", SIZES)
def test_dgrad_through_the_window_maxima_leaves_the_bits_of_the_full_tensor_form(co, ci, H, W):
    """spcl_conv3x3_dgrad_poolmax[_acc] against spcl_conv3x3_dgrad_poolstats[_acc] on the same inputs: g, the rows and the
    block's words bit for bit.  At 21 x 21 the full-tensor form does not exist (no 14-column specialisation is picked at that
    width, spcl_conv_dgrad_poolstats_supported == 0): there the new form must refuse as well; the shifted-tile paths that size
    was meant for are covered by 20 x 28 and 35 x 35."""
    n = _n()
    dtc, N = 1, 2
    H2, W2 = 2 * H, 2 * W
    if (H, W) == (21, 21):
        assert not n.call("spcl_conv_dgrad_poolstats_supported", dtc, N, H, W, co, ci, H2, W2)
        assert not n.call("spcl_conv_dgrad_poolmax_supported", dtc, N, H, W, co, ci)
        assert not n.call("spcl_conv_dgrad_poolmax_acc_supported", dtc, N, H, W, co, ci)
        return
    assert n.call("spcl_conv_dgrad_poolstats_supported", dtc, N, H, W, co, ci, H2, W2)
    assert n.call("spcl_conv_dgrad_poolmax_supported", dtc, N, H, W, co, ci)
    g = torch.Generator().manual_seed(co + H)
    dy = nhwc((torch.randn(N, co, H, W, generator=g) * 1e-2).to(BF16).float(), BF16)
    y2 = torch.randint(-3, 4, (N, H2, W2, ci), generator=g).to(BF16).cuda()  # small integers: tied maxima in most windows
    y2[0, 1, 4, 5] = float("nan")   # position (1, 0) of its window
    y2[1, 6, 3, 9] = float("nan")   # position (0, 1)
    wp_t = pack(n, torch.randn(co, ci, 3, 3, generator=g) / (3.0 * co ** 0.5), 1, BF16)
    st = _coefficients(ci, g)
    _, ymax = _pool_ymax(n, y2, dtc, st[2], st[3])
    nt = n.call("spcl_conv_stat_rows", dtc, N, H, W, co, ci)
    g0, g1 = (torch.full((N, H, W, ci), 7.0, dtype=BF16, device="cuda") for _ in range(2))
    r0, r1 = (torch.full((nt * 2 * ci,), 7.0, device="cuda") for _ in range(2))
    n.call("spcl_conv3x3_dgrad_poolstats", n.ptr(dy), dtc, N, H, W, co, ci, n.ptr(wp_t), n.ptr(g0), n.ptr(y2), H2, W2,
           n.ptr(st[2]), n.ptr(st[3]), n.ptr(st[0]), n.ptr(r0), n.stream())
    n.call("spcl_conv3x3_dgrad_poolmax", n.ptr(dy), dtc, N, H, W, co, ci, n.ptr(wp_t), n.ptr(g1), n.ptr(ymax),
           n.ptr(st[2]), n.ptr(st[3]), n.ptr(st[0]), n.ptr(r1), n.stream())
    assert torch.equal(_bits(g1), _bits(g0))
    assert not bool(torch.isnan(r0).any()) and float(r0.abs().max()) > 0
    assert torch.equal(r1, r0)
    has_acc = n.call("spcl_conv_dgrad_poolstats_acc_supported", dtc, N, H, W, co, ci, H2, W2)
    assert n.call("spcl_conv_dgrad_poolmax_acc_supported", dtc, N, H, W, co, ci) == has_acc
    if has_acc:
        b0, b1 = (torch.zeros(n.call("spcl_bn_acc_elems", ci), dtype=torch.int64, device="cuda") for _ in range(2))
        g2, g3 = torch.empty_like(g0), torch.empty_like(g0)
        n.call("spcl_conv3x3_dgrad_poolstats_acc", n.ptr(dy), dtc, N, H, W, co, ci, n.ptr(wp_t), n.ptr(g2), n.ptr(y2), H2, W2,
               n.ptr(st[2]), n.ptr(st[3]), n.ptr(st[0]), n.ptr(b0), n.stream())
        n.call("spcl_conv3x3_dgrad_poolmax_acc", n.ptr(dy), dtc, N, H, W, co, ci, n.ptr(wp_t), n.ptr(g3), n.ptr(ymax),
               n.ptr(st[2]), n.ptr(st[3]), n.ptr(st[0]), n.ptr(b1), n.stream())
        assert torch.equal(_bits(g2), _bits(g0)) and torch.equal(_bits(g3), _bits(g0))
        assert bool((b0 != 0).any()) and torch.equal(b1, b0)


def test_two_blocks_train_to_the_same_bits_with_and_without_the_window_maxima(monkeypatch):
    """two linked encoder blocks, forward and backward: with the side tensor the consumer's dgrad runs the window-maximum form,
    without it the full-tensor form; every parameter gradient is the same bits.  Eval and no-grad forwards never ask for it."""
    import spcl_amd  # noqa
    from spcl_amd import functional as F
    from spcl_amd.semi_seg.arch.unet import _ConvBlock
    torch.manual_seed(7)
    a = _ConvBlock(16, 32).cuda().train()
    b = _ConvBlock(32, 64).cuda().train()
    for m in (a, b):
        m._compute_dtype = BF16
    x = torch.rand(4, 16, 56, 56, device="cuda").bfloat16().contiguous(memory_format=torch.channels_last)

    def run(pays, backward=True):
        monkeypatch.setattr(F, "_pool_ymax_pays", lambda *shape: pays)
        for m in (a, b):
            m.zero_grad(set_to_none=True)
        used = []
        real = F._n.call
        monkeypatch.setattr(F._n, "call", lambda name, *args: (used.append(name), real(name, *args))[1])
        a._plan = (False, True)
        a(x)
        p = a.take_pooled()
        b._plan = (True, False)
        b._link_in, a._link_out = a._link_out, None
        o = b(p)
        if backward:
            o.float().square().mean().backward()
        torch.cuda.synchronize()
        monkeypatch.setattr(F._n, "call", real)
        return [q.grad.clone() for m in (a, b) for q in m.parameters()] if backward else None, used

    g1, used1 = run(True)
    g0, used0 = run(False)
    assert "spcl_bnrelu_pool_forward_ymax" in used1 and any(u.startswith("spcl_conv3x3_dgrad_poolmax") for u in used1)
    assert not any("ymax" in u or "poolmax" in u for u in used0)
    assert any(u.startswith("spcl_conv3x3_dgrad_poolstats") for u in used0)
    assert len(g1) == len(g0) > 0
    for u, v in zip(g1, g0):
        assert torch.equal(u, v)
    for m in (a, b):
        m.eval()
    with torch.no_grad():
        _, used_eval = run(True, backward=False)
    assert not any("ymax" in u for u in used_eval)
    for m in (a, b):
        m.train()
    with torch.no_grad():
        _, used_nograd = run(True, backward=False)
    assert not any("ymax" in u for u in used_nograd)
