"""The image block without its first convolution's raw output (semi_seg/arch/unet.py:123 -> :72-75 of the reference): the
tensor between Conv1.a and Conv1.b is never stored; the statistics-only image kernel leaves the BatchNorm / autocorrelation
rows, Conv1.b's loader and the one-pass backward form the tensor again per tile from the image (csrc/conv_fast.hip MODE 8,
csrc/conv16_bwd.hip RECOMP).  Everything is compared with the stored-tensor path on the same inputs with torch.equal: the
recomputation uses the image kernel's instruction, operands and rounding, so no bit may move.

Shapes (N, H, W): 3 x 14 x 14 one tile whose whole halo is outside the image, odd batch; 2 x 28 x 28 every tile touches a
border; 1 x 42 x 56 interior tiles and all four edges; 2 x 30 x 44 no multiple of 14 (refused; the stored path runs).
Inputs: images that are non-zero on the border rows / columns, Conv1.a's BatchNorm with beta = 3 and gamma of mixed sign, so
that a padded halo pixel evaluated as relu(shift) instead of 0 moves the output (the trap csrc/discr.hip's notes describe).

The library's own dispatch runs these kernels above 112 rows only (14-row tiles; spcl_block1_recompute_supported); the entry
points take every whole-tile size, and their stored-tensor forms run the SAME kernels on the same 14 x 14 tiles, which is what
makes the statistics rows comparable bit for bit at the small shapes (spcl_block1_kernels_take says where they may be
called).  The switch functional._BLOCK1_RECOMPUTE is exercised
at 2 x 126 x 140, the smallest whole-tile size above that threshold (9 x 10 tiles: no multiple of 8, no XCD remap)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import spcl_oracle as O

SHAPES = [(3, 14, 14), (2, 28, 28), (1, 42, 56)]
_CACHE = {}


def _mods():
    import spcl_amd  # noqa
    from spcl_amd import functional as F_, native as _n
    return F_, _n


def _inputs(N, H, W):
    g = torch.Generator().manual_seed(100 + N + H + W)
    img = (torch.rand(N, H, W, generator=g) + 0.25).cuda()  # (>= 0.25 everywhere: the border rows / columns too)
    assert float(img[:, 0].min()) > 0 and float(img[:, -1].min()) > 0 and float(img[:, :, 0].min()) > 0
    gamma = torch.randn(16, generator=g)
    gamma[::2], gamma[1::2] = gamma[::2].abs() + 0.1, -gamma[1::2].abs() - 0.1  # mixed sign
    return dict(img=img, wa=(torch.randn(16, 1, 3, 3, generator=g) * 0.3).cuda(), ga=gamma.cuda(),
                ba=torch.full((16,), 3.0).cuda(), wb=(torch.randn(16, 16, 3, 3, generator=g) * 0.1).cuda(),
                dy=torch.randn(N, H, W, 16, generator=g).cuda().bfloat16())


def _run(N, H, W, x, stored):
    """the block's launches on 14 x 14 tiles through the C ABI -> dict of every tensor they leave"""
    F_, _n = _mods()
    bf, dev = torch.bfloat16, x["img"].device
    dtc = _n.dtype_code(bf)
    nt = N * (H // 14) * (W // 14)
    wpa, wpb, wpb_t = F_._pack(x["wa"], 0, dtc, bf), F_._pack(x["wb"], 0, dtc, bf), F_._pack(x["wb"], 1, dtc, bf)
    out = {}
    # ---- Conv1.a: statistics rows + autocorrelation rows (+ the tensor itself on the stored path)
    y1a = torch.empty(N, H, W, 16, dtype=bf, device=dev) if stored else None
    sa = torch.empty(_n.call("spcl_bn_stats_elems", nt, 16), dtype=torch.float32, device=dev)
    acorr = torch.empty(nt, 64, dtype=torch.float32, device=dev)
    _n.call("spcl_conv3x3_forward_image_acorr", _n.ptr(x["img"]), dtc, N, H, W, 1, 16, _n.ptr(wpa), _n.ptr(y1a), _n.ptr(sa),
            _n.ptr(acorr), _n.stream())
    out["stats_a"], out["acorr"] = sa[:nt * 48].clone(), acorr
    rm, rv, nbt = torch.zeros(16, device=dev), torch.ones(16, device=dev), torch.zeros((), dtype=torch.int64, device=dev)
    sta = torch.empty(4, 16, dtype=torch.float32, device=dev)
    _n.call("spcl_bn_finalize", _n.ptr(sa), nt, 16, 16, _n.ptr(x["ga"]), _n.ptr(x["ba"]), ctypes.c_float(0.1),
            ctypes.c_float(1e-5), _n.ptr(rm), _n.ptr(rv), _n.ptr(nbt), _n.ptr(sta[0]), _n.ptr(sta[1]), _n.ptr(sta[2]),
            _n.ptr(sta[3]), _n.stream())
    out["sta"], out["running_mean"], out["running_var"] = sta, rm, rv
    # ---- Conv1.b forward
    y1b, sb = F_._conv_from_image(x["img"], y1a, dtc, bf, N, H, W, 16, wpa, sta[2], sta[3], wpb, True)
    assert sb.ntiles == nt
    out["y1b"], out["stats_b"] = y1b, sb[:nt * 48].clone()
    # ---- backward of Conv1.b in one pass, per-tile rows and per-workgroup rows; Conv1.a's gradients from either
    nsplit = _n.call("spcl_conv16_bwd_fused_splits", N, H, W)
    name = "spcl_conv16_bwd_fused" if stored else "spcl_conv16_bwd_fused_image"
    for wg in (False, True):
        rows = torch.empty((11 * 16 * nsplit) if wg else (nt * 11 * 16), dtype=torch.float32, device=dev)
        rows.wg, rows.ntiles = (nsplit if wg else 0), nt
        a16 = torch.empty(16, 64, dtype=torch.float32, device=dev)
        rows.acorr16 = a16
        ws = torch.empty(nsplit * 9 * 256, dtype=torch.float32, device=dev)
        dwb = torch.empty(16, 16, 3, 3, dtype=torch.float32, device=dev)
        _n.call(name, _n.ptr(x["dy"]), dtc, N, H, W, _n.ptr(wpb_t), _n.ptr(y1a if stored else wpa), _n.ptr(sta[2]),
                _n.ptr(sta[3]), _n.ptr(sta[0]), _n.ptr(x["img"]), None if wg else _n.ptr(rows), _n.ptr(ws), _n.ptr(dwb), 16, 16,
                _n.ptr(rows) if wg else None, _n.ptr(acorr) if wg else None, nt if wg else 0, _n.ptr(a16) if wg else None,
                _n.stream())
        dwa, dga, dba = F_._bnrelu_bwd_rows_image3(rows, acorr, x["wa"], N, H, W, 16, 16, sta, True, (None, None, None))
        k = "wg_" if wg else "tile_"
        out[k + "rows"], out[k + "dwb"], out[k + "dwa"], out[k + "dga"], out[k + "dba"] = rows, dwb, dwa, dga, dba
        if wg:
            out["acorr16"] = a16
    torch.cuda.synchronize()
    return out


def _pair(N, H, W):
    """both paths on one set of inputs, computed once per shape and shared by the tests below"""
    if (N, H, W) not in _CACHE:
        x = _inputs(N, H, W)
        _CACHE[(N, H, W)] = (_run(N, H, W, x, True), _run(N, H, W, x, False), x)
    return _CACHE[(N, H, W)]


def _same(a, b, keys):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert torch.equal(a[k].view(torch.int16 if a[k].dtype == torch.bfloat16 else torch.int32),
                           b[k].view(torch.int16 if b[k].dtype == torch.bfloat16 else torch.int32)), k
        assert bool(torch.isfinite(a[k].float()).all()) and float(a[k].float().abs().max()) > 0, k


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_statistics_only_image_kernel_leaves_the_same_rows(N, H, W):
    """conv3x3_image_kernel<.., STORE = false>: BatchNorm partial rows and autocorrelation rows bit for bit those of the
    writing kernel, hence scale / shift and the running statistics"""
    old, new, _ = _pair(N, H, W)
    _same(old, new, ["stats_a", "acorr", "sta", "running_mean", "running_var"])


def test_statistics_only_kernel_walking_several_images():
    """The statistics-only image kernel lets a workgroup walk ipw = ceil(tiles / 4096) images at its tile position, the next
    image's halo requested ahead -- 1 at the shapes above.  65 x 112 x 112: 4 160 tiles -> ipw = 2, 33 workgroups per tile
    position of which the last walks ONE image (N % ipw != 0); 64 tiles per image, a multiple of 8, so the XCD remap runs
    with the walk.  Statistics and autocorrelation rows of every tile bit for bit those of the writing kernel (one image per
    workgroup), twice."""
    F_, _n = _mods()
    N, H, W = 65, 112, 112
    bf = torch.bfloat16
    dtc = _n.dtype_code(bf)
    assert _n.call("spcl_block1_kernels_take", dtc, N, H, W, 1, 16) == 1
    assert _n.call("spcl_conv3x3_forward_image_acorr_rows", dtc, N, H, W, 1, 16) == 0  # (the library's dispatch: 7-row tiles)
    nt = N * (H // 14) * (W // 14)
    assert nt == 4160 and (H // 14) * (W // 14) % 8 == 0
    g = torch.Generator().manual_seed(65)
    img = (torch.rand(N, H, W, generator=g) + 0.25).cuda()
    wpa = F_._pack((torch.randn(16, 1, 3, 3, generator=g) * 0.3).cuda(), 0, dtc, bf)
    res = []
    for stored in (True, False, False):
        y = torch.empty(N, H, W, 16, dtype=bf, device=img.device) if stored else None
        sa = torch.zeros(_n.call("spcl_bn_stats_elems", nt, 16), dtype=torch.float32, device=img.device)
        acorr = torch.zeros(nt, 64, dtype=torch.float32, device=img.device)
        _n.call("spcl_conv3x3_forward_image_acorr", _n.ptr(img), dtc, N, H, W, 1, 16, _n.ptr(wpa), _n.ptr(y), _n.ptr(sa),
                _n.ptr(acorr), _n.stream())
        res.append({"stats_a": sa[:nt * 48].clone(), "acorr": acorr})
    torch.cuda.synchronize()
    _same(res[0], res[1], ["stats_a", "acorr"])
    _same(res[1], res[2], ["stats_a", "acorr"])
    # every tile of every image was written, the last (odd) image's too
    assert float(res[1]["stats_a"].view(N, -1, 48)[:, :, :16].min()) == 196.0
    assert float(res[1]["acorr"].view(N, -1, 64)[:, :, 45].min()) > 0


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_conv1b_forward_from_the_image(N, H, W):
    """conv3x3_fast_kernel MODE 8 against MODE 1 on the stored tensor: y1b and its statistics rows.  beta = 3: a halo pixel
    outside the image evaluated as relu(shift) = 3 instead of 0 would move every border pixel of y1b (checked: the border
    differs from what a shift-padded input gives)."""
    old, new, x = _pair(N, H, W)
    _same(old, new, ["y1b", "stats_b"])
    # the padded activation is zero: against fp64 math on the kernel's own rounded operands, all border pixels included
    sta = old["sta"].double().cpu()
    y1a = torch.nn.functional.conv2d(x["img"].bfloat16().double().cpu()[:, None], x["wa"].bfloat16().double().cpu(), padding=1)
    act = torch.relu(y1a.bfloat16().double() * sta[2][None, :, None, None] + sta[3][None, :, None, None]).bfloat16().double()
    want = torch.nn.functional.conv2d(act, x["wb"].bfloat16().double().cpu(), padding=1)
    got = new["y1b"].double().cpu().permute(0, 3, 1, 2)
    # bf16 storage of y1b (2^-9 relative) + a few ReLU / rounding-boundary flips of the bf16 activations upstream
    err = float((got - want).abs().max() / want.abs().max())
    assert err < 2e-2, err
    padded = torch.relu(sta[3]).bfloat16().double()[None, :, None, None].expand(N, 16, H + 2, W + 2).clone()
    padded[:, :, 1:-1, 1:-1] = act  # (what relu(shift) in the padding would give)
    wrong = torch.nn.functional.conv2d(padded, x["wb"].bfloat16().double().cpu())
    assert float((wrong - want).abs().max() / want.abs().max()) > 10 * err


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_one_pass_backward_from_the_image(N, H, W):
    """conv16_bwd_rows_kernel<.., RECOMP> against the kernel reading the stored tensor, random upstream gradient: Conv1.b's
    weight gradient, the rows11 / wg_rows sums, the folded autocorrelation rows, and Conv1.a's dW, dgamma, dbeta from them"""
    old, new, _ = _pair(N, H, W)
    _same(old, new, [p + k for p in ("tile_", "wg_") for k in ("rows", "dwb", "dwa", "dga", "dba")] + ["acorr16"])


def test_two_identical_calls_give_the_same_bits():
    N, H, W = SHAPES[2]
    _, new, x = _pair(N, H, W)
    again = _run(N, H, W, x, False)
    _same(new, again, [k for k in new])


def _block_step(N, H, W, recompute, dtype=torch.bfloat16, seed=7):
    """one forward / backward of the UNet's first block through the module -> (output, Conv1 gradients, running statistics)"""
    F_, _n = _mods()
    from spcl_amd.semi_seg.arch import UNet
    keep = (F_._BLOCK1_RECOMPUTE, F_._BN_ACC)
    # (rows + finalize on both BatchNorms, as the 64 x 224^2 step has them: with few tiles Conv1.b's statistics would go through
    # an accumulator block, a form the recomputation is not offered for)
    F_._BLOCK1_RECOMPUTE, F_._BN_ACC = recompute, False
    try:
        m = UNet(input_dim=1, num_classes=4, max_channel=256)
        sd = O.init_unet_state(1, 4, 256, seed=seed)
        g = torch.Generator().manual_seed(seed)
        gam = torch.randn(16, generator=g)
        gam[::2], gam[1::2] = gam[::2].abs() + 0.1, -gam[1::2].abs() - 0.1
        sd["_Conv1.conv.1.weight"], sd["_Conv1.conv.1.bias"] = gam, torch.full((16,), 3.0)
        m.load_state_dict(sd, strict=True)
        m.cuda().train()
        m.set_compute_dtype(dtype)
        x = torch.rand(N, 1, H, W, generator=g) + 0.25
        y = m(x.cuda(), until="Conv1")
        r = torch.randn(y.shape, generator=g)
        (y.float() * r.cuda()).sum().backward()
        torch.cuda.synchronize()
        c1 = m._Conv1.conv
        grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if n.startswith("_Conv1")}
        run = {"mean_a": c1[1].running_mean.clone(), "var_a": c1[1].running_var.clone(),
               "mean_b": c1[4].running_mean.clone(), "var_b": c1[4].running_var.clone()}
        return y.detach().clone(), grads, run, sd, x, r
    finally:
        F_._BLOCK1_RECOMPUTE, F_._BN_ACC = keep


def test_block_through_the_switch_is_bit_identical():
    """functional._BLOCK1_RECOMPUTE on / off at 2 x 126 x 140: the block's output, every Conv1 gradient and the running
    statistics of both BatchNorms; and the recomputing path really ran (no tensor between the two convolutions was saved)"""
    F_, _n = _mods()
    N, H, W = 2, 126, 140
    assert _n.call("spcl_block1_recompute_supported", _n.dtype_code(torch.bfloat16), N, H, W, 1, 16) == 1
    assert _n.call("spcl_block1_recompute_supported", _n.dtype_code(torch.float32), N, H, W, 1, 16) == 0  # f32 storage
    assert _n.call("spcl_block1_recompute_supported", _n.dtype_code(torch.bfloat16), N, 112, 112, 1, 16) == 0  # 7-row tiles
    calls = []
    real = F_._conv_from_image
    F_._conv_from_image = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        y1, g1, r1 = _block_step(N, H, W, True)[:3]
        assert calls == [1]
        y0, g0, r0 = _block_step(N, H, W, False)[:3]
        assert calls == [1]
    finally:
        F_._conv_from_image = real
    assert torch.equal(y0, y1)
    assert sorted(g0) == sorted(g1) and len(g0) == 6
    for k in g0:
        assert torch.equal(g0[k], g1[k]) and float(g0[k].abs().max()) > 0, k
    for k in r0:
        assert torch.equal(r0[k], r1[k]), k


def test_a_size_that_is_no_multiple_of_14_keeps_the_stored_path():
    """2 x 30 x 44: spcl_block1_recompute_supported says no, the block runs as before (switch on) and still matches the bf16
    emulating oracle at the bars of tests/test_gpu_encoder.py::test_block_bf16_vs_bf16_emulating_oracle: 5e-3 relative L2 on
    the block output, 6e-2 on the gradients"""
    F_, _n = _mods()
    N, H, W = 2, 30, 44
    dtc = _n.dtype_code(torch.bfloat16)
    assert _n.call("spcl_block1_recompute_supported", dtc, N, H, W, 1, 16) == 0
    assert _n.call("spcl_block1_kernels_take", dtc, N, H, W, 1, 16) == 0
    calls = []
    real = F_._conv_from_image
    F_._conv_from_image = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        y, grads, _, sd, x, r = _block_step(N, H, W, True)
    finally:
        F_._conv_from_image = real
    assert calls == []
    sdo = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.clone())
           for k, v in sd.items()}
    yr = O.encoder_forward(x, sdo, "Conv1", q=O.BF16Emulation)
    (yr * r).sum().backward()
    rel = lambda a, b: float(np.linalg.norm(a.astype(np.float64) - b) / max(1e-30, np.linalg.norm(b)))  # noqa: E731
    assert rel(y.float().cpu().numpy(), yr.detach().numpy()) < 5e-3
    for name, gr in grads.items():
        e = rel(gr.float().cpu().numpy(), sdo[name].grad.numpy())
        assert e < 6e-2, (name, e)
