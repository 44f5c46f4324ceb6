"""The eval-mode pass -- the one every reported Dice, loss and surface distance comes from -- against float64, on weights
whose running statistics are real (tests/_eval_oracle.py): the coefficient kernels (spcl_bn_eval_affine, its multi-layer
form, spcl_rows_bn_eval_affine), the float32 network stage by stage, the bf16 network stage by stage with teacher forcing,
``EvalEpocher`` and the eval branch (`training = 0`) of the BatchNorm backward, at kernel and at network level.

Every bar is the float32 CPU oracle's own distance from float64 on the same numbers (times a stated margin), a number
format's precision, or a bar the project already holds elsewhere; none is taken from what the kernels return.  The figures
measured on an MI355X are in docs/eval_parity.md (tools/eval_parity_collect.py)."""
from contextlib import contextmanager
from ctypes import c_float

import pytest
import torch
import torch.nn.functional as TF

pytestmark = pytest.mark.gpu

from oracle import spcl_oracle as O  # noqa: E402
from tests import _eval_oracle as E  # noqa: E402
from tests.test_gpu_kernels import _n, nhwc, rnd, ru16  # noqa: E402

SENTINEL = -12345.5
EPS = 1e-5
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))  # what the kernels are handed (c_float)


# ----------------------------------------------------------------------------------------------------------------------
# a. the coefficient kernels
def _layer(C, seed):
    """gamma (every 5th negative), beta, running_mean (|.| up to 1e3), running_var (0, 1e-12, 1e-3, 1e4 among ordinary ones) of
    one BatchNorm.  beta takes the sign of -running_mean * gamma: shift = beta - running_mean * scale then adds two terms of
    one sign, and a RELATIVE bar on it is a bar on the kernel's arithmetic (where they cancel it is a bar on luck)."""
    g = torch.Generator().manual_seed(seed)
    gamma = 0.5 + torch.rand(C, generator=g)
    gamma[::5] *= -1.0
    rm = torch.randn(C, generator=g) * 3.0
    rm[::7] = 1e3 * (2 * torch.rand(rm[::7].shape, generator=g) - 1)
    rm[0] = -1e3
    rv = 0.5 + 1.5 * torch.rand(C, generator=g)
    for k, v in enumerate((0.0, 1e-12, 1e-3, 1e4)):
        rv[k::11] = v  # (C = 1: running_var = 0)
    beta = 0.3 * torch.randn(C, generator=g).abs() * -torch.sign(rm * gamma)
    return gamma, beta, rm, rv


def _affine_f64(gamma, beta, rm, rv):
    invstd = 1.0 / (rv.double() + EPS32).sqrt()
    scale = gamma.double() * invstd
    return torch.stack([rm.double(), invstd, scale, beta.double() - rm.double() * scale])


def _single(n, C, CS, dev):
    """spcl_bn_eval_affine on device tensors ``dev`` = (gamma, beta, rm, rv) into sentinel-filled rows -> [4, CS]"""
    st = torch.full((4, CS), SENTINEL, device="cuda")
    n.call("spcl_bn_eval_affine", C, CS, n.ptr(dev[0]), n.ptr(dev[1]), n.ptr(dev[2]), n.ptr(dev[3]), c_float(EPS),
           n.ptr(st[0]), n.ptr(st[1]), n.ptr(st[2]), n.ptr(st[3]), n.stream())
    return st


def _check_affine(st, C, layer):
    ref = _affine_f64(*layer)
    got = st.cpu().double()
    assert torch.equal(got[:, C:], torch.zeros_like(got[:, C:]))  # the padding lanes: exactly 0, in all four rows
    assert torch.equal(got[0, :C], ref[0])                        # the mean is a copy
    for row, name in ((1, "invstd"), (2, "scale"), (3, "shift")):
        rel = ((got[row, :C] - ref[row]).abs() / ref[row].abs()).max()
        assert float(rel) <= 2e-6, (name, float(rel))  # a float32 sqrt, a division, two multiplications (and one sum)


@pytest.mark.parametrize("C,CS", [(1, 16), (16, 16), (24, 32), (256, 256), (300, 304), (512, 512)])
def test_bn_eval_affine_against_float64(C, CS):
    n = _n()
    layer = _layer(C, 10 * C + CS)
    st = _single(n, C, CS, [t.cuda() for t in layer])
    _check_affine(st, C, layer)


LAYER_CYCLE = [(1, 16), (512, 512), (16, 16), (300, 304), (256, 256), (24, 32)]  # a multi-block layer between single-block ones
PAD = 16  # sentinel floats around every st block


def _multi(n, shapes, nlaunch=None):
    """spcl_bn_eval_affine_multi over ``shapes`` = [(C, CS)], every st block surrounded by sentinels -> (buffer, offsets,
    layers, device tensors)"""
    layers = [_layer(C, 1000 + 17 * i + C) for i, (C, _) in enumerate(shapes)]
    devs = [[t.cuda() for t in layer] for layer in layers]
    offs, total = [], PAD
    for _, CS in shapes:
        offs.append(total)
        total += 4 * CS + PAD
    buf = torch.full((total,), SENTINEL, device="cuda")
    items = [n.BnEvalItem(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                          buf[o:o + 4 * CS].data_ptr(), C, CS, EPS) for d, o, (C, CS) in zip(devs, offs, shapes)]
    arr = (n.BnEvalItem * len(items))(*items)
    n.call("spcl_bn_eval_affine_multi", arr, len(items) if nlaunch is None else nlaunch, n.stream())
    return buf, offs, layers, devs


@pytest.mark.parametrize("count", [1, 22, 32])
def test_bn_eval_affine_multi_is_the_single_kernel_layer_by_layer(count):
    n = _n()
    shapes = [LAYER_CYCLE[i % len(LAYER_CYCLE)] for i in range(count)]
    buf, offs, layers, devs = _multi(n, shapes)
    covered = torch.zeros(buf.numel(), dtype=torch.bool)
    for (C, CS), o, layer, dev in zip(shapes, offs, layers, devs):
        st = buf[o:o + 4 * CS].view(4, CS)
        assert torch.equal(st.view(torch.int32), _single(n, C, CS, dev).view(torch.int32)), (C, CS, o)
        _check_affine(st, C, layer)
        covered[o:o + 4 * CS] = True
    outside = buf.cpu()[~covered]
    assert outside.numel() == PAD * (count + 1) and bool((outside == SENTINEL).all())


@pytest.mark.parametrize("count", [0, 33])
def test_bn_eval_affine_multi_refuses_a_bad_layer_count(count):
    n = _n()
    shapes = [(16, 16)] * 33
    layers = [_layer(16, 5)] * 33
    dev = [t.cuda() for t in layers[0]]
    buf = torch.full((33 * 64,), SENTINEL, device="cuda")
    items = [n.BnEvalItem(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
                          buf[64 * i:64 * i + 64].data_ptr(), C, CS, EPS) for i, (C, CS) in enumerate(shapes)]
    arr = (n.BnEvalItem * 33)(*items)
    with pytest.raises(RuntimeError, match=r"spcl_bn_eval_affine_multi failed \(-1\)"):  # SPCL_EINVAL
        n.call("spcl_bn_eval_affine_multi", arr, count, n.stream())
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


def test_prepare_eval_affines_chunks_and_hands_over_every_layer():
    """40 BatchNorms: two launches (SPCL_BN_EVAL_MAX = 32), 40 entries keyed (running_mean storage, CS), each the single-layer
    kernel's bits; ``clear_prepacked`` drops them"""
    from spcl_amd import functional as F
    n = _n()
    assert n.BN_EVAL_MAX == 32
    bns = []
    for i in range(40):
        C = LAYER_CYCLE[i % len(LAYER_CYCLE)][0]
        bn = torch.nn.BatchNorm2d(C, eps=EPS)
        gamma, beta, rm, rv = _layer(C, 300 + i)
        with torch.no_grad():
            bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
        bns.append(bn.cuda().eval())
    with _recorded_calls() as used:
        F.prepare_eval_affines(bns)
    try:
        assert [u for u in used if u.startswith("spcl_bn_eval")] == ["spcl_bn_eval_affine_multi"] * 2
        assert len(F._EVAL_AFFINE) == 40
        for bn in bns:
            C, CS = bn.num_features, ru16(bn.num_features)
            st = F._EVAL_AFFINE[(bn.running_mean.data_ptr(), CS)]
            assert tuple(st.shape) == (4, CS)
            ref = _single(n, C, CS, [bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var])
            assert torch.equal(st.view(torch.int32), ref.view(torch.int32)), C
    finally:
        F.clear_prepacked()
    assert len(F._EVAL_AFFINE) == 0


@pytest.mark.parametrize("C", [1, 8, 64, 100])
def test_rows_bn_eval_affine_against_float64(C):
    n = _n()
    layer = _layer(C, 77 + C)
    dev = [t.cuda() for t in layer]
    st = torch.full((4 * C + PAD,), SENTINEL, device="cuda")
    n.call("spcl_rows_bn_eval_affine", n.ptr(dev[0]), n.ptr(dev[1]), n.ptr(dev[2]), n.ptr(dev[3]), c_float(EPS), C, n.ptr(st),
           n.stream())
    assert bool((st[4 * C:] == SENTINEL).all())
    _check_affine(st[:4 * C].view(4, C), C, layer)


# ----------------------------------------------------------------------------------------------------------------------
# b. the float32 network, every stage
@contextmanager
def _recorded_calls():
    """the entry points launched inside the block, in order (tests/test_gpu_poolmax.py records them the same way)"""
    from spcl_amd import functional as F
    used, real = [], F._n.call
    F._n.call = lambda name, *args: (used.append(name), real(name, *args))[1]
    try:
        yield used
    finally:
        F._n.call = real


@contextmanager
def _f32_products(mode):
    n = _n()
    n.call("spcl_conv_set_f32_split", 1 if mode == "split" else 0)
    try:
        yield
    finally:
        n.call("spcl_conv_set_f32_split", 1)


def _statistics(model):
    return {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}


def _assert_statistics_unchanged(model, before):
    after = model.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), k


def _eval_stage(model, x, stage):
    """one no-grad eval pass up to ``stage`` -> (output on the CPU in float64, entry points it called)"""
    with torch.no_grad(), _recorded_calls() as used:
        out = model(x, until=E.until_of(stage))
        torch.cuda.synchronize()
    return out.detach().double().cpu(), used


def _assert_eval_route(used, stage):
    """the route the issue names: ONE multi-layer coefficient launch that every layer then takes its rows from, no batch
    statistics, no accumulator-block or window-maximum forms"""
    assert used.count("spcl_bn_eval_affine_multi") == 1, (stage, used)
    assert "spcl_bn_eval_affine" not in used, stage          # every layer found its rows in _EVAL_AFFINE
    assert not any(u.startswith("spcl_bn_finalize") for u in used), stage
    assert not any(u.endswith("_acc") or "ymax" in u for u in used), (stage, used)


def _assert_stage_close(stage, dev, c, where):
    err, bar = E.relmax(dev, c["f64"][stage]), c["f32_err"][stage]
    print(f"[eval f32] {where} {stage}: device {err:.2e}, float32 oracle {bar:.2e}, ratio {err / bar:.1f}")
    # 8 x: another summation order plus the split-product mode's documented 4e-7 .. 1e-6 per layer over up to 23 layers;
    # 2e-4: a noisy oracle figure must not excuse a real error
    assert err <= 8 * bar and err <= 2e-4, (where, stage, err, bar)


def _assert_argmax(dev_logits, c, where):
    ref = c["f64"]["Deconv_1x1"]
    low = E.low_margin(ref)
    assert float(low.double().mean()) <= E.MARGIN_SHARE, where
    assert int((dev_logits.argmax(1) != ref.argmax(1))[~low].sum()) == 0, where


SMALL = [(3, 48, 32, 128), (2, 64, 64, 256), (1, 112, 80, 128), (2, 16, 16, 128)]
_ids = lambda s: "x".join(map(str, s))  # noqa: E731


@pytest.mark.parametrize("f32_products", ["exact", "split"])
@pytest.mark.parametrize("shape", SMALL, ids=_ids)
def test_eval_network_fp32_every_stage_against_float64(shape, f32_products):
    N, H, W, mc = shape
    c = E.case(N, H, W, mc)
    model = E.load_unet(c["sd"], mc, torch.float32)
    before = _statistics(model)
    x = c["x"].float().cuda()
    print()
    with _f32_products(f32_products):
        for stage in E.STAGES:
            dev, used = _eval_stage(model, x, stage)
            _assert_eval_route(used, stage)
            _assert_stage_close(stage, dev, c, f"{shape} {f32_products}")
    _assert_argmax(dev, c, shape)
    _assert_statistics_unchanged(model, before)


@pytest.mark.parametrize("f32_products", ["exact", "split"])
def test_eval_network_fp32_logits_at_the_product_size(f32_products):
    """(2, 224, 224), max_channel 256: the tile and fusion decisions of the product's size differ from the small ones"""
    shape = (2, 224, 224, 256)
    c = E.case(*shape)
    model = E.load_unet(c["sd"], 256, torch.float32)
    before = _statistics(model)
    print()
    with _f32_products(f32_products):
        dev, used = _eval_stage(model, c["x"].float().cuda(), "Deconv_1x1")
    _assert_eval_route(used, "Deconv_1x1")
    _assert_stage_close("Deconv_1x1", dev, c, f"{shape} {f32_products}")
    _assert_argmax(dev, c, shape)
    _assert_statistics_unchanged(model, before)


@pytest.mark.parametrize("f32_products", ["exact", "split"])
@pytest.mark.parametrize("shape", [(3, 1, 28, 28), (2, 1, 48, 40), (2, 2, 32, 32), (3, 1, 100, 72)], ids=_ids)
def test_eval_encoder_fp32_odd_sizes_against_float64(shape, f32_products):
    """the odd sizes of test_encoder_fp32_vs_oracle_shapes (tile edges, an odd size in front of a pool, a two-channel image)"""
    N, cin, H, W = shape
    c = E.case(N, H, W, 128, cin, True)
    model = E.load_unet(c["sd"], 128, torch.float32, input_dim=cin)
    before = _statistics(model)
    x = c["x"].float().cuda()
    print()
    with _f32_products(f32_products):
        for stage in O.ENCODER_NAMES:
            dev, used = _eval_stage(model, x, stage)
            _assert_eval_route(used, stage)
            _assert_stage_close(stage, dev, c, f"{shape} {f32_products}")
    _assert_statistics_unchanged(model, before)


# ----------------------------------------------------------------------------------------------------------------------
# c. the bf16 network: every stage from the DEVICE's outputs of the stages before it
BF16_STAGE_BAR = 5e-3    # relative L2 per stage: the per-block bar of test_block_bf16_vs_bf16_emulating_oracle
BF16_NETWORK_BAR = 0.15  # relative L2 of the whole pass: the bar of test_encoder_bf16_drift_vs_fp32_golden


def _bf16_device_outputs(model, x, stages):
    outs = {}
    for s in stages:
        out, used = _eval_stage(model, x, s)
        _assert_eval_route(used, s)
        outs[s] = out
    return outs


@pytest.mark.parametrize("shape,compared", [((3, 48, 32, 128), E.STAGES), ((2, 64, 64, 256), E.STAGES),
                                            ((2, 224, 224, 256), ("Conv1", "Up_conv2", "Deconv_1x1"))],
                         ids=["3x48x32x128", "2x64x64x256", "2x224x224x256"])
def test_eval_network_bf16_stage_by_stage_teacher_forced(shape, compared):
    N, H, W, mc = shape
    c = E.case(N, H, W, mc)
    model = E.load_unet(c["sd"], mc, torch.bfloat16)
    before = _statistics(model)
    needed = [s for s in E.STAGES if s in compared or any(
        s in (E.STAGES[E.STAGES.index(t) - 1], E._SKIP.get(t)) for t in compared if t != "Conv1")]
    dev = _bf16_device_outputs(model, c["x"].float().cuda(), needed)
    print()
    for s in compared:
        if s != "Deconv_1x1":
            assert torch.equal(dev[s], dev[s].bfloat16().double()), s  # block outputs are bf16 values
        with torch.no_grad():
            ref = E.stage_oracle(s, E.stage_inputs(s, c["x"], dev), c["sd"], q=O.BF16Emulation)
        err = E.rel_l2(dev[s], ref)
        print(f"[eval bf16] {shape} {s}: relative L2 {err:.2e}")
        assert err <= BF16_STAGE_BAR, (shape, s, err)
    if len(compared) == len(E.STAGES):  # the whole pass from x: a wrong skip, a wrong half of a concatenation, a missing BatchNorm
        whole = E.rel_l2(dev["Deconv_1x1"], E.chain(c["x"], c["sd"], q=O.BF16Emulation)["Deconv_1x1"])
        print(f"[eval bf16] {shape} logits from x: relative L2 {whole:.2e}")
        assert whole <= BF16_NETWORK_BAR, (shape, whole)
    _assert_statistics_unchanged(model, before)


# ----------------------------------------------------------------------------------------------------------------------
# d. EvalEpocher
@pytest.mark.parametrize("graph", [False, True])
def test_eval_epocher_loss_and_dice_counts_against_the_oracle(graph):
    from spcl_amd.semi_seg.epochers.finetune import _EvalGraphs
    from tests.test_gpu_eval_graph import _Scans, _eval
    C, mc = 4, 128
    sd = E.eval_state(mc, 41, hw=(64, 64))
    model = E.load_unet(sd, mc, torch.float32)
    before = _statistics(model)
    loader = _Scans([6, 9], size=64, seed=43, classes=C)
    for _ in range(3 if graph else 1):  # a shape is run eagerly at first sight, captured at the second, replayed from then on
        _, inter, union, names, loss, _ = _eval(model, loader, graph=graph)
    if graph:
        entries = _EvalGraphs.of(model).entries
        assert len(entries) == 2 and all(e["graph"] is not None for e in entries.values())
    losses, row = [], 0
    for (img, tgt), _, _ in loader:
        img, tgt = img.cpu().double(), tgt.cpu().squeeze(1)
        logits = E.chain(img, sd)["Deconv_1x1"]
        losses.append(float(O.finetune_loss(logits, tgt)))
        low = E.low_margin(logits)
        pred = logits.argmax(1)
        near = (logits.max(1, keepdim=True).values - logits) < E.MARGIN * logits.abs().max()  # [N, C, H, W]: the classes a
        # float32 pass may name at a pixel (where every logit is the bias -- a dead pixel -- that is all of them)
        for b in range(img.shape[0]):
            sure = ~low[b]
            # the pixels float32 cannot flip, counted by the oracle; a low-margin pixel adds to a class's intersection only
            # where the label is that class, to its union the label and ONE of the classes within the margin of the leader
            ri, ru = O.dice_counts(pred[b][sure][None, None], tgt[b][sure][None, None], C)
            tgt_is = torch.stack([tgt[b][low[b]] == k for k in range(C)])  # [C, low pixels]
            low_tgt, low_top, low_hit = tgt_is.sum(1), near[b][:, low[b]].sum(1), (tgt_is & near[b][:, low[b]]).sum(1)
            di, du = inter[row].long(), union[row].long()
            assert bool((di >= ri[0]).all()) and bool((di <= ri[0] + low_hit).all()), (row, di, ri, low_hit)
            assert bool((du >= ru[0] + low_tgt).all()) and bool((du <= ru[0] + low_tgt + low_top).all()), (row, du, ru)
            assert int(du.sum()) == 2 * 64 * 64
            row += 1
    assert row == inter.shape[0] == 15
    ref_loss = sum(losses) / len(losses)  # the meter averages the batches' losses
    print(f"\n[eval epocher] graph={graph}: loss {loss:.8f}, oracle {ref_loss:.8f}")
    assert abs(loss - ref_loss) <= 1e-4 * abs(ref_loss), (loss, ref_loss)
    _assert_statistics_unchanged(model, before)


# ----------------------------------------------------------------------------------------------------------------------
# e. the eval branch of the BatchNorm backward
def _eval_bn_case(dtype, N, C, H, W, pool, with_act, seed, up2=False, y=None):
    """raw convolution output y (rounded to ``dtype``), an eval-mode BatchNorm in the style of ``_layer`` (negative gamma,
    running_var 0 / 1e-12 / 1e-3 / 1e4 channels, one |running_mean| = 1e3 channel), the incoming gradients, and float64
    autograd of relu(batch_norm(y, rm, rv, g, b, training=False)) (+ max_pool2d, or -- ``up2`` -- + nearest x2 upsampling)"""
    g = torch.Generator().manual_seed(seed)
    if y is None:
        y = rnd(torch.randn(N, C, H, W, generator=g) * 1.5 + 0.3, dtype)
    gamma = 0.5 + torch.rand(C, generator=g)
    gamma[::5] *= -1.0
    beta = 0.3 * torch.randn(C, generator=g)
    rm = 0.3 + torch.randn(C, generator=g)
    rv = 0.5 + 1.5 * torch.rand(C, generator=g)
    for k, v in enumerate((0.0, 1e-12, 1e-3, 1e4)):
        rv[k + 1::13] = v
    rm[C - 1] = 1e3 * (1.0 if gamma[C - 1] < 0 else -1.0)  # gamma * (y - rm) > 0: the channel is alive, all of it
    yr = y.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    a = TF.relu(TF.batch_norm(yr, rm.double(), rv.double(), gr, br, False, 0.1, EPS32))
    a.retain_grad()
    outs = []
    if up2:
        outs.append(TF.interpolate(a, scale_factor=2, mode="nearest"))
    elif with_act or not pool:
        outs.append(a)
    if pool:
        outs.append(TF.max_pool2d(a, 2, 2))
    douts = [rnd(torch.randn(o.shape, generator=g), dtype).double() for o in outs]
    torch.autograd.backward(outs, douts)
    # what the two sums add up, per channel: a float32 sum is off by a fraction of the sum of its terms' MAGNITUDES, so that is
    # what each channel's error is held against (one maximum over all channels would be the |running_mean| = 1e3 channel's)
    dz = (a.grad * (a > 0)).detach()
    yhat = (y.double() - rm.double().view(1, C, 1, 1)) / (rv.double() + EPS32).sqrt().view(1, C, 1, 1)
    mass = ((dz * yhat).abs().sum((0, 2, 3)), dz.abs().sum((0, 2, 3)))
    dact = douts[0].float() if (up2 or with_act or not pool) else None
    dpool = douts[-1].float() if pool else None
    return y, (gamma, beta, rm, rv), dact, dpool, (yr.grad, gr.grad, br.grad), mass, dz


def _eval_bn_errors(dgamma, dbeta, dy_nhwc, C, ref, mass):
    """-> (dgamma, dbeta, dy) errors, each the worst channel's: the sums against the sum of their terms' magnitudes, dy against
    the channel's largest |dy| (the channels' scales differ by 1e4: running_var 0 beside running_var 1e4)"""
    dy_ref, dg_ref, db_ref = ref
    eg = ((dgamma.cpu().double() - dg_ref).abs() / mass[0].clamp_min(1e-300)).max()
    eb = ((dbeta.cpu().double() - db_ref).abs() / mass[1].clamp_min(1e-300)).max()
    d = (dy_nhwc[..., :C].permute(0, 3, 1, 2).double().cpu() - dy_ref).abs().amax((0, 2, 3))
    ed = (d / dy_ref.abs().amax((0, 2, 3)).clamp_min(1e-300)).max()
    return float(eg), float(eb), float(ed)


BN_SHAPES = [(2, 16, 28, 28, True, False), (2, 48, 14, 10, True, True), (3, 32, 7, 5, True, True), (2, 64, 14, 14, False, True),
             (1, 24, 9, 9, True, False)]  # those of test_bn_relu_pool_forward_backward
BN_TOL = {"f32": 5e-5, "bf16": 8e-3}      # and its tolerances
BN_DT = {"f32": torch.float32, "bf16": torch.bfloat16}
# the entry points an eval-mode backward of the network reaches (test_eval_mode_backward_against_float64 records them): each
# has its training = 0 test below
EVAL_BWD_ENTRY_POINTS = ("spcl_bnrelu_pool_backward", "spcl_bnrelu_pool_backward_strided", "spcl_bnrelu_backward_up2",
                         "spcl_bnrelu_backward_image_wgrad", "spcl_bnrelu_backward_rows")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N,C,H,W,pool,with_act", BN_SHAPES)
def test_bnrelu_pool_backward_eval_branch(dt, N, C, H, W, pool, with_act):
    """spcl_bnrelu_pool_backward(training = 0): dy = scale dz, dgamma = sum dz (y - running_mean) invstd, dbeta = sum dz, with
    the coefficients spcl_bn_eval_affine makes of the running statistics"""
    n = _n()
    dtype = BN_DT[dt]
    dtc, cs = n.dtype_code(dtype), ru16(C)
    y, layer, dact, dpool, ref, mass, _ = _eval_bn_case(dtype, N, C, H, W, pool, with_act, 3 * C + H)
    st = _single(n, C, cs, [t.cuda() for t in layer])
    ys = nhwc(y, dtype)
    dact_d = nhwc(dact, dtype) if dact is not None else None
    dpool_d = nhwc(dpool, dtype) if dpool is not None else None
    ws = torch.empty(n.call("spcl_bnrelu_bwd_workspace_bytes", N, H, W, cs) // 4, device="cuda")
    dgm, dbt = torch.full((C,), SENTINEL, device="cuda"), torch.full((C,), SENTINEL, device="cuda")
    dy = torch.full((N, H, W, cs), SENTINEL, dtype=dtype, device="cuda")
    n.call("spcl_bnrelu_pool_backward", n.ptr(ys), n.ptr(dact_d), n.ptr(dpool_d), dtc, N, H, W, C, cs, n.ptr(st[0]),
           n.ptr(st[1]), n.ptr(st[2]), n.ptr(st[3]), 0, n.ptr(ws), n.ptr(dgm), n.ptr(dbt), n.ptr(dy), n.stream())
    e = _eval_bn_errors(dgm, dbt, dy, C, ref, mass)
    print(f"\n[eval bn bwd] {dt} {(N, C, H, W, pool, with_act)}: dgamma {e[0]:.2e}, dbeta {e[1]:.2e}, dy {e[2]:.2e}")
    assert max(e) < BN_TOL[dt], e


def _bwd_buffers(n, dtype, N, H, W, C, cs):
    ws = torch.empty(n.call("spcl_bnrelu_bwd_workspace_bytes", N, H, W, cs) // 4, device="cuda")
    dgm, dbt = torch.full((C,), SENTINEL, device="cuda"), torch.full((C,), SENTINEL, device="cuda")
    return ws, dgm, dbt, torch.full((N, H, W, cs), SENTINEL, dtype=dtype, device="cuda")


def _report(name, dt, shape, e):
    print(f"\n[eval bn bwd] {name} {dt} {shape}: dgamma {e[0]:.2e}, dbeta {e[1]:.2e}, dy {e[2]:.2e}")
    assert max(e) < BN_TOL[dt], (name, e)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N,C,H,W,pool", [(2, 48, 14, 10, True), (2, 64, 14, 14, False), (3, 24, 7, 5, False)])
def test_bnrelu_pool_backward_strided_eval_branch(dt, N, C, H, W, pool):
    """... with dact the SECOND half of a concatenation's gradient (pixel stride 2 CS), as a decoder skip hands it over"""
    n = _n()
    dtype = BN_DT[dt]
    dtc, cs = n.dtype_code(dtype), ru16(C)
    y, layer, dact, dpool, ref, mass, _ = _eval_bn_case(dtype, N, C, H, W, pool, True, 5 * C + W)
    st = _single(n, C, cs, [t.cuda() for t in layer])
    wide = torch.full((N, H, W, 2 * cs), 3.0, dtype=dtype, device="cuda")  # (the other half: a gradient that is not ours)
    wide[..., cs:] = nhwc(dact, dtype)
    half = wide[..., cs:]
    dpool_d = nhwc(dpool, dtype) if dpool is not None else None
    ws, dgm, dbt, dy = _bwd_buffers(n, dtype, N, H, W, C, cs)
    ys = nhwc(y, dtype)  # (every tensor a launch reads stays referenced until the results are back)
    n.call("spcl_bnrelu_pool_backward_strided", n.ptr(ys), n.ptr(half), 2 * cs, n.ptr(dpool_d), dtc, N, H, W, C, cs,
           n.ptr(st[0]), n.ptr(st[1]), n.ptr(st[2]), n.ptr(st[3]), 0, n.ptr(ws), n.ptr(dgm), n.ptr(dbt), n.ptr(dy), n.stream())
    _report("strided", dt, (N, C, H, W, pool), _eval_bn_errors(dgm, dbt, dy, C, ref, mass))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N,C,H,W", [(2, 16, 14, 14), (1, 48, 7, 5), (2, 64, 4, 4)])
def test_bnrelu_backward_up2_eval_branch(dt, N, C, H, W):
    """... with the gradient arriving behind nn.Upsample(scale_factor=2): [N, 2H, 2W, CS], summed 2 x 2 on the way"""
    n = _n()
    dtype = BN_DT[dt]
    dtc, cs = n.dtype_code(dtype), ru16(C)
    y, layer, d_up, _, ref, mass, _ = _eval_bn_case(dtype, N, C, H, W, False, False, 7 * C + H, up2=True)
    st = _single(n, C, cs, [t.cuda() for t in layer])
    gsum = torch.full((N, H, W, cs), SENTINEL, dtype=dtype, device="cuda")
    ws, dgm, dbt, dy = _bwd_buffers(n, dtype, N, H, W, C, cs)
    ys, dus = nhwc(y, dtype), nhwc(d_up, dtype)
    n.call("spcl_bnrelu_backward_up2", n.ptr(ys), n.ptr(dus), n.ptr(gsum), dtc, N, H, W, C, cs,
           n.ptr(st[0]), n.ptr(st[1]), n.ptr(st[2]), n.ptr(st[3]), 0, n.ptr(ws), n.ptr(dgm), n.ptr(dbt), n.ptr(dy), n.stream())
    _report("up2", dt, (N, C, H, W), _eval_bn_errors(dgm, dbt, dy, C, ref, mass))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N,C,H,W,nrows", [(2, 16, 28, 28, 1), (2, 64, 14, 14, 3), (1, 40, 9, 11, 7)])
def test_bnrelu_backward_rows_eval_branch(dt, N, C, H, W, nrows):
    """... with the two sums handed in as partial rows [nrows][2][CS] (sum dz, sum dz (y - mean)), as the dgrad epilogues
    and the 1x1 head's backward leave them: here the float64 sums of ``nrows`` slices of the pixels"""
    n = _n()
    dtype = BN_DT[dt]
    dtc, cs = n.dtype_code(dtype), ru16(C)
    y, layer, dact, _, ref, mass, dz = _eval_bn_case(dtype, N, C, H, W, False, True, 11 * C + H)
    st = _single(n, C, cs, [t.cuda() for t in layer])
    px_dz = dz.permute(1, 0, 2, 3).reshape(C, -1)
    px_yc = (y.double() - layer[2].double().view(1, C, 1, 1)).permute(1, 0, 2, 3).reshape(C, -1)
    rows = torch.zeros(nrows, 2, cs, dtype=torch.float64)
    for r, idx in enumerate(torch.arange(px_dz.shape[1]).chunk(nrows)):
        rows[r, 0, :C], rows[r, 1, :C] = px_dz[:, idx].sum(1), (px_dz[:, idx] * px_yc[:, idx]).sum(1)
    rows_d = rows.float().cuda()
    ws, dgm, dbt, dy = _bwd_buffers(n, dtype, N, H, W, C, cs)
    ys, das = nhwc(y, dtype), nhwc(dact, dtype)
    n.call("spcl_bnrelu_backward_rows", n.ptr(ys), n.ptr(das), None, n.ptr(rows_d), nrows, dtc, N, H, W,
           C, cs, n.ptr(st[0]), n.ptr(st[1]), n.ptr(st[2]), n.ptr(st[3]), 0, n.ptr(ws), n.ptr(dgm), n.ptr(dbt), n.ptr(dy), None,
           n.stream())
    _report("rows", dt, (N, C, H, W, nrows), _eval_bn_errors(dgm, dbt, dy, C, ref, mass))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N,C,H,W", [(2, 16, 30, 44), (3, 8, 17, 9)])
def test_bnrelu_backward_image_wgrad_eval_branch(dt, N, C, H, W):
    """... fused with the first convolution's weight gradient (one-channel image): dW = correlation of dy = scale dz with the
    image, no dy tensor.  dW against its own terms' magnitudes, like the two sums."""
    n = _n()
    dtype = BN_DT[dt]
    dtc, cs = n.dtype_code(dtype), ru16(C)
    g = torch.Generator().manual_seed(13 * C + H)
    x = torch.rand(N, 1, H, W, generator=g)
    w = torch.randn(C, 1, 3, 3, generator=g) * 0.5
    y = rnd(TF.conv2d(x, w, padding=1), dtype)  # the raw output as the forward pass stored it
    y, layer, dact, _, (dy_ref, dg_ref, db_ref), mass, _ = _eval_bn_case(dtype, N, C, H, W, False, True, 17 * C + W, y=y)
    dw_ref = torch.nn.grad.conv2d_weight(x.double(), (C, 1, 3, 3), dy_ref, 1, 1)
    dw_mass = torch.nn.grad.conv2d_weight(x.double(), (C, 1, 3, 3), dy_ref.abs(), 1, 1)  # (x >= 0: the terms' magnitudes)
    st = _single(n, C, cs, [t.cuda() for t in layer])
    ws = torch.empty(n.call("spcl_bnrelu_image_wgrad_workspace_bytes", N, H, W, cs) // 4, device="cuda")
    dgm, dbt = torch.full((C,), SENTINEL, device="cuda"), torch.full((C,), SENTINEL, device="cuda")
    dw = torch.full((C, 1, 3, 3), SENTINEL, device="cuda")
    xs = x.permute(0, 2, 3, 1).contiguous().cuda()
    ys, das = nhwc(y, dtype), nhwc(dact, dtype)
    n.call("spcl_bnrelu_backward_image_wgrad", n.ptr(ys), n.ptr(das), n.ptr(xs), dtc, N, H, W, C, cs,
           n.ptr(st[0]), n.ptr(st[1]), n.ptr(st[2]), n.ptr(st[3]), 0, n.ptr(ws), n.ptr(dgm), n.ptr(dbt), n.ptr(dw), n.stream())
    eg = float(((dgm.cpu().double() - dg_ref).abs() / mass[0].clamp_min(1e-300)).max())
    eb = float(((dbt.cpu().double() - db_ref).abs() / mass[1].clamp_min(1e-300)).max())
    ew = float(((dw.cpu().double() - dw_ref).abs() / dw_mass.clamp_min(1e-300)).max())
    print(f"\n[eval bn bwd] image_wgrad {dt} {(N, C, H, W)}: dgamma {eg:.2e}, dbeta {eb:.2e}, dW {ew:.2e}")
    assert max(eg, eb, ew) < BN_TOL[dt], (eg, eb, ew)


@pytest.mark.parametrize("shape", [(3, 48, 32, 128), (2, 64, 64, 256)], ids=_ids)
def test_eval_mode_backward_against_float64(shape):
    """a frozen-statistics network under grad (model.eval(), float32): every parameter gradient of the fine-tune loss against
    the float64 oracle at train=False.  (The gradient w.r.t. the IMAGE is no part of this: the first block refuses it in
    either mode -- see test_image_gradient_is_refused_not_wrong.)"""
    from spcl_amd import functional as F
    N, H, W, mc = shape
    gc = E.grad_case(N, H, W, mc)
    c, labels, loss64, g64 = gc["case"], gc["labels"], gc["loss"], gc["grads"]
    model = E.load_unet(c["sd"], mc, torch.float32)
    before = _statistics(model)
    x = c["x"].float().cuda()
    with _recorded_calls() as used:
        logits = model(x)
        loss = F.kl_div(F.softmax_classes(logits), F.one_hot_classes(labels.cuda(), 4))
        loss.backward()
        torch.cuda.synchronize()
    assert model.training is False
    bwd = sorted({u for u in used if u.startswith("spcl_bnrelu") and "backward" in u})
    print(f"\n[eval bwd] {shape}: loss {float(loss.detach()):.8f} (float64 {loss64:.8f}); BatchNorm backward entry points: {bwd}")
    assert used.count("spcl_bn_eval_affine_multi") == 1 and not any(u.startswith("spcl_bn_finalize") for u in used)
    assert abs(float(loss.detach()) - loss64) <= 1e-4 * abs(loss64)  # (the bar EvalEpocher's loss is held to above)
    failures = []
    params = dict(model.named_parameters())
    assert set(params) == set(g64)
    for k in sorted(g64):
        assert params[k].grad is not None, k
        err, bar = E.relmax(params[k].grad, g64[k]), gc["f32_err"][k]
        print(f"[eval bwd] {shape} {k}: device {err:.2e}, float32 oracle {bar:.2e}, ratio {err / max(bar, 1e-300):.1f}")
        if not (err <= 8 * bar and err <= 5e-4):
            failures.append((k, err, bar))
    assert not failures, failures
    assert set(bwd) <= set(EVAL_BWD_ENTRY_POINTS), bwd  # each of them has its kernel-level eval test above
    _assert_statistics_unchanged(model, before)


def test_image_gradient_is_refused_not_wrong():
    """the first block has no input-gradient kernel for the image, in train mode or eval mode: asking for it is an error (a
    missing kernel is never a quiet fall-back), so an eval-mode input gradient cannot be silently wrong"""
    from spcl_amd import functional as F
    gc = E.grad_case(3, 48, 32, 128)
    model = E.load_unet(gc["case"]["sd"], 128, torch.float32)
    x = gc["case"]["x"].float().cuda().requires_grad_(True)
    loss = F.kl_div(F.softmax_classes(model(x)), F.one_hot_classes(gc["labels"].cuda(), 4))
    with pytest.raises(NotImplementedError, match="input image"):
        loss.backward()
    torch.cuda.synchronize()
