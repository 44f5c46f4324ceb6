"""GPU: ``spcl_cross_pseudo_ce`` (csrc/cross_pseudo.hip) through ``functional.cross_pseudo_ce`` against the float64 restatement
of tests/_cps_oracle.py; two runs give the same bits in every output.

Each keep mask is a threshold compare of an f32 confidence: it cannot agree with float64 at pixels whose confidence sits on
the threshold.  So, as tests/test_gpu_pseudo_label_kernels.py does:

(b)  the pixels OF EITHER MAP with |conf64 - tau[y]| <= BAND = 2e-6 number at most max(1, 0.2 % of M) -- asserted on the oracle
     alone, before the kernel is looked at (on the CPU, for these inputs: 0 pixels at the five small shapes; 6, 16 and 4 of
     501 760 at the large one for 0.6, 0.95 and the linspace, against a bound of 1003);
(a)  outside the band both keep masks (``label != 255``) equal the oracle's at every pixel, and at every kept pixel the label
     is the arg-max of the logits;
(c)  ``hist[:2C]`` is the oracle's count of the two arg-maxes over all pixels, exactly; ``hist[2C:4C]`` is the count of the
     kernel's own label maps; ``hist[4C]`` is the number of pixels with yA == yB (29, 12, 361, 1338, 2106, 125 575);
(d)  with the KERNEL's masks given to the oracle: loss and both parts within 1e-5 relative, loss within 1e-6 relative of
     parts[0] + parts[1], da and db each within 1e-5 relative L2 (the bars of the sibling criteria), exact zeros in both
     gradients at every dropped pixel;
(f)  two runs give identical bits."""
import functools

import pytest
import torch

from tests import _cps_oracle as CO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 23
BAND = 2e-6
SHAPES = [(2, 2, 5, 7), (1, 16, 9, 33), (3, 4, 20, 24), (2, 3, 40, 52), (2, 4, 64, 66), (10, 4, 224, 224)]
AGREE = {(2, 2, 5, 7): 29, (1, 16, 9, 33): 12, (3, 4, 20, 24): 361, (2, 3, 40, 52): 1338, (2, 4, 64, 66): 2106,
         (10, 4, 224, 224): 125575}
THRESHOLDS = ("none", "0.6", "0.95", "linspace")
CASES = [(shape, th) for shape in SHAPES for th in THRESHOLDS]
SMALL = (3, 4, 20, 24)


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def _cl(x):
    return x.to(DEV).contiguous(memory_format=torch.channels_last)


def _tau(th, C):
    if th == "none":
        return None
    if th == "linspace":
        return torch.linspace(0.5, 0.9, C, dtype=torch.float32)
    return torch.full((C,), float(th), dtype=torch.float32)


@functools.lru_cache(maxsize=8)
def _inputs(shape):
    """(a, b, float64 confidences, labels): drawn and restated once, never modified"""
    g = torch.Generator().manual_seed(SEED)
    a = 3.0 * torch.randn(*shape, generator=g)
    b = 3.0 * torch.randn(*shape, generator=g)
    confA, yA = CO.conf_and_label(a)
    confB, yB = CO.conf_and_label(b)
    return a, b, confA, yA, confB, yB


def _run(a, b, tau, weight, upstream=None):
    """-> (loss, da, db, parts, hist, label_a, label_b), clones on the device"""
    from spcl_amd import functional as F_hip
    ad, bd = _cl(a).requires_grad_(True), _cl(b).requires_grad_(True)
    out = []
    loss = F_hip.cross_pseudo_ce(ad, bd, tau, weight, out=out)
    (loss if upstream is None else upstream * loss).backward()
    parts, hist, la, lb = out
    C = a.shape[1]
    assert loss.shape == () and loss.dtype == torch.float32
    assert parts.is_cuda and parts.dtype == torch.float32 and parts.shape == (2,)
    assert hist.dtype == torch.int64 and hist.shape == (4 * C + 1,)
    for lab in (la, lb):
        assert lab.shape == (a.shape[0], a.shape[2], a.shape[3]) and lab.dtype == torch.uint8
    return (loss.detach().clone(), ad.grad.clone(), bd.grad.clone(), parts.clone(), hist.clone(), la.clone(), lb.clone())


def _check_mask(label, conf64, y, tau):
    """(a) of one map against the thresholds ``tau`` (CPU f32 [C], or None); -> the kept map"""
    kept = label != 255
    if tau is None:
        assert bool(kept.all())
    else:
        in_band = (conf64 - tau.double()[y]).abs() <= BAND
        wrong = (kept != (conf64 >= tau.double()[y])) & ~in_band
        assert int(wrong.sum()) == 0, int(wrong.sum())
    assert torch.equal(label[kept].long(), y[kept])
    return kept


@pytest.mark.parametrize("shape,th", CASES)
def test_cross_pseudo_ce_vs_float64(shape, th):
    a, b, confA, yA, confB, yB = _inputs(shape)
    C, M = shape[1], confA.numel()
    tau = _tau(th, C)
    weight = 2.5 if shape[0] == 3 else 1.0
    n_band = 0
    if tau is not None:  # (b): the oracle alone
        n_band = int((((confA - tau.double()[yA]).abs() <= BAND) | ((confB - tau.double()[yB]).abs() <= BAND)).sum())
    assert n_band <= max(1, int(0.002 * M)), n_band
    tau_d = None if tau is None else tau.to(DEV)
    runs = [_run(a, b, tau_d, weight) for _ in range(2)]
    for x, y in zip(runs[0], runs[1]):  # (f)
        assert torch.equal(x, y)
    if tau is not None:
        assert torch.equal(tau_d.cpu(), tau)  # the thresholds are read only
    loss, da, db, parts, hist, la, lb = (x.cpu() for x in runs[0])
    keepA, keepB = _check_mask(la, confA, yA, tau), _check_mask(lb, confB, yB, tau)  # (a)
    count = functools.partial(torch.bincount, minlength=C)
    assert torch.equal(hist[:C], count(yA.flatten())) and torch.equal(hist[C:2 * C], count(yB.flatten()))  # (c)
    assert torch.equal(hist[2 * C:3 * C], count(la[keepA].long())) and torch.equal(hist[3 * C:4 * C], count(lb[keepB].long()))
    assert int(hist[4 * C]) == int((yA == yB).sum()) == AGREE[shape]
    assert torch.equal(hist, CO.hist(yA, yB, keepA, keepB, C))
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    ref_a, ref_b = CO.parts(a64, b64, yA, yB, keepA, keepB, weight)  # (d): the kernel's own masks
    ref = CO.loss(a64, b64, yA, yB, keepA, keepB, weight)
    ref.backward()
    ref, ref_a, ref_b = ref.detach(), ref_a.detach(), ref_b.detach()
    assert int(keepA.sum()) > 0 and int(keepB.sum()) > 0  # (these inputs keep pixels of both maps at every threshold)
    lerr, perr = _rel(loss, ref), max(_rel(parts[0], ref_a), _rel(parts[1], ref_b))
    serr = _rel(loss, parts.double().sum())
    gerr = max(_rel_l2(da, a64.grad), _rel_l2(db, b64.grad))
    print(f"cps {shape} tau={th}: kept {int(keepA.sum())} + {int(keepB.sum())} of 2 x {M}, in band {n_band}, agree "
          f"{int(hist[4 * C])}, loss rel {lerr:.2e}, parts rel {perr:.2e}, loss vs parts {serr:.2e}, grad rel L2 {gerr:.2e}")
    assert lerr <= 1e-5 and perr <= 1e-5 and gerr <= 1e-5, (lerr, perr, gerr)
    assert serr <= 1e-6, serr
    assert not bool(da[(~keepB)[:, None].expand_as(da)].any())  # exact zeros at every dropped pixel
    assert not bool(db[(~keepA)[:, None].expand_as(db)].any())


@pytest.mark.parametrize("shape,th", [((2, 3, 40, 52), "linspace"), ((2, 4, 64, 66), "0.6"), ((2, 4, 64, 66), "none")])
def test_swapping_the_arguments_swaps_the_outputs_bit_for_bit(shape, th):
    a, b = _inputs(shape)[:2]
    C = shape[1]
    tau = _tau(th, C)
    tau = None if tau is None else tau.to(DEV)
    loss, da, db, parts, hist, la, lb = _run(a, b, tau, 1.5)
    loss2, da2, db2, parts2, hist2, la2, lb2 = _run(b, a, tau, 1.5)
    assert torch.equal(loss, loss2)
    assert torch.equal(parts, parts2.flip(0))
    assert torch.equal(da, db2) and torch.equal(db, da2)
    assert torch.equal(la, lb2) and torch.equal(lb, la2)
    assert torch.equal(hist[:C], hist2[C:2 * C]) and torch.equal(hist[C:2 * C], hist2[:C])
    assert torch.equal(hist[2 * C:3 * C], hist2[3 * C:4 * C]) and torch.equal(hist[3 * C:4 * C], hist2[2 * C:3 * C])
    assert int(hist[4 * C]) == int(hist2[4 * C])


def test_exact_logit_ties_go_to_the_lowest_class():
    """labels by a hand-stated expectation, not by torch's tie rule: ties of two classes and of all classes, in both maps"""
    rows_a = [[1.0, 1.0, 0.0, 0.0], [0.0, 2.0, 2.0, 1.0], [0.0, 0.0, 0.0, 0.0], [-1.0, 0.0, 3.0, 3.0], [0.0, 5.0, 1.0, 5.0],
              [-2.0, -2.0, -2.0, -1.0]]
    rows_b = [[0.0, 0.0, 0.0, 0.0], [3.0, 1.0, 3.0, 0.0], [7.0, 7.0, 7.0, 7.0], [0.0, 0.0, 4.0, 4.0], [1.0, 0.0, 0.0, 1.0],
              [0.0, 1.0, 1.0, 1.0]]
    expect_a, expect_b = [0, 1, 0, 2, 1, 3], [0, 0, 0, 2, 0, 1]
    a = torch.tensor(rows_a).t().reshape(1, 4, 1, 6).contiguous()
    b = torch.tensor(rows_b).t().reshape(1, 4, 1, 6).contiguous()
    _, _, _, _, hist, la, lb = _run(a, b, None, 1.0)
    assert la.flatten().tolist() == expect_a and lb.flatten().tolist() == expect_b
    assert hist.tolist() == [2, 2, 1, 1] + [4, 1, 1, 0] + [2, 2, 1, 1] + [4, 1, 1, 0] + [3]
    # conf of an all-equal pixel is exactly 1 / C = 0.25 in f32: kept at tau[0] = 0.25, dropped one ulp above it
    quarter = torch.tensor([0.25, 0.0, 0.0, 0.0])
    _, _, _, _, _, la, lb = _run(a, b, quarter.to(DEV), 1.0)
    assert la.flatten().tolist()[2] == 0 and lb.flatten().tolist()[0] == 0 and lb.flatten().tolist()[2] == 0
    above = torch.nextafter(quarter, torch.ones(4))
    _, _, _, _, hist, la, lb = _run(a, b, above.to(DEV), 1.0)
    assert la.flatten().tolist()[2] == 255 and lb.flatten().tolist()[0] == 255 and lb.flatten().tolist()[2] == 255
    assert int(hist[8]) == 1 and int(hist[12]) == 2 and int(hist[0]) == 2 and int(hist[4]) == 4


def test_one_tensor_on_both_sides_agrees_everywhere_and_gets_both_gradients():
    from spcl_amd import functional as F_hip
    a = _inputs(SMALL)[0]
    M = a.shape[0] * a.shape[2] * a.shape[3]
    _, da, db, parts, hist, la, lb = _run(a, a, None, 2.5)
    assert int(hist[16]) == M and torch.equal(la, lb) and torch.equal(da, db) and torch.equal(parts[0], parts[1])
    x = _cl(a).requires_grad_(True)
    loss = F_hip.cross_pseudo_ce(x, x, None, 2.5)
    loss.backward()
    assert torch.equal(x.grad, da + db)
    x64 = a.double().requires_grad_(True)
    y = CO.conf_and_label(a)[1]
    (2.5 * 2.0 * torch.nn.functional.cross_entropy(x64, y)).backward()
    assert _rel_l2(x.grad, x64.grad) <= 1e-5


@pytest.mark.parametrize("shape", [SMALL, (2, 3, 40, 52)])
def test_labels_and_one_direction_equal_pseudo_label_ce(shape):
    """at the same tau the label maps are those ``pseudo_label_ce`` writes for the same teacher, exactly (the confidence is
    formed by the same helper); ``parts[0]`` and ``da`` are that call's loss and gradient at the 1e-5 bars"""
    from spcl_amd import functional as F_hip
    a, b = _inputs(shape)[:2]
    C = shape[1]
    tau = _tau("linspace", C).to(DEV)
    _, da, db, parts, hist, la, lb = _run(a, b, tau, 1.5)
    for teacher, student, label, part, grad, kept in ((b, a, lb, parts[0], da, hist[3 * C:4 * C]),
                                                      (a, b, la, parts[1], db, hist[2 * C:3 * C])):
        sd = _cl(student).requires_grad_(True)
        out = []
        loss = F_hip.pseudo_label_ce(_cl(teacher), sd, tau, 1.5, None, out=out)
        loss.backward()
        assert torch.equal(out[2], label)
        assert torch.equal(out[1][C:], kept)
        assert _rel(part, loss.detach()) <= 1e-5 and _rel_l2(grad, sd.grad) <= 1e-5


def test_a_threshold_above_one_keeps_nothing():
    a, b = _inputs(SMALL)[:2]
    tau = torch.full((4,), 1.5, device=DEV)
    loss, da, db, parts, hist, la, lb = _run(a, b, tau, 2.5)
    assert float(loss) == 0.0 and parts.tolist() == [0.0, 0.0] and not bool(da.any()) and not bool(db.any())
    assert bool((la == 255).all()) and bool((lb == 255).all())
    assert int(hist[8:16].sum()) == 0 and int(hist[:4].sum()) == int(hist[4:8].sum()) == la.numel()


def test_a_non_unit_upstream_gradient_scales_both_gradients():
    a, b, _, yA, _, yB = _inputs(SMALL)
    tau = torch.full((4,), 0.6, device=DEV)
    _, da1, db1, _, _, la1, lb1 = _run(a, b, tau, 1.0)
    _, da2, db2, _, _, la2, lb2 = _run(a, b, tau, 1.0, upstream=2.5)
    assert torch.equal(la1, la2) and torch.equal(lb1, lb2)
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    (2.5 * CO.loss(a64, b64, yA, yB, la2.cpu() != 255, lb2.cpu() != 255, 1.0)).backward()
    assert _rel_l2(da2, a64.grad) <= 1e-5 and _rel_l2(db2, b64.grad) <= 1e-5
    assert _rel_l2(da2, 2.5 * da1) <= 1e-6 and _rel_l2(db2, 2.5 * db1) <= 1e-6


def test_the_registered_unit_gradient_takes_the_shortcut():
    """the epocher's ``backward(gradient=ones)``: both saved maps come back as they are, no pass over them"""
    from spcl_amd import functional as F_hip
    a, b = _inputs(SMALL)[:2]
    _, da, db, _, _, _, _ = _run(a, b, None, 1.0)
    ad, bd = _cl(a).requires_grad_(True), _cl(b).requires_grad_(True)
    unit = F_hip.register_unit_gradient(torch.ones((), device=DEV))
    F_hip.cross_pseudo_ce(ad, bd).backward(gradient=unit)
    assert torch.equal(ad.grad, da) and torch.equal(bd.grad, db)


def test_unaligned_four_class_maps_take_the_generic_path_to_the_same_labels():
    from spcl_amd import functional as F_hip
    a, b = _inputs(SMALL)[:2]
    tau = torch.full((4,), 0.6, device=DEV)

    def shifted(x):
        nhwc = x.permute(0, 2, 3, 1).contiguous()
        buf = torch.empty(nhwc.numel() + 1, device=DEV)
        view = buf[1:].view(nhwc.shape)
        view.copy_(nhwc)
        assert view.data_ptr() % 16 == 4
        return view.permute(0, 3, 1, 2)

    outs = []
    for ad, bd in ((_cl(a), _cl(b)), (shifted(a), shifted(b))):
        out = []
        loss = F_hip.cross_pseudo_ce(ad, bd, tau, 1.0, out=out)
        outs.append((float(loss), [o.cpu() for o in out[1:]]))
    for x, y in zip(outs[0][1], outs[1][1]):
        assert torch.equal(x, y)
    assert abs(outs[0][0] - outs[1][0]) <= 1e-6 * abs(outs[0][0])


def test_the_call_captures_into_a_graph_and_replays_to_the_same_bits():
    """Five replays of one captured call.  Before each the captured inputs get new data (the two maps change places, so the
    expected outputs are the swapped ones) and every output is overwritten, with other launches and allocations in between:
    whatever the outputs hold afterwards, THAT replay wrote -- the closing workgroup's loss, parts and hist included."""
    from spcl_amd import functional as F_hip
    a, b = _inputs((2, 4, 64, 66))[:2]
    tau = torch.full((4,), 0.6, device=DEV)
    want = _run(a, b, tau, 1.5)
    ad, bd = _cl(a).requires_grad_(True), _cl(b).requires_grad_(True)
    unit = F_hip.register_unit_gradient(torch.ones((), device=DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # (warm-up outside the capture)
        torch.autograd.grad(F_hip.cross_pseudo_ce(ad, bd, tau, 1.5, out=[]), (ad, bd), grad_outputs=unit)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    out = []
    with torch.cuda.graph(graph):
        loss = F_hip.cross_pseudo_ce(ad, bd, tau, 1.5, out=out)
        da, db = torch.autograd.grad(loss, (ad, bd), grad_outputs=unit)
    got = (loss.detach(), da, db, *out)
    wants = (want, _run(b, a, tau, 1.5))
    assert not torch.equal(wants[0][3], wants[1][3]) and not torch.equal(wants[0][4], wants[1][4])
    for k in range(5):
        with torch.no_grad():
            ad.copy_(_cl(a if k % 2 == 0 else b))
            bd.copy_(_cl(b if k % 2 == 0 else a))
            for t in got:
                t.fill_(7)
        junk = torch.ones(4096, dtype=torch.bool, device=DEV)  # (an allocation between the replays)
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(got, wants[k % 2]):
            assert torch.equal(x, y), k
        del junk


def test_a_nan_logit_keeps_its_pixel_out_of_the_direction_it_teaches():
    """a NaN confidence keeps nothing: the pixel of ``a`` with a NaN logit teaches ``b`` nothing (label_a 255, db zero there);
    every other pixel is as it was, and nothing faults"""
    a, b = _inputs(SMALL)[:2]
    bad = a.clone()
    bad[1, 2, 7, 5] = float("nan")
    for tau in (None, torch.full((4,), 0.6, device=DEV)):
        _, da0, db0, _, hist0, la0, lb0 = _run(a, b, tau, 1.0)
        _, da, db, parts, hist, la, lb = _run(bad, b, tau, 1.0)
        torch.cuda.synchronize()
        assert int(la[1, 7, 5]) == 255 and not bool(db[1, :, 7, 5].any())
        assert bool(torch.isfinite(db).all()) and bool(torch.isfinite(parts[1]))
        assert torch.equal(lb, lb0)
        la0[1, 7, 5] = 255
        assert torch.equal(la, la0)
        db0[1, :, 7, 5] = 0.0
        assert torch.equal(db, db0)
        keep = torch.ones_like(la, dtype=torch.bool)
        keep[1, 7, 5] = False
        assert torch.equal(da[keep[:, None].expand_as(da)], da0[keep[:, None].expand_as(da0)])
        assert int(hist[8:12].sum()) == int((la != 255).sum())


def test_bad_arguments_are_refused_with_an_error():
    from spcl_amd import functional as F_hip
    t = torch.zeros(1, 4, 8, 8, device=DEV)
    tau = torch.full((4,), 0.5, device=DEV)
    with pytest.raises(ValueError, match="tau"):
        F_hip.cross_pseudo_ce(t, t, tau.double())  # dtype
    with pytest.raises(ValueError, match="tau"):
        F_hip.cross_pseudo_ce(t, t, tau[:3])  # length
    with pytest.raises(ValueError, match="tau"):
        F_hip.cross_pseudo_ce(t, t, torch.full((8,), 0.5, device=DEV)[::2])  # not contiguous
    with pytest.raises(ValueError, match="tau"):
        F_hip.cross_pseudo_ce(t, t, tau.cpu())  # device
    with pytest.raises(ValueError, match="tau"):
        F_hip.cross_pseudo_ce(t, t, [0.5] * 4)  # not a tensor
    with pytest.raises(AssertionError, match="differ"):
        F_hip.cross_pseudo_ce(t, torch.zeros(1, 4, 8, 9, device=DEV))
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.cross_pseudo_ce(t, t.cpu())
    t17 = torch.zeros(1, 17, 8, 8, device=DEV)
    with pytest.raises(ValueError, match="C = 17"):
        F_hip.cross_pseudo_ce(t17, t17)
    torch.cuda.synchronize()
