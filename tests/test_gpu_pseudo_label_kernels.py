"""GPU: ``spcl_pseudo_label_ce`` (csrc/pseudo_label.hip) through ``functional.pseudo_label_ce`` against the float64 restatement
of tests/_pseudo_label_oracle.py; two runs give the same bits in every output.

The mask is a threshold compare of an f32 confidence: it cannot agree with float64 at pixels whose confidence sits on the
threshold.  So, as tests/test_gpu_ucmt_kernels.py does for its f32 entropy:

(b)  the pixels with |conf64 - tau[y]| <= BAND = 2e-6 number at most max(1, 0.2 % of M) -- asserted on the oracle alone,
     before the kernel is looked at (on the CPU, for these inputs: 0 pixels at the four small shapes, at most 10 of 501 760 at
     the large one; f32 against f64 confidence differs by at most 3.0e-7, about 6x room for ``expf``);
(a)  outside the band the kernel's mask (``label != 255``) equals the oracle's at every pixel;
(a') at every kept pixel ``label`` is the arg-max of the logits, and ``hist[:C]`` is the oracle's count of the arg-max over all
     pixels, exactly (tie-independent: the same f32 values are compared);
(c)  ``hist[C:]`` is the count of the kernel's own ``label`` map, its sum the number of kept pixels;
(d)  with the KERNEL's mask given to the oracle: loss within 1e-5 relative, gradient within 1e-5 relative L2 (the bars of the
     sibling criteria), exact zeros in the gradient at every dropped pixel;
(e)  ``stats`` within 1e-5 relative of the float64 sums.  The kernel sums f32 values (conf = 1 / z, q_c = e_c / z) in double;
     restated on the CPU in f32 (exp(x - max), their sum z, 1 / z and e_c / z, summed in float64) the miss against the float64
     sums was at most 2.8e-8 relative (1 x 16 x 9 x 33) and 1.8e-10 at 10 x 4 x 224 x 224: the bar of 1e-5 leaves more than
     350x room;
(f)  two runs give identical bits.

Adaptive mode: before each of three calls on three different batches ``tau`` is read back; that call's mask obeys (a) against
THAT ``tau`` (the one-step lag), and afterwards ``state`` / ``tau`` equal ``update()`` fed the kernel's own ``stats``."""
import functools

import pytest
import torch

from tests import _pseudo_label_oracle as PO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 11
BAND = 2e-6
BIG_FLAGS = (3, 0, 1, 2, 0, 3, 1, 2, 0, 3)
SHAPES = [((3, 4, 20, 24), (3, 0, 1)), ((3, 4, 20, 24), None), ((2, 2, 5, 7), (2, 1)), ((1, 16, 9, 33), (3,)),
          ((2, 3, 192, 200), None), ((10, 4, 224, 224), BIG_FLAGS)]
THRESHOLDS = ("0.6", "0.95", "linspace")
CASES = [(shape, flags, th) for shape, flags in SHAPES for th in THRESHOLDS]


def _rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _cl(x):
    return x.to(DEV).contiguous(memory_format=torch.channels_last)


def _tau(th, C):
    if th == "linspace":
        return torch.linspace(0.5, 0.9, C, dtype=torch.float32)
    return torch.full((C,), float(th), dtype=torch.float32)


@functools.lru_cache(maxsize=8)
def _inputs(shape, flags, seed=SEED):
    """(teacher, student, float64 confidence, label, float64 stats): drawn and restated once, never modified"""
    g = torch.Generator().manual_seed(seed)
    t, s = 3.0 * torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
    conf, label = PO.conf_and_label(t, flags)
    return t, s, conf, label, PO.stats(t, flags)


def _run(t, s, tau, weight, flags, state=None, momentum=0.999, upstream=None):
    from spcl_amd import functional as F_hip
    fl = None if flags is None else torch.tensor(flags, dtype=torch.uint8, device=DEV)
    td, sd = _cl(t).requires_grad_(True), _cl(s).requires_grad_(True)
    out = []
    loss = F_hip.pseudo_label_ce(td, sd, tau, weight, fl, state=state, momentum=momentum, out=out)
    (loss if upstream is None else upstream * loss).backward()
    assert td.grad is None  # the teacher gets no gradient
    stats, hist, label = out
    C = s.shape[1]
    assert stats.is_cuda and stats.dtype == torch.float64 and stats.shape == (1 + C,)
    assert hist.dtype == torch.int64 and hist.shape == (2 * C,)
    assert label.shape == (s.shape[0], s.shape[2], s.shape[3]) and label.dtype == torch.uint8
    return loss.detach().clone(), sd.grad.clone(), stats.clone(), hist.clone(), label.clone()


def _check_mask(label, conf64, y, tau):
    """(a) and (a') of one call against the thresholds ``tau`` (CPU f32 [C]); -> (kept map, pixels in the band)"""
    in_band = (conf64 - tau.double()[y]).abs() <= BAND
    kept = label != 255
    wrong = (kept != (conf64 >= tau.double()[y])) & ~in_band
    assert int(wrong.sum()) == 0, int(wrong.sum())
    assert torch.equal(label[kept].long(), y[kept])
    return kept, int(in_band.sum())


@pytest.mark.parametrize("shape,flags,th", CASES)
def test_pseudo_label_ce_vs_float64(shape, flags, th):
    t, s, conf64, y, stats64 = _inputs(shape, flags)
    C, M = shape[1], conf64.numel()
    tau = _tau(th, C)
    weight = 1.0 if flags is None else 2.5
    in_band = (conf64 - tau.double()[y]).abs() <= BAND
    assert int(in_band.sum()) <= max(1, int(0.002 * M)), int(in_band.sum())  # (b): the oracle alone
    tau_d = tau.to(DEV)
    runs = [_run(t, s, tau_d, weight, flags) for _ in range(2)]
    for a, b in zip(runs[0], runs[1]):  # (f)
        assert torch.equal(a, b)
    assert torch.equal(tau_d.cpu(), tau)  # fixed thresholds are read only
    loss, grad, stats, hist, label = (x.cpu() for x in runs[0])
    kept, n_band = _check_mask(label, conf64, y, tau)  # (a), (a')
    assert torch.equal(hist[:C], torch.bincount(y.flatten(), minlength=C))
    assert torch.equal(hist[C:], torch.bincount(label[kept].long(), minlength=C))  # (c)
    assert int(hist[C:].sum()) == int(kept.sum())
    s64 = s.double().requires_grad_(True)
    ref = PO.loss(s64, y, kept, weight)  # (d): the kernel's own mask
    ref.backward()
    if int(kept.sum()) == 0:
        assert float(loss) == 0.0 and not bool(grad.any())
        lerr = gerr = 0.0
    else:
        lerr = abs(float(loss) - float(ref.detach())) / float(ref.detach())
        gerr = _rel_l2(grad, s64.grad)
    serr = float(((stats - stats64).abs() / stats64.abs()).max())  # (e)
    print(f"pseudo-label {shape} flags={flags is not None} tau={th}: kept {int(kept.sum())} of {M}, in band {n_band}, "
          f"loss rel {lerr:.2e}, grad rel L2 {gerr:.2e}, stats rel {serr:.2e}")
    assert lerr <= 1e-5 and gerr <= 1e-5, (lerr, gerr)
    assert serr <= 1e-5, serr
    dropped = (~kept)[:, None].expand_as(grad)
    assert not bool(grad[dropped].any())  # exact zeros at every dropped pixel


def test_a_threshold_above_one_keeps_nothing():
    shape, flags = SHAPES[0]
    t, s, _, _, _ = _inputs(shape, flags)
    tau = torch.full((4,), 1.5, device=DEV)
    loss, grad, stats, hist, label = _run(t, s, tau, 2.5, flags)
    assert float(loss) == 0.0 and not bool(grad.any()) and bool((label == 255).all())
    assert int(hist[4:].sum()) == 0 and int(hist[:4].sum()) == label.numel()


def test_a_threshold_of_zero_is_the_plain_cross_entropy():
    shape, flags = SHAPES[0]
    t, s, _, y, _ = _inputs(shape, flags)
    tau = torch.zeros(4, device=DEV)
    loss, grad, stats, hist, label = _run(t, s, tau, 2.5, flags)
    assert torch.equal(label.cpu().long(), y) and torch.equal(hist[:4], hist[4:])
    s64 = s.double().requires_grad_(True)
    ref = 2.5 * torch.nn.functional.cross_entropy(s64, y)
    ref.backward()
    assert abs(float(loss) - float(ref.detach())) <= 1e-5 * float(ref.detach())
    assert _rel_l2(grad, s64.grad) <= 1e-5


def test_exact_logit_ties_go_to_the_lowest_class():
    """labels by a hand-stated expectation, not by torch's tie rule; the all-equal pixel is class 0 with conf == 1 / C"""
    rows = [[1.0, 1.0, 0.0, 0.0], [0.0, 2.0, 2.0, 1.0], [0.0, 0.0, 0.0, 0.0], [-1.0, 0.0, 3.0, 3.0], [0.0, 5.0, 1.0, 5.0],
            [-2.0, -2.0, -2.0, -1.0]]
    expect = [0, 1, 0, 2, 1, 3]
    t = torch.tensor(rows).t().reshape(1, 4, 1, 6).contiguous()
    s = torch.randn(1, 4, 1, 6, generator=torch.Generator().manual_seed(SEED))
    _, _, stats, hist, label = _run(t, s, torch.zeros(4, device=DEV), 1.0, None)
    assert label.flatten().tolist() == expect
    assert hist.tolist() == [2, 2, 1, 1, 2, 2, 1, 1]
    # conf of the all-equal pixel is exactly 1 / C = 0.25 in f32: kept at tau[0] = 0.25, dropped one ulp above it
    quarter = torch.tensor([0.25, 0.0, 0.0, 0.0])
    _, _, _, _, label = _run(t, s, quarter.to(DEV), 1.0, None)
    assert label.flatten().tolist()[2] == 0
    above = torch.nextafter(quarter, torch.ones(4))
    _, _, _, hist, label = _run(t, s, above.to(DEV), 1.0, None)
    assert label.flatten().tolist()[2] == 255 and int(hist[4]) == 1 and int(hist[0]) == 2


def test_a_non_unit_upstream_gradient_is_scaled():
    shape, flags = SHAPES[0]
    t, s, _, y, _ = _inputs(shape, flags)
    tau = torch.full((4,), 0.6, device=DEV)
    _, g1, _, _, l1 = _run(t, s, tau, 1.0, flags)
    _, g2, _, _, l2 = _run(t, s, tau, 1.0, flags, upstream=2.5)
    assert torch.equal(l1, l2)
    s64 = s.double().requires_grad_(True)
    (2.5 * PO.loss(s64, y, l2.cpu() != 255, 1.0)).backward()
    assert _rel_l2(g2, s64.grad) <= 1e-5
    assert _rel_l2(g2, 2.5 * g1) <= 1e-6


def test_unaligned_four_class_maps_take_the_scalar_path_to_the_same_labels():
    """C = 4 maps that are not 16-byte aligned leave the vector path: same labels and counts, loss within the f32 bar"""
    shape, flags = SHAPES[0]
    t, s, _, _, _ = _inputs(shape, flags)
    from spcl_amd import functional as F_hip
    fl = torch.tensor(flags, dtype=torch.uint8, device=DEV)
    tau = torch.full((4,), 0.6, device=DEV)

    def shifted(x):
        nhwc = x.permute(0, 2, 3, 1).contiguous()
        buf = torch.empty(nhwc.numel() + 1, device=DEV)
        view = buf[1:].view(nhwc.shape)
        view.copy_(nhwc)
        assert view.data_ptr() % 16 == 4
        return view.permute(0, 3, 1, 2)

    outs = []
    for td, sd in ((_cl(t), _cl(s)), (shifted(t), shifted(s))):
        out = []
        loss = F_hip.pseudo_label_ce(td, sd, tau, 1.0, fl, out=out)
        outs.append((float(loss), out[1].cpu(), out[2].cpu()))
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])
    assert abs(outs[0][0] - outs[1][0]) <= 1e-6 * abs(outs[0][0])


@pytest.mark.parametrize("shape", [(3, 4, 20, 24), (2, 3, 192, 200)])
@pytest.mark.parametrize("momentum", [0.9, 0.5])
def test_adaptive_thresholds_lag_one_step_and_follow_the_update(shape, momentum):
    from spcl_amd import functional as F_hip
    C = shape[1]
    flags = (3, 0, 1) if shape[0] == 3 else None
    tau, state = F_hip.pseudo_label_state(C, DEV)
    assert torch.equal(tau.cpu(), torch.full((C,), 1.0 / C))
    assert torch.equal(state.cpu(), torch.full((1 + C,), 1.0 / C, dtype=torch.float64))
    for step in range(3):
        t, s, conf64, y, _ = _inputs(shape, flags, SEED + step)
        M = conf64.numel()
        tau_before, state_before = tau.cpu().clone(), state.cpu().clone()
        loss, grad, stats, hist, label = (x.cpu() for x in _run(t, s, tau, 1.0, flags, state=state, momentum=momentum))
        kept, n_band = _check_mask(label, conf64, y, tau_before)  # the lag: THIS call compared against the old tau
        assert int(hist[C:].sum()) == int(kept.sum())
        want_state, want_tau = PO.update(state_before, stats, M, momentum)
        serr = float(((state.cpu() - want_state).abs() / want_state.abs()).max())
        want32 = want_tau.float()
        ulp = torch.nextafter(want32, torch.full_like(want32, 2.0)) - want32
        terr = float(((tau.cpu() - want32).abs() / ulp).max())
        print(f"adaptive {shape} m={momentum} step {step}: kept {int(kept.sum())} of {M}, in band {n_band}, tau_g "
              f"{float(state[0]):.6f}, state rel {serr:.2e}, tau off by {terr:.1f} ulp")
        assert serr <= 1e-14, serr
        assert terr <= 1.0, terr
        assert not torch.equal(tau.cpu(), tau_before)


def test_bad_arguments_are_refused_with_an_error():
    from spcl_amd import functional as F_hip
    t = torch.zeros(1, 4, 8, 8, device=DEV)
    tau = torch.full((4,), 0.5, device=DEV)
    with pytest.raises(ValueError):
        F_hip.pseudo_label_ce(t, t, tau.double())  # dtype
    with pytest.raises(ValueError):
        F_hip.pseudo_label_ce(t, t, tau[:3])  # length
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.pseudo_label_ce(t, t, tau.cpu())  # device
    with pytest.raises(ValueError):
        F_hip.pseudo_label_ce(t, t, tau, state=torch.zeros(5, device=DEV))  # f32 state
    with pytest.raises(ValueError):
        F_hip.pseudo_label_ce(t, t, tau, state=torch.zeros(4, dtype=torch.float64, device=DEV))  # length
    with pytest.raises(ValueError):
        F_hip.pseudo_label_ce(t, t, tau, momentum=1.0)
    t17 = torch.zeros(1, 17, 8, 8, device=DEV)
    with pytest.raises(RuntimeError, match="C <= 16"):
        F_hip.pseudo_label_ce(t17, t17, torch.full((17,), 0.5, device=DEV))
    torch.cuda.synchronize()
