"""GPU: csrc/cutmix.hip through ``functional.cutmix_boxes``, ``cutmix_images`` and ``cross_pseudo_ce_mixed``.

The boxes are exactly those of the integer restatement in tests/_cutmix_oracle.py; the image mix is bit-equal to ``torch.where``
built from the oracle's boxes; the criterion is checked against float64 as tests/test_gpu_cps_kernels.py checks its sibling,
with the teachers gathered through the boxes:

(b)  the pixels whose GATHERED float64 confidence of either teacher lies within BAND = 2e-6 of its threshold number at most
     max(1, 0.2 % of M) -- asserted on the oracle alone, before the kernel is looked at (on the CPU, for these inputs: 0 pixels
     at the five small shapes; 5, 9 and 9 of 501 760 at the large one for 0.6, 0.95 and the linspace, against a bound of 1003);
(a)  outside the band both keep masks (``label != 255``) equal the oracle's at every pixel, and every kept label is the arg-max
     of the gathered teacher;
(c)  ``hist[:2C]``, the agreement count ``hist[4C]`` and the inside-a-box count ``hist[4C + 1]`` are the oracle's, exactly;
     ``hist[2C:4C]`` counts the kernel's own label maps;
(d)  with the KERNEL's masks given to the oracle: loss and both parts within 1e-5 relative, loss within 1e-6 relative of
     parts[0] + parts[1], both gradients within 1e-5 relative L2 (the bars of the sibling criteria), exact zeros in both
     gradients at every dropped pixel;
(f)  two runs give identical bits.

The shapes put every slab boundary (1024 pixels) of the 64 x 66 and 224 x 224 maps inside a box, take the generic and the C = 4
vector path, the general path at C = 16, and leave the last wave of the ballots partly filled (70, 891, 1440 pixels)."""
import functools

import pytest
import torch

from tests import _cps_oracle as CO
from tests import _cutmix_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 23
BAND = 2e-6
RANGES = [(0.25, 0.5), (1.0, 1.0), (1 / 65536, 1 / 65536)]
SHAPES = [(2, 2, 5, 7), (3, 16, 9, 33), (3, 4, 20, 24), (2, 3, 40, 52), (2, 4, 64, 66), (10, 4, 224, 224)]
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


# ------------------------------------------------------------------------------------------------------------------- boxes
@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (9, 33), (224, 1), (224, 224)])
@pytest.mark.parametrize("N", [1, 2, 7, 300])
def test_boxes_are_the_oracles(N, hw):
    from spcl_amd import functional as F_hip
    H, W = hw
    for prop in RANGES:
        for seed in (0, 23, 2 ** 31 + 5):
            want = O.boxes(seed, N, H, W, prop)
            got = F_hip.cutmix_boxes(seed, N, H, W, prop, device=DEV)
            assert got.dtype == torch.int32 and got.shape == (N, 4) and got.is_cuda
            assert torch.equal(got.cpu(), want), (seed, prop)
            word = torch.tensor([seed - 2 ** 32 if seed >= 2 ** 31 else seed], dtype=torch.int32, device=DEV)
            assert torch.equal(F_hip.cutmix_boxes(word, N, H, W, prop), got)  # an int and a device word: the same bits
            assert torch.equal(F_hip.cutmix_boxes(seed, N, H, W, prop, device=DEV), got)  # two calls
            y0, x0, bh, bw = (got.cpu()[:, k] for k in range(4))
            assert bool((y0 >= 0).all() and (x0 >= 0).all() and (bh >= 1).all() and (bw >= 1).all())
            assert bool((y0 + bh <= H).all() and (x0 + bw <= W).all())
    if H * W > 1:  # (a 1 x 1 image has one box)
        a, b = (F_hip.cutmix_boxes(s, N, H, W, device=DEV) for s in (23, 24))
        assert not torch.equal(a, b)
    full = F_hip.cutmix_boxes(7, N, H, W, (1.0, 1.0), device=DEV).cpu()
    assert full.tolist() == [[0, 0, H, W]] * N


def test_the_fixed_boxes_and_the_seed_word_is_read_at_run_time():
    from spcl_amd import functional as F_hip
    word = torch.tensor([23], dtype=torch.int32, device=DEV)
    got = F_hip.cutmix_boxes(word, 3, 20, 24)
    assert got.cpu().tolist() == [[6, 8, 14, 10], [2, 11, 18, 12], [5, 3, 9, 17]]
    assert int(word) == 23  # read only
    word.add_(1)
    assert torch.equal(F_hip.cutmix_boxes(word, 3, 20, 24).cpu(), O.boxes(24, 3, 20, 24))


def test_boxes_refuse_bad_arguments():
    from spcl_amd import functional as F_hip
    for bad in ((0.0, 0.5), (0.5, 0.25), (0.5, 1.5), (-0.1, 0.5), 0.3, (0.1, 0.2, 0.3)):
        with pytest.raises(ValueError, match="prop_range"):
            F_hip.cutmix_boxes(0, 2, 8, 8, bad, device=DEV)
    for seed in (-1, 2 ** 32, 1.5, True, torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(1, device=DEV)):
        with pytest.raises(ValueError, match="seed"):
            F_hip.cutmix_boxes(seed, 2, 8, 8, device=DEV)
    for N, H, W in ((0, 8, 8), (2, 0, 8), (2, 8, -1), (2 ** 20 + 1, 8, 8), (2.0, 8, 8)):
        with pytest.raises(ValueError):
            F_hip.cutmix_boxes(0, N, H, W, device=DEV)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ images
@pytest.mark.parametrize("shape,dtype,layout", [((2, 1, 5, 7), torch.float32, "nchw"), ((3, 1, 64, 66), torch.bfloat16, "nchw"),
                                                ((4, 3, 20, 24), torch.float32, "nchw"), ((4, 3, 20, 24), torch.float32, "nhwc"),
                                                ((4, 3, 20, 24), torch.bfloat16, "nhwc"), ((3, 2, 9, 33), torch.bfloat16, "nhwc"),
                                                ((10, 1, 224, 224), torch.float32, "nchw")])
def test_the_image_mix_is_torch_where_bit_for_bit(shape, dtype, layout):
    from spcl_amd import functional as F_hip
    N, C, H, W = shape
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(*shape, generator=g).to(dtype).to(DEV)
    if layout == "nhwc":
        x = x.contiguous(memory_format=torch.channels_last)
    before = x.clone()
    for prop in ((0.25, 0.5), (1.0, 1.0), (1 / 65536, 1 / 65536)):
        bx = O.boxes(SEED, N, H, W, prop)
        for roll in sorted({1, N - 1}):
            got = F_hip.cutmix_images(x, bx.to(DEV), roll)
            want = O.mix_images(x, bx, roll)
            assert got.dtype == dtype and got.shape == x.shape and got.stride() == x.stride()
            assert torch.equal(got, want), (prop, roll)
            assert torch.equal(got.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                               want.contiguous(memory_format=torch.channels_last if layout == "nhwc"
                                               else torch.contiguous_format).view(
                                   torch.int16 if dtype == torch.bfloat16 else torch.int32))
            assert torch.equal(got, F_hip.cutmix_images(x, bx.to(DEV), roll))
    assert torch.equal(x, before)  # the input is read only
    inside = O.inside(O.boxes(SEED, N, H, W), H, W)
    assert 0 < int(inside.sum()) < inside.numel()


def test_the_image_mix_on_unaligned_and_strided_batches():
    """a batch whose storage starts 4 bytes past a 16-byte boundary takes the scalar path; any other striding is made
    contiguous first: the same result"""
    from spcl_amd import functional as F_hip
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(4, 3, 20, 24, generator=g).to(DEV)
    bx = O.boxes(SEED, 4, 20, 24)
    want = O.mix_images(x, bx, 1)
    buf = torch.empty(x.numel() + 1, device=DEV)
    view = buf[1:].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4
    assert torch.equal(F_hip.cutmix_images(view, bx.to(DEV), 1), want)
    wide = torch.randn(4, 3, 20, 48, generator=g).to(DEV)
    half = wide[..., ::2]
    assert not half.is_contiguous()
    assert torch.equal(F_hip.cutmix_images(half, bx.to(DEV), 1), O.mix_images(half, bx, 1))


def test_the_image_mix_never_indexes_by_a_box_value():
    """boxes that no sampler writes (negative, huge, overflowing extents) only change which of the two samples a pixel shows:
    the result is ``torch.where`` with the mask of the unsigned range compare"""
    from spcl_amd import functional as F_hip
    big = 2 ** 31 - 1
    bx = torch.tensor([[-5, -5, 10, 10], [0, 0, big, big], [big, big, big, big], [3, 4, -1, 2]], dtype=torch.int32)
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(4, 2, 9, 12, generator=g).to(DEV)
    ys, xs = torch.arange(9).view(1, 9, 1), torch.arange(12).view(1, 1, 12)
    b = bx.long()

    def rng(v, lo, ext):  # (unsigned)(v - lo) < (unsigned)ext on 32-bit words
        return ((v - lo.view(-1, 1, 1)) % 2 ** 32) < (ext.view(-1, 1, 1) % 2 ** 32)

    mask = rng(ys, b[:, 0], b[:, 2]) & rng(xs, b[:, 1], b[:, 3])
    assert mask[1].all() and mask[0, :5, :5].all() and int(mask[0].sum()) == 25 and not mask[2].any() and mask[3].any()
    want = torch.where(mask.view(4, 1, 9, 12).to(DEV), x.roll(-1, 0), x)
    assert torch.equal(F_hip.cutmix_images(x, bx.to(DEV), 1), want)
    torch.cuda.synchronize()


def test_images_refuse_bad_arguments():
    from spcl_amd import functional as F_hip
    x = torch.zeros(3, 1, 8, 8, device=DEV)
    bx = torch.zeros(3, 4, dtype=torch.int32, device=DEV)
    for roll in (0, 3, -1, 1.0, True):
        with pytest.raises(ValueError, match="roll"):
            F_hip.cutmix_images(x, bx, roll)
    with pytest.raises(ValueError, match="roll"):
        F_hip.cutmix_images(x[:1], bx[:1], 1)  # one sample has nothing to mix with
    for bad in (bx.long(), bx[:2], bx.cpu(), bx.view(4, 3), [[0, 0, 1, 1]] * 3):
        with pytest.raises(ValueError, match="boxes"):
            F_hip.cutmix_images(x, bad, 1)
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        F_hip.cutmix_images(x.half(), bx, 1)
    with pytest.raises(ValueError, match="N, C, H, W"):
        F_hip.cutmix_images(x[0], bx, 1)
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.cutmix_images(x.cpu(), bx, 1)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------------------- criterion
@functools.lru_cache(maxsize=8)
def _inputs(shape):
    """(s_a, s_b, t_a, t_b, boxes, float64 confidences and labels of the GATHERED teachers): drawn and restated once, never
    modified"""
    g = torch.Generator().manual_seed(SEED)
    s_a, s_b, t_a, t_b = (3.0 * torch.randn(*shape, generator=g) for _ in range(4))
    N, _, H, W = shape
    bx = O.boxes(SEED, N, H, W, (0.25, 0.5))
    confA, yA, confB, yB = O.teachers(t_a, t_b, bx, 1)
    return s_a, s_b, t_a, t_b, bx, confA, yA, confB, yB


def _run(s_a, s_b, t_a, t_b, bx, tau, weight, upstream=None, roll=1):
    """-> (loss, da, db, parts, hist, label_a, label_b), clones on the device"""
    from spcl_amd import functional as F_hip
    ad, bd = _cl(s_a).requires_grad_(True), _cl(s_b).requires_grad_(True)
    out = []
    loss = F_hip.cross_pseudo_ce_mixed(ad, bd, _cl(t_a), _cl(t_b), None if bx is None else bx.to(DEV), roll, tau, weight,
                                       out=out)
    (loss if upstream is None else upstream * loss).backward()
    parts, hist, la, lb = out
    C = s_a.shape[1]
    assert loss.shape == () and loss.dtype == torch.float32
    assert parts.is_cuda and parts.dtype == torch.float32 and parts.shape == (2,)
    assert hist.dtype == torch.int64 and hist.shape == (4 * C + 2,)
    for lab in (la, lb):
        assert lab.shape == (s_a.shape[0], s_a.shape[2], s_a.shape[3]) and lab.dtype == torch.uint8
    return (loss.detach().clone(), ad.grad.clone(), bd.grad.clone(), parts.clone(), hist.clone(), la.clone(), lb.clone())


def _check_mask(label, conf64, y, tau):
    """(a) of one teacher against the thresholds ``tau`` (CPU f32 [C], or None); -> the kept map"""
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
def test_cross_pseudo_ce_mixed_vs_float64(shape, th):
    s_a, s_b, t_a, t_b, bx, confA, yA, confB, yB = _inputs(shape)
    N, C, H, W = shape
    M = confA.numel()
    tau = _tau(th, C)
    weight = 2.5 if shape == SMALL else 1.0
    n_band = 0
    if tau is not None:  # (b): the oracle alone
        n_band = int((((confA - tau.double()[yA]).abs() <= BAND) | ((confB - tau.double()[yB]).abs() <= BAND)).sum())
    assert n_band <= max(1, int(0.002 * M)), n_band
    tau_d = None if tau is None else tau.to(DEV)
    runs = [_run(s_a, s_b, t_a, t_b, bx, tau_d, weight) for _ in range(2)]
    for x, y in zip(runs[0], runs[1]):  # (f)
        assert torch.equal(x, y)
    if tau is not None:
        assert torch.equal(tau_d.cpu(), tau)  # the thresholds are read only
    loss, da, db, parts, hist, la, lb = (x.cpu() for x in runs[0])
    keepA, keepB = _check_mask(la, confA, yA, tau), _check_mask(lb, confB, yB, tau)  # (a)
    count = functools.partial(torch.bincount, minlength=C)
    assert torch.equal(hist[:C], count(yA.flatten())) and torch.equal(hist[C:2 * C], count(yB.flatten()))  # (c)
    assert torch.equal(hist[2 * C:3 * C], count(la[keepA].long())) and torch.equal(hist[3 * C:4 * C], count(lb[keepB].long()))
    n_in = int(O.inside(bx, H, W).sum())
    assert int(hist[4 * C]) == int((yA == yB).sum()) and int(hist[4 * C + 1]) == n_in and 0 < n_in < M
    assert torch.equal(hist, O.hist(yA, yB, keepA, keepB, C, bx))
    a64, b64 = s_a.double().requires_grad_(True), s_b.double().requires_grad_(True)
    ref_a, ref_b = O.parts(a64, b64, yA, yB, keepA, keepB, weight)  # (d): the kernel's own masks
    ref = O.loss(a64, b64, yA, yB, keepA, keepB, weight)
    ref.backward()
    ref, ref_a, ref_b = ref.detach(), ref_a.detach(), ref_b.detach()
    assert int(keepA.sum()) > 0 and int(keepB.sum()) > 0  # (these inputs keep pixels of both teachers at every threshold)
    lerr, perr = _rel(loss, ref), max(_rel(parts[0], ref_a), _rel(parts[1], ref_b))
    serr = _rel(loss, parts.double().sum())
    gerr = max(_rel_l2(da, a64.grad), _rel_l2(db, b64.grad))
    print(f"cps mixed {shape} tau={th}: kept {int(keepA.sum())} + {int(keepB.sum())} of 2 x {M}, in band {n_band}, agree "
          f"{int(hist[4 * C])}, inside {n_in}, loss rel {lerr:.2e}, parts rel {perr:.2e}, loss vs parts {serr:.2e}, grad rel L2 "
          f"{gerr:.2e}")
    assert lerr <= 1e-5 and perr <= 1e-5 and gerr <= 1e-5, (lerr, perr, gerr)
    assert serr <= 1e-6, serr
    assert not bool(da[(~keepB)[:, None].expand_as(da)].any())  # exact zeros at every dropped pixel
    assert not bool(db[(~keepA)[:, None].expand_as(db)].any())


def _oracle_check(got, s_a, s_b, t_a, t_b, bx, weight):
    """loss, parts and gradients of one threshold-free run against float64 (every pixel kept), hist exactly"""
    loss, da, db, parts, hist, la, lb = (x.cpu() for x in got)
    N, C, H, W = s_a.shape
    _, yA, _, yB = O.teachers(t_a, t_b, bx, 1)
    every = torch.ones_like(yA, dtype=torch.bool)
    assert torch.equal(la.long(), yA) and torch.equal(lb.long(), yB)
    assert torch.equal(hist, O.hist(yA, yB, every, every, C, bx))
    a64, b64 = s_a.double().requires_grad_(True), s_b.double().requires_grad_(True)
    ref = O.loss(a64, b64, yA, yB, every, every, weight)
    ref.backward()
    assert _rel(loss, ref.detach()) <= 1e-5 and _rel(loss, parts.double().sum()) <= 1e-6
    assert _rel_l2(da, a64.grad) <= 1e-5 and _rel_l2(db, b64.grad) <= 1e-5


def test_the_sibling_and_the_mixed_entry_at_one_workspace_size_do_not_share_a_ticket():
    """``cross_pseudo_ce`` on 22 x 4 x 32 x 32 and ``cross_pseudo_ce_mixed`` on 21 x 4 x 32 x 32 both ask for 1912 bytes (22 * 84 +
    64 = 21 * 88 + 64) with the ticket at byte 352 and at byte 336.  Neither entry zeroes its ticket, so one kept buffer for both
    would hand the mixed entry a partial sum of the sibling's as its ticket: no workgroup would close, and loss, parts and hist
    would stay what ``torch.empty`` found.  Either order, twice; every output against the oracle."""
    from spcl_amd import functional as F_hip
    from spcl_amd import native
    L = native.lib()
    assert L.spcl_cross_pseudo_workspace_bytes(22, 4, 32, 32) == L.spcl_cross_pseudo_mixed_workspace_bytes(21, 4, 32, 32) == 1912
    g = torch.Generator().manual_seed(SEED)
    big = [3.0 * torch.randn(22, 4, 32, 32, generator=g) for _ in range(2)]
    s_a, s_b, t_a, t_b = (3.0 * torch.randn(21, 4, 32, 32, generator=g) for _ in range(4))
    bx = O.boxes(SEED, 21, 32, 32)
    (confA, yA), (confB, yB) = CO.conf_and_label(big[0]), CO.conf_and_label(big[1])
    every = torch.ones_like(yA, dtype=torch.bool)
    ref = CO.loss(big[0].double(), big[1].double(), yA, yB, every, every, 1.0)
    firsts = []
    for k in range(2):
        out = []
        sib = F_hip.cross_pseudo_ce(_cl(big[0]), _cl(big[1]), None, 1.0, out=out)  # fills the rows of its own layout
        assert _rel(sib, ref) <= 1e-5 and torch.equal(out[1].cpu(), CO.hist(yA, yB, every, every, 4)), k
        got = _run(s_a, s_b, t_a, t_b, bx, None, 1.0)
        _oracle_check(got, s_a, s_b, t_a, t_b, bx, 1.0)
        firsts.append(got)
    for x, y in zip(*firsts):
        assert torch.equal(x, y)
    out = []
    sib = F_hip.cross_pseudo_ce(_cl(big[0]), _cl(big[1]), None, 1.0, out=out)  # and the sibling after the mixed entry
    assert _rel(sib, ref) <= 1e-5 and torch.equal(out[1].cpu(), CO.hist(yA, yB, every, every, 4))


def test_one_entry_at_two_class_counts_of_one_workspace_size_does_not_share_a_ticket():
    """within the mixed entry: C = 2 with 9 workgroups and C = 3 with 7 ask for 568 bytes each (9 * 56 + 64 = 7 * 72 + 64), the
    ticket at byte 144 and at byte 112 -- where the C = 2 layout keeps the partial sums of its row 7"""
    from spcl_amd import native
    L = native.lib()
    assert L.spcl_cross_pseudo_mixed_workspace_bytes(9, 2, 32, 32) == L.spcl_cross_pseudo_mixed_workspace_bytes(7, 3, 32, 32) == 568
    g = torch.Generator().manual_seed(SEED)
    two = [3.0 * torch.randn(9, 2, 32, 32, generator=g) for _ in range(4)]
    three = [3.0 * torch.randn(7, 3, 32, 32, generator=g) for _ in range(4)]
    for k in range(2):
        for maps in (two, three):
            bx = O.boxes(SEED + k, maps[0].shape[0], 32, 32)
            _oracle_check(_run(*maps, bx, None, 1.0), *maps, bx, 1.0)


def test_the_mix_matters_and_the_last_roll_reads_the_sample_before():
    """the labels differ from the unmixed teachers' inside the boxes only; roll N - 1 gathers from sample n - 1"""
    s_a, s_b, t_a, t_b, bx, _, yA, _, yB = _inputs(SMALL)
    N, C, H, W = SMALL
    inside = O.inside(bx, H, W)
    _, _, _, _, hist, la, lb = (x.cpu() for x in _run(s_a, s_b, t_a, t_b, bx, None, 1.0))
    plainA, plainB = CO.conf_and_label(t_a)[1], CO.conf_and_label(t_b)[1]
    assert torch.equal(la.long(), yA) and torch.equal(lb.long(), yB)
    assert torch.equal(la.long()[~inside], plainA[~inside]) and not torch.equal(la.long()[inside], plainA[inside])
    assert torch.equal(la.long()[inside], plainA.roll(-1, 0)[inside]) and torch.equal(lb.long()[inside], plainB.roll(-1, 0)[inside])
    _, _, _, _, hist2, la2, lb2 = (x.cpu() for x in _run(s_a, s_b, t_a, t_b, bx, None, 1.0, roll=N - 1))
    _, yA2, _, yB2 = O.teachers(t_a, t_b, bx, N - 1)
    assert torch.equal(la2.long(), yA2) and torch.equal(lb2.long(), yB2)
    assert torch.equal(la2.long()[inside], plainA.roll(1, 0)[inside]) and int(hist2[4 * C + 1]) == int(inside.sum())


def test_a_non_unit_upstream_gradient_scales_both_gradients():
    s_a, s_b, t_a, t_b, bx, _, yA, _, yB = _inputs(SMALL)
    tau = torch.full((4,), 0.6, device=DEV)
    _, da1, db1, _, _, la1, lb1 = _run(s_a, s_b, t_a, t_b, bx, tau, 1.0)
    _, da2, db2, _, _, la2, lb2 = _run(s_a, s_b, t_a, t_b, bx, tau, 1.0, upstream=2.5)
    assert torch.equal(la1, la2) and torch.equal(lb1, lb2)
    a64, b64 = s_a.double().requires_grad_(True), s_b.double().requires_grad_(True)
    (2.5 * O.loss(a64, b64, yA, yB, la2.cpu() != 255, lb2.cpu() != 255, 1.0)).backward()
    assert _rel_l2(da2, a64.grad) <= 1e-5 and _rel_l2(db2, b64.grad) <= 1e-5
    assert _rel_l2(da2, 2.5 * da1) <= 1e-6 and _rel_l2(db2, 2.5 * db1) <= 1e-6


# ------------------------------------------------------------------------------------------------------ identities, bit for bit
@pytest.mark.parametrize("shape,th", [((2, 2, 5, 7), "none"), ((3, 16, 9, 33), "linspace"), ((2, 3, 40, 52), "0.6"),
                                      ((2, 4, 64, 66), "0.6"), ((10, 4, 224, 224), "linspace"), ((10, 4, 224, 224), "none")])
def test_without_boxes_and_with_the_students_as_teachers_it_is_cross_pseudo_ce(shape, th):
    from spcl_amd import functional as F_hip
    s_a, s_b = _inputs(shape)[:2]
    C = shape[1]
    tau = _tau(th, C)
    tau = None if tau is None else tau.to(DEV)
    loss, da, db, parts, hist, la, lb = _run(s_a, s_b, s_a, s_b, None, tau, 1.5)
    ad, bd = _cl(s_a).requires_grad_(True), _cl(s_b).requires_grad_(True)
    out = []
    want = F_hip.cross_pseudo_ce(ad, bd, tau, 1.5, out=out)
    want.backward()
    assert torch.equal(loss, want.detach()) and torch.equal(parts, out[0])
    assert torch.equal(da, ad.grad) and torch.equal(db, bd.grad)
    assert torch.equal(hist[:4 * C + 1], out[1]) and int(hist[4 * C + 1]) == 0
    assert torch.equal(la, out[2]) and torch.equal(lb, out[3])


@pytest.mark.parametrize("shape,th", [((2, 3, 40, 52), "linspace"), ((2, 4, 64, 66), "0.6"), ((2, 4, 64, 66), "none")])
def test_swapping_the_networks_swaps_the_outputs_bit_for_bit(shape, th):
    s_a, s_b, t_a, t_b, bx = _inputs(shape)[:5]
    C = shape[1]
    tau = _tau(th, C)
    tau = None if tau is None else tau.to(DEV)
    loss, da, db, parts, hist, la, lb = _run(s_a, s_b, t_a, t_b, bx, tau, 1.5)
    loss2, da2, db2, parts2, hist2, la2, lb2 = _run(s_b, s_a, t_b, t_a, bx, tau, 1.5)
    assert torch.equal(loss, loss2)
    assert torch.equal(parts, parts2.flip(0))
    assert torch.equal(da, db2) and torch.equal(db, da2)
    assert torch.equal(la, lb2) and torch.equal(lb, la2)
    assert torch.equal(hist[:C], hist2[C:2 * C]) and torch.equal(hist[C:2 * C], hist2[:C])
    assert torch.equal(hist[2 * C:3 * C], hist2[3 * C:4 * C]) and torch.equal(hist[3 * C:4 * C], hist2[2 * C:3 * C])
    assert torch.equal(hist[4 * C:], hist2[4 * C:])


@pytest.mark.parametrize("shape", [SMALL, (2, 3, 40, 52), (2, 4, 64, 66)])
def test_keep_masks_and_labels_equal_two_pseudo_label_ce_calls_on_gathered_teachers(shape):
    """the composition from the package's ops: ``torch.where`` gathers of the teachers, then ``pseudo_label_ce`` each way.  Keep
    masks and labels are equal exactly (one confidence helper); each part and gradient is that call's at the 1e-5 bars"""
    from spcl_amd import functional as F_hip
    s_a, s_b, t_a, t_b, bx = _inputs(shape)[:5]
    N, C, H, W = shape
    tau = _tau("linspace", C).to(DEV)
    _, da, db, parts, hist, la, lb = _run(s_a, s_b, t_a, t_b, bx, tau, 1.5)
    mask = O.inside(bx, H, W).view(N, 1, H, W).to(DEV)
    for teacher, student, label, part, grad, kept in ((t_b, s_a, lb, parts[0], da, hist[3 * C:4 * C]),
                                                      (t_a, s_b, la, parts[1], db, hist[2 * C:3 * C])):
        td = teacher.to(DEV)
        mixed_teacher = torch.where(mask, td.roll(-1, 0), td)
        sd = _cl(student).requires_grad_(True)
        out = []
        loss = F_hip.pseudo_label_ce(_cl(mixed_teacher), sd, tau, 1.5, None, out=out)
        loss.backward()
        assert torch.equal(out[2], label)
        assert torch.equal(out[1][C:], kept)
        assert _rel(part, loss.detach()) <= 1e-5 and _rel_l2(grad, sd.grad) <= 1e-5


def test_teachers_handed_in_with_requires_grad_get_none():
    from spcl_amd import functional as F_hip
    s_a, s_b, t_a, t_b, bx = _inputs(SMALL)[:5]
    sa, sb, ta, tb = (_cl(t).requires_grad_(True) for t in (s_a, s_b, t_a, t_b))
    F_hip.cross_pseudo_ce_mixed(sa, sb, ta, tb, bx.to(DEV), 1).backward()
    assert sa.grad is not None and sb.grad is not None and ta.grad is None and tb.grad is None
    assert bool(sa.grad.any()) and bool(sb.grad.any())


def test_the_criterion_never_indexes_by_a_box_value():
    """boxes no sampler writes: the teachers' sample is n or n + 1 mod N whatever they hold; nothing faults and the labels are
    the oracle's under the unsigned range compare"""
    s_a, s_b, t_a, t_b = _inputs(SMALL)[:4]
    N, C, H, W = SMALL
    big = 2 ** 31 - 1
    bx = torch.tensor([[-5, -5, 10, 10], [0, 0, big, big], [3, 4, -1, 2]], dtype=torch.int32)
    ys, xs = torch.arange(H).view(1, H, 1), torch.arange(W).view(1, 1, W)
    b = bx.long()

    def rng(v, lo, ext):
        return ((v - lo.view(-1, 1, 1)) % 2 ** 32) < (ext.view(-1, 1, 1) % 2 ** 32)

    mask = rng(ys, b[:, 0], b[:, 2]) & rng(xs, b[:, 1], b[:, 3])
    m = torch.where(mask, (torch.arange(N).view(N, 1, 1) + 1) % N, torch.arange(N).view(N, 1, 1).expand(N, H, W))
    yA, yB = CO.conf_and_label(O.gather(t_a, m))[1], CO.conf_and_label(O.gather(t_b, m))[1]
    _, _, _, _, hist, la, lb = (x.cpu() for x in _run(s_a, s_b, t_a, t_b, bx, None, 1.0))
    assert torch.equal(la.long(), yA) and torch.equal(lb.long(), yB) and int(hist[4 * C + 1]) == int(mask.sum())
    torch.cuda.synchronize()


def test_the_call_captures_into_a_graph_and_replays_to_the_same_bits():
    """Five replays of one captured call (boxes, criterion, gradients).  Before each the captured inputs get new data -- the two
    networks change places and the SEED WORD changes, so the boxes do -- and every output is overwritten, with other launches and
    allocations in between: whatever the outputs hold afterwards, THAT replay wrote."""
    from spcl_amd import functional as F_hip
    shape = (2, 4, 64, 66)
    s_a, s_b, t_a, t_b = _inputs(shape)[:4]
    N, _, H, W = shape
    tau = torch.full((4,), 0.6, device=DEV)
    seeds = (23, 24)
    wants = (_run(s_a, s_b, t_a, t_b, O.boxes(seeds[0], N, H, W), tau, 1.5),
             _run(s_b, s_a, t_b, t_a, O.boxes(seeds[1], N, H, W), tau, 1.5))
    assert not torch.equal(wants[0][3], wants[1][3]) and not torch.equal(wants[0][4], wants[1][4])
    ad, bd = _cl(s_a).requires_grad_(True), _cl(s_b).requires_grad_(True)
    tad, tbd = _cl(t_a), _cl(t_b)
    word = torch.tensor([seeds[0]], dtype=torch.int32, device=DEV)
    unit = F_hip.register_unit_gradient(torch.ones((), device=DEV))

    def call(out):
        bx = F_hip.cutmix_boxes(word, N, H, W)
        return F_hip.cross_pseudo_ce_mixed(ad, bd, tad, tbd, bx, 1, tau, 1.5, out=out), bx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # (warm-up outside the capture)
        torch.autograd.grad(call([])[0], (ad, bd), grad_outputs=unit)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    out = []
    with torch.cuda.graph(graph):
        loss, bx = call(out)
        da, db = torch.autograd.grad(loss, (ad, bd), grad_outputs=unit)
    got = (loss.detach(), da, db, *out)
    for k in range(5):
        with torch.no_grad():
            ad.copy_(_cl(s_a if k % 2 == 0 else s_b))
            bd.copy_(_cl(s_b if k % 2 == 0 else s_a))
            tad.copy_(_cl(t_a if k % 2 == 0 else t_b))
            tbd.copy_(_cl(t_b if k % 2 == 0 else t_a))
            word.fill_(seeds[k % 2])
            bx.fill_(-3)
            for t in got:
                t.fill_(7)
        junk = torch.ones(4096, dtype=torch.bool, device=DEV)  # (an allocation between the replays)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bx.cpu(), O.boxes(seeds[k % 2], N, H, W)), k
        for x, y in zip(got, wants[k % 2]):
            assert torch.equal(x, y), k
        del junk


def test_bad_arguments_are_refused_with_an_error():
    from spcl_amd import functional as F_hip
    t = torch.zeros(2, 4, 8, 8, device=DEV)
    tau = torch.full((4,), 0.5, device=DEV)
    bx = torch.zeros(2, 4, dtype=torch.int32, device=DEV)
    for bad in (tau.double(), tau[:3], torch.full((8,), 0.5, device=DEV)[::2], tau.cpu(), [0.5] * 4):
        with pytest.raises(ValueError, match="tau"):
            F_hip.cross_pseudo_ce_mixed(t, t, t, t, bx, 1, bad)
    for bad in (bx.long(), bx[:1], bx.cpu(), torch.zeros(2, 3, dtype=torch.int32, device=DEV), [[0, 0, 1, 1]] * 2):
        with pytest.raises(ValueError, match="boxes"):
            F_hip.cross_pseudo_ce_mixed(t, t, t, t, bad, 1)
    for roll in (0, 2, -1, 1.0):
        with pytest.raises(ValueError, match="roll"):
            F_hip.cross_pseudo_ce_mixed(t, t, t, t, bx, roll)
    with pytest.raises(ValueError, match="roll"):  # one sample has nothing to mix with
        F_hip.cross_pseudo_ce_mixed(t[:1], t[:1], t[:1], t[:1], bx[:1], 1)
    F_hip.cross_pseudo_ce_mixed(t[:1], t[:1], t[:1], t[:1], None, 0)  # (no boxes: the roll is not looked at)
    other = torch.zeros(2, 4, 8, 9, device=DEV)
    for k in range(1, 4):
        maps = [t, t, t, t]
        maps[k] = other
        with pytest.raises(AssertionError, match="differ"):
            F_hip.cross_pseudo_ce_mixed(*maps, bx, 1)
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.cross_pseudo_ce_mixed(t, t, t, t.cpu(), bx, 1)
    t17 = torch.zeros(2, 17, 8, 8, device=DEV)
    with pytest.raises(ValueError, match="C = 17"):
        F_hip.cross_pseudo_ce_mixed(t17, t17, t17, t17, bx, 1)
    torch.cuda.synchronize()
