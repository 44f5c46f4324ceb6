"""GPU: ``spcl_strong_view_params`` and ``spcl_strong_view_apply`` (csrc/strong_view.hip) against tests/_strong_view_oracle.py.

The two layers are judged apart: the table against the oracle's (draws, mask, seed word and count bit for bit; the mean within
one float32 spacing of the float32-rounded float64 mean -- the float64 sum's own error is below 2^-40 relative), and the apply
kernel, fed the ORACLE's table, against the float64 pipeline.

The bar of the apply kernel: ``atol = K * 2^-24 * c_hi * b_hi`` with K = 64 where gamma is on (``powf`` at the OpenCL bound of 16
ulp on a value <= 1) and K = 16 elsewhere (at most a dozen further roundings on magnitudes <= c_hi * b_hi plus the noise; the
total doubled); c_hi, b_hi: the upper ends of the contrast and brightness ranges where those ops are on, else 1.  Where the
oracle's value before the last clamp lies beyond [0, 1] by more than the bar, the output is exactly 0 or 1.  bf16: within 2^-8 (one
bf16 spacing below 1, plus the float32 error).

Shapes: one pixel; smaller than the halo with W no multiple of 4; one past the tile in both directions; C > 1 with odd extents;
an aligned vector case; one batch of the workload's size.  Every flag value occurs in every case."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _strong_view_oracle as O
from tests.test_strong_view_host import APPLY_REFUSALS, OPS, PARAMS_REFUSALS, call_apply, call_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1, 1, 1), (2, 1, 3, 5), "tile+1", (2, 3, 17, 23), (4, 1, 64, 64), (10, 1, 224, 224)]
IDS = ["1x1x1x1", "2x1x3x5", "3x1xtile+1", "2x3x17x23", "4x1x64x64", "10x1x224x224"]


def _shape(shape):
    if shape == "tile+1":
        from spcl_amd import functional as F_hip
        th, tw = F_hip.strong_view_tile()
        return (3, 1, th + 1, tw + 1)
    return shape


def _cfg(on, p=1.0):
    """the default ranges with the gates of the ops in ``on`` at ``p`` and every other gate shut"""
    from spcl_amd.functional import StrongViewConfig
    return StrongViewConfig(**{name: {"p": p if name in on else 0.0} for name in OPS})


def _input(shape, dtype, seed=0):
    """values in [-0.1, 1.1]: the first clamp has work to do; -> (device tensor, the stored values as float64 numpy)"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(shape, generator=g) * 1.2 - 0.1).to(dtype)
    return x.to(DEV), x.double().numpy()


def _flag_sets(N):
    """flag vectors for N samples in which, together, all four values occur"""
    return [[(n + r) % 4 for n in range(N)] for r in range(0, 4, min(N, 4))]


def _bits(t):
    return np.ascontiguousarray(t).view(np.uint32)


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


# ------------------------------------------------------------------------------------------------------------------ table
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_table_is_the_oracles(shape, dtype):
    from spcl_amd import functional as F_hip
    shape = _shape(shape)
    x, x64 = _input(shape, dtype, seed=1)
    cfg = _cfg(OPS, p=0.5)
    for seed in (0, 23, 2 ** 32 - 1):
        got = F_hip.strong_view_params(x, seed, cfg).cpu().numpy()
        want = O.table(x64, seed, cfg.p16, cfg.lo, cfg.hi)
        assert got.shape == (shape[0], 16) and got.dtype == np.float32
        cols = [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15]
        assert np.array_equal(_bits(got[:, cols]), _bits(want[:, cols])), seed
        ulps = np.abs(got[:, 7].astype(np.float64) - want[:, 7].astype(np.float64)) / np.spacing(np.abs(want[:, 7]))
        print(f"strong_view table {shape} {dtype}: seed {seed}, mean within {ulps.max():.1f} ulp, ops {got[:, 8].tolist()}")
        assert ulps.max() <= 1.0, (seed, ulps)


def test_the_draws_of_many_samples_bit_for_bit_and_their_gates():
    from spcl_amd import functional as F_hip
    x, x64 = _input((700, 1, 3, 5), torch.float32, seed=2)
    cfg = _cfg(OPS, p=0.5)
    got = F_hip.strong_view_params(x, 5, cfg).cpu().numpy()
    want = O.table(x64, 5, cfg.p16, cfg.lo, cfg.hi)
    assert np.array_equal(_bits(got[:, :7]), _bits(want[:, :7])) and np.array_equal(got[:, 8:], want[:, 8:])
    mask = got[:, 5].astype(np.int64)
    for k, name in enumerate(OPS):
        on = (mask >> k) & 1 == 1
        assert 0.4 < on.mean() < 0.6, name
        neutral = np.float32(O.NEUTRAL[k])
        assert (got[~on, k] == neutral).all() and (got[on, k] >= np.float32(cfg.lo[k])).all() and \
            (got[on, k] <= np.float32(cfg.hi[k])).all(), name
    assert np.array_equal(got[:, 8], np.array([bin(m).count("1") for m in mask], dtype=np.float32))


def test_one_seed_gives_the_same_bits_and_the_next_seed_another_table():
    from spcl_amd import functional as F_hip
    x, _ = _input((4, 1, 64, 64), torch.float32, seed=3)
    flags = torch.tensor([0, 1, 2, 3], dtype=torch.uint8, device=DEV)
    cfg = _cfg(OPS)
    ta, tb = [], []
    a = F_hip.strong_view(x, flags, 23, cfg, out=ta)
    b = F_hip.strong_view(x, flags, torch.tensor([23], dtype=torch.int32, device=DEV), cfg, out=tb)
    assert torch.equal(a, b) and torch.equal(ta[0].view(torch.int32), tb[0].view(torch.int32))
    tc = []
    c = F_hip.strong_view(x, flags, 24, cfg, out=tc)
    assert not torch.equal(ta[0][:, :5], tc[0][:, :5]) and not torch.equal(a, c)
    assert torch.equal(ta[0][:, 7], tc[0][:, 7])  # the mean does not depend on the seed


# ------------------------------------------------------------------------------------------------------------------ apply
CONFIGS = [(name,) for name in OPS] + [OPS]


@pytest.mark.parametrize("on", CONFIGS, ids=[c[0] if len(c) == 1 else "all" for c in CONFIGS])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_apply_vs_the_float64_pipeline(shape, on):
    from spcl_amd import functional as F_hip
    shape = _shape(shape)
    x, x64 = _input(shape, torch.float32, seed=4)
    cfg = _cfg(on)
    t = O.table(x64, 31, cfg.p16, cfg.lo, cfg.hi)
    assert (t[:, 5] == sum(1 << OPS.index(name) for name in on)).all()
    c_hi = cfg.hi[1] if "contrast" in on else 1.0
    b_hi = cfg.hi[2] if "brightness" in on else 1.0
    atol = (64 if "gamma" in on else 16) * 2.0 ** -24 * c_hi * b_hi
    td = _dev(t)
    worst = 0.0
    for flags in _flag_sets(shape[0]):
        got = F_hip.strong_view_apply(x, torch.tensor(flags, dtype=torch.uint8, device=DEV), td).cpu().double().numpy()
        pre, want = O.apply(x64, flags, t)
        worst = max(worst, float(np.abs(got - want).max()))
        assert (got[pre > 1.0 + atol] == 1.0).all() and (got[pre < -atol] == 0.0).all()
        assert got.min() >= 0.0 and got.max() <= 1.0
    print(f"strong_view apply {shape} f32 {'+'.join(on)}: max abs err {worst:.3e} (bar {atol:.3e})")
    assert worst <= atol, (worst, atol)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_apply_in_bf16_vs_the_float64_pipeline(shape):
    from spcl_amd import functional as F_hip
    shape = _shape(shape)
    x, x64 = _input(shape, torch.bfloat16, seed=5)
    cfg = _cfg(OPS)
    t = O.table(x64, 32, cfg.p16, cfg.lo, cfg.hi)
    td = _dev(t)
    worst = 0.0
    for flags in _flag_sets(shape[0]):
        got = F_hip.strong_view_apply(x, torch.tensor(flags, dtype=torch.uint8, device=DEV), td)
        assert got.dtype == torch.bfloat16 and got.shape == x.shape
        _, want = O.apply(x64, flags, t)
        worst = max(worst, float(np.abs(got.cpu().double().numpy() - want).max()))
    print(f"strong_view apply {shape} bf16 all: max abs err {worst:.3e} (bar {2.0 ** -8:.3e})")
    assert worst <= 2.0 ** -8


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_an_all_neutral_table_is_flip_batch_bit_for_bit(shape, dtype):
    from spcl_amd import functional as F_hip
    shape = _shape(shape)
    g = torch.Generator().manual_seed(6)
    x = (torch.randn(shape, generator=g) * 3.0).to(dtype).to(DEV)  # far beyond [0, 1]: a copy does not clamp
    x.view(-1)[0] = float("nan")
    t = _dev(O.neutral_table(shape[0], 0.25))
    as_int = torch.int32 if dtype == torch.float32 else torch.int16
    for flags in _flag_sets(shape[0]):
        fl = torch.tensor(flags, dtype=torch.uint8, device=DEV)
        assert torch.equal(F_hip.strong_view_apply(x, fl, t).view(as_int), F_hip.flip_batch(x, fl).view(as_int)), flags
    # ... and so is the whole call with every gate shut
    fl = torch.tensor(_flag_sets(shape[0])[-1], dtype=torch.uint8, device=DEV)
    assert torch.equal(F_hip.strong_view(x, fl, 9, _cfg(())).view(as_int), F_hip.flip_batch(x, fl).view(as_int))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_pointers_off_the_16_byte_grid_take_the_element_path(dtype):
    """W is a multiple of 16 bytes but the batch starts one element into its storage"""
    from spcl_amd import functional as F_hip
    shape = (3, 1, 18, 72)
    g = torch.Generator().manual_seed(7)
    n = shape[0] * shape[2] * shape[3]
    store = (torch.rand(n + 1, generator=g) * 1.2 - 0.1).to(dtype).to(DEV)
    x = store[1:].view(shape)
    assert x.data_ptr() % 16 != 0 and x.is_contiguous()
    aligned = x.clone()
    assert aligned.data_ptr() % 16 == 0
    x64 = x.cpu().double().numpy()
    cfg = _cfg(OPS)
    t = O.table(x64, 33, cfg.p16, cfg.lo, cfg.hi)
    flags = [1, 2, 3]
    fl = torch.tensor(flags, dtype=torch.uint8, device=DEV)
    got = F_hip.strong_view_apply(x, fl, _dev(t))
    # the two access widths run the same arithmetic
    assert torch.equal(got, F_hip.strong_view_apply(aligned, fl, _dev(t)))
    _, want = O.apply(x64, flags, t)
    bar = 64 * 2.0 ** -24 * cfg.hi[1] * cfg.hi[2] if dtype == torch.float32 else 2.0 ** -8
    assert float(np.abs(got.cpu().double().numpy() - want).max()) <= bar
    assert torch.equal(F_hip.strong_view_apply(x, fl, _dev(O.neutral_table(3))), F_hip.flip_batch(x, fl))
    table = F_hip.strong_view_params(x, 33, cfg).cpu().numpy()
    assert np.array_equal(_bits(table[:, :7]), _bits(t[:, :7]))


def test_neutral_and_strong_rows_in_one_batch():
    from spcl_amd import functional as F_hip
    x, x64 = _input((4, 2, 17, 23), torch.float32, seed=8)
    cfg = _cfg(OPS)
    t = O.table(x64, 34, cfg.p16, cfg.lo, cfg.hi)
    t[[0, 2]] = O.neutral_table(2, 0.5)
    flags = [3, 2, 1, 0]
    fl = torch.tensor(flags, dtype=torch.uint8, device=DEV)
    got = F_hip.strong_view_apply(x, fl, _dev(t))
    plain = F_hip.flip_batch(x, fl)
    assert torch.equal(got[[0, 2]], plain[[0, 2]]) and not torch.equal(got[1], plain[1])
    _, want = O.apply(x64, flags, t)
    assert float(np.abs(got.cpu().double().numpy() - want).max()) <= 64 * 2.0 ** -24 * cfg.hi[1] * cfg.hi[2]


def test_a_strided_batch_is_made_contiguous_and_the_input_is_left_alone():
    from spcl_amd import functional as F_hip
    base, _ = _input((3, 2, 20, 24), torch.float32, seed=9)
    x = base[:, :1]  # one channel of two: not contiguous
    assert not x.is_contiguous()
    before = base.clone()
    fl = torch.tensor([1, 2, 3], dtype=torch.uint8, device=DEV)
    cfg = _cfg(OPS)
    got = F_hip.strong_view(x, fl, 3, cfg)
    assert torch.equal(got, F_hip.strong_view(x.contiguous(), fl, 3, cfg)) and torch.equal(base, before)


def test_the_call_captures_into_a_graph_and_replays_with_the_new_seed_word():
    from spcl_amd import functional as F_hip
    x, _ = _input((4, 1, 64, 66), torch.float32, seed=10)
    flags = torch.tensor([0, 1, 2, 3], dtype=torch.uint8, device=DEV)
    cfg = _cfg(OPS)
    word = torch.tensor([23], dtype=torch.int32, device=DEV)

    def call():
        out = []
        return F_hip.strong_view(x, flags, word, cfg, out=out), out[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # (warm-up outside the capture)
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        image, table = call()
    for seed in (23, 24, 25):  # (the word is advanced on the device between the replays, as the hook advances `draw`)
        image.fill_(7.0)
        table.fill_(7.0)
        junk = torch.ones(4096, dtype=torch.bool, device=DEV)  # (an allocation between the replays)
        graph.replay()
        torch.cuda.synchronize()
        keep = []
        want = F_hip.strong_view(x, flags, seed, cfg, out=keep)
        assert torch.equal(image, want) and torch.equal(table.view(torch.int32), keep[0].view(torch.int32)), seed
        del junk
        word.add_(1)
    assert int(word) == 26


# --------------------------------------------------------------------------------------------------------------- refusals
def test_each_refusal_returns_the_error_code_and_launches_nothing():
    from spcl_amd import native
    L = native.lib()
    x = torch.rand(3, 1, 20, 24, device=DEV)
    seed = torch.tensor([1], dtype=torch.int32, device=DEV)
    table = torch.full((3, 16), -5.0, device=DEV)
    out = torch.full((3, 1, 20, 24), -5.0, device=DEV)
    flags = torch.zeros(3, dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for change, word in PARAMS_REFUSALS:
        if change.get("H") == 32768:
            continue  # (the host test covers the size limit: no buffer of that size is made here)
        assert call_params(L, p(x), p(seed), p(table), change) == -1, change
        assert word in L.spcl_last_error(), (change, L.spcl_last_error())
    for change, word in APPLY_REFUSALS:
        if change.get("H") == 32768:
            continue
        assert call_apply(L, p(x), p(out), p(flags), p(table), change) == -1, change
        assert word in L.spcl_last_error(), (change, L.spcl_last_error())
    torch.cuda.synchronize()
    assert bool((table == -5.0).all()) and bool((out == -5.0).all())


def test_the_binding_refuses_flags_and_tables_of_another_kind():
    from spcl_amd import functional as F_hip
    x = torch.rand(3, 1, 8, 8, device=DEV)
    t = _dev(O.neutral_table(3))
    fl = torch.zeros(3, dtype=torch.uint8, device=DEV)
    for bad in (fl[:2], fl.int(), fl.cpu(), [0, 0, 0]):
        with pytest.raises(ValueError, match="flags"):
            F_hip.strong_view_apply(x, bad, t)
    for bad in (t[:2], t[:, :8], t.double(), t.cpu(), None):
        with pytest.raises(ValueError, match="table"):
            F_hip.strong_view_apply(x, fl, bad)
    with pytest.raises(ValueError, match="requires a gradient"):
        F_hip.strong_view_apply(x.clone().requires_grad_(True), fl, t)
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.strong_view_params(x, torch.zeros(1, dtype=torch.int32), _cfg(OPS))  # (the seed word lies on the host)
    torch.cuda.synchronize()
