"""``functional.tta_merge`` / ``spcl_tta_merge`` against the float64 oracle of tests/_tta_oracle.py on its seeded inputs (whose
top-two gap tests/test_tta_host.py asserts on the CPU, so the arg-max is compared at every pixel), the index map with no
tolerance (V exactly flipped / transposed copies of one map merge to the bits of that map alone: a wrong axis, a wrong flip
order or a running sum breaks it), ties, reproducibility across calls of different sizes (the ticket reset) and the
refusals of the C entry."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _tta_oracle as O

pytestmark = pytest.mark.gpu

REL = 1e-5  # relative L2, the bar of tests/test_gpu_semi_reg_kernels.py for the sibling softmax criteria


def _F():
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    return F_hip


def _dev(t, offset=False):
    """CPU [N,C,H,W] f32 -> the logical view of channels-last device storage (``offset``: the storage starts 4 bytes past a
    16-byte boundary)"""
    N, C, H, W = t.shape
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    store = buf[1:1 + t.numel()] if offset else buf[:t.numel()]
    store = store.view(N, H, W, C)
    store.copy_(t.permute(0, 2, 3, 1))
    assert store.data_ptr() % 16 == (4 if offset else 0)
    return store.permute(0, 3, 1, 2)


def _rel(got, want):
    got, want = got.detach().cpu().double(), want.double()
    return float((got - want).norm() / want.norm())


_ORACLE = {}


def _oracle(case):
    """(CPU logits, oracle outputs) of a case, computed once and shared"""
    if case[0] not in _ORACLE:
        logits = O.case_logits(case)
        _ORACLE[case[0]] = (logits, O.merge(logits, case[2]))
    return _ORACLE[case[0]]


@pytest.mark.parametrize("case", O.CASES, ids=[c[0] for c in O.CASES])
def test_merge_against_float64(case):
    F_hip = _F()
    name, shape, ops, _ = case
    logits, (w_prob, w_pred, w_ent, w_mean, gap) = _oracle(case)
    dev = [_dev(t, offset=(name == "offset-4-bytes" and j == 1)) for j, t in enumerate(logits)]
    prob, pred, entropy, mean_entropy = F_hip.tta_merge(dev, ops)
    N, C, H, W = shape
    assert prob.shape == (N, C, H, W) and prob.permute(0, 2, 3, 1).is_contiguous() and prob.dtype == torch.float32
    assert pred.shape == (N, H, W) and pred.dtype == torch.int64
    assert entropy.shape == (N, H, W) and entropy.dtype == torch.float32
    assert mean_entropy.shape == () and mean_entropy.dtype == torch.float32 and mean_entropy.is_cuda
    r_prob, r_ent = _rel(prob, w_prob), _rel(entropy, w_ent)
    r_mean = abs(float(mean_entropy) - w_mean) / abs(w_mean)
    print(f"{name}: rel L2 prob {r_prob:.2e} entropy {r_ent:.2e} mean entropy {r_mean:.2e}; oracle gap {gap:.2e}")
    assert r_prob <= REL and r_ent <= REL and r_mean <= REL
    assert torch.equal(pred.cpu(), w_pred)  # every pixel: the gap is asserted on the host
    assert np.array_equal(pred.cpu().numpy(), prob.cpu().numpy().argmax(axis=1))  # the first maximum of the device's own prob
    # without the entropy map: the same three other outputs
    prob2, pred2, none, mean2 = F_hip.tta_merge(dev, ops, want_entropy=False)
    assert none is None and torch.equal(prob2, prob) and torch.equal(pred2, pred) and torch.equal(mean2, mean_entropy)


@pytest.mark.parametrize("mode,shape", [("flips", (2, 4, 6, 10)), ("flips", (1, 16, 5, 7)), ("dihedral", (2, 4, 8, 8)),
                                        ("dihedral", (2, 5, 12, 12))])
def test_index_map_exact_copies_merge_to_the_bits_of_one(mode, shape):
    F_hip = _F()
    L = 3 * torch.randn(shape, generator=torch.Generator().manual_seed(11))
    ops = O.MODES[mode]
    one = F_hip.tta_merge([_dev(L)], [0])
    for sub in (ops, ops[::-1], ops[:2], ops[-2:]):  # (any order and any sub-tree of the views)
        got = F_hip.tta_merge([_dev(O.view(L, op)) for op in sub], sub)
        for a, b, what in zip(got, one, ("prob", "pred", "entropy", "mean_entropy")):
            assert torch.equal(a, b), (what, sub)
    # and the copies are real views: an asymmetric map read through the WRONG op is another map
    wrong = F_hip.tta_merge([_dev(O.view(L, ops[1]))], [0])
    assert not torch.equal(wrong[0], one[0])


@pytest.mark.parametrize("shape,ops", [((2, 4, 6, 10), (0, 1, 2, 3)), ((2, 5, 12, 12), tuple(range(8))), ((1, 16, 5, 7), (3,)),
                                       ((2, 2, 7, 3), (0, 2))])
def test_ties_go_to_class_zero_and_entropy_is_one(shape, ops):
    F_hip = _F()
    prob, pred, entropy, mean_entropy = F_hip.tta_merge([_dev(torch.zeros(shape)) for _ in ops], ops)
    assert int(pred.abs().max()) == 0
    assert float((prob - 1 / shape[1]).abs().max()) <= 1e-7
    assert float((entropy - 1).abs().max()) <= 1e-6 and abs(float(mean_entropy) - 1) <= 1e-6


def test_two_calls_and_a_call_after_another_size_give_the_same_bits():
    F_hip = _F()
    big, small = O.CASES[1], O.CASES[0]  # 297 pixels (two workgroups) and 120
    dev_big = [_dev(t) for t in O.case_logits(big)]
    dev_small = [_dev(t) for t in O.case_logits(small)]
    first = F_hip.tta_merge(dev_big, big[2])
    again = F_hip.tta_merge(dev_big, big[2])
    small_first = F_hip.tta_merge(dev_small, small[2])
    after = F_hip.tta_merge(dev_big, big[2])
    small_again = F_hip.tta_merge(dev_small, small[2])
    for a, b, c in zip(first, again, after):
        assert torch.equal(a, b) and torch.equal(a, c)
    for a, b in zip(small_first, small_again):
        assert torch.equal(a, b)
    # one workspace serving both sizes in turn: the ticket is back at zero after every call
    from spcl_amd import native as _n
    ws = torch.empty(_n.call("spcl_tta_merge_workspace_bytes", 3, 9, 11), dtype=torch.uint8, device="cuda")
    outs = []
    for dev, case in ((dev_big, big), (dev_small, small), (dev_big, big)):
        outs.append(_raw(dev, case[2], ws=ws))
    for a, b in zip(outs[0], outs[2]):
        assert torch.equal(a, b)
    for a, b in zip(outs[0], first):
        assert torch.equal(a, b.permute(0, 2, 3, 1) if b.dim() == 4 else b)


SENTINEL = -7.0


def _raw(dev, ops, ws=None, ws_bytes=None, C=None, H=None, W=None, expect=None):
    """the C entry itself on sentinel-filled outputs -> (prob storage, pred, entropy, mean_entropy); ``expect``: the message
    of the refusal it must answer with, and the outputs must then be untouched"""
    from spcl_amd import native as _n
    stores = [t.permute(0, 2, 3, 1) for t in dev]
    assert all(s.is_contiguous() for s in stores)
    N, h, w, c = stores[0].shape
    C, H, W = c if C is None else C, h if H is None else H, w if W is None else W
    prob = torch.full((N, h, w, max(c, 17)), SENTINEL, dtype=torch.float32, device="cuda")  # (room for any C the call names)
    if C == c:
        prob = torch.full((N, h, w, c), SENTINEL, dtype=torch.float32, device="cuda")
    pred = torch.full((N, h, w), int(SENTINEL), dtype=torch.int64, device="cuda")
    entropy = torch.full((N, h, w), SENTINEL, dtype=torch.float32, device="cuda")
    mean = torch.full((), SENTINEL, dtype=torch.float32, device="cuda")
    if ws is None:
        ws = torch.empty(_n.call("spcl_tta_merge_workspace_bytes", N, h, w), dtype=torch.uint8, device="cuda")
    args = (_n.ptr_array(stores), (ctypes.c_uint8 * len(ops))(*ops), len(ops), N, C, H, W, ctypes.c_float(1e-16), _n.ptr(prob),
            _n.ptr(pred), _n.ptr(entropy), _n.ptr(mean), _n.ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, _n.stream())
    if expect is None:
        _n.call("spcl_tta_merge", *args)
        return prob, pred, entropy, mean
    with pytest.raises(RuntimeError, match=expect):
        _n.call("spcl_tta_merge", *args)
    torch.cuda.synchronize()
    for t in (prob, entropy, mean):
        assert float((t - SENTINEL).abs().max()) == 0  # nothing was launched
    assert int((pred - int(SENTINEL)).abs().max()) == 0


def test_refusals_launch_nothing():
    from spcl_amd import native as _n
    rect = [_dev(torch.zeros(2, 4, 6, 10)) for _ in range(2)]
    # C = 1 and C = 17, named over storage that is large enough for neither to matter
    wide = [_dev(torch.zeros(2, 17, 6, 10)) for _ in range(2)]
    _raw(wide, (0, 1), C=1, expect=r"C = 1 classes \(2 <= C <= 16\)")
    _raw(wide, (0, 1), C=17, expect=r"C = 17 classes \(2 <= C <= 16\)")
    # the axis swap on a non-square map
    _raw(rect, (0, 4), expect=r"needs H == W, given 6 x 10")
    _raw(rect, (0, 7), expect=r"needs H == W")
    # a workspace one byte short, and none
    need = _n.call("spcl_tta_merge_workspace_bytes", 2, 6, 10)
    assert need >= 8 + 4
    _raw(rect, (0, 1), ws_bytes=need - 1, expect="workspace too small")
    _raw(rect, (0, 1), ws_bytes=0, expect="workspace too small")
    # an op outside the table and a view count outside the tree
    _raw(rect, (0, 8), expect=r"op 8 of view 1")
    _raw(rect + rect[:1], (0, 1, 2), expect=r"V = 3 views")
    # the binding raises the library's message as it is
    F_hip = _F()
    with pytest.raises(RuntimeError, match=r"C = 17 classes"):
        F_hip.tta_merge(wide, (0, 1))
    # and the same arguments are accepted once they are in range
    prob, pred, entropy, mean = _raw(rect, (0, 1))
    assert float((prob - 0.25).abs().max()) <= 1e-7 and int(pred.abs().max()) == 0 and abs(float(mean) - 1) <= 1e-6
