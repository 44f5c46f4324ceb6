"""CPU-only side of the boundary loss (contrastyou/losses/boundary.py, csrc/boundary.hip): the scipy oracle of
tests/_boundary_oracle.py against an integer brute force, ``build_sup_criterion``'s new name, every refusal of the criterion,
the alpha schedule, the graph key, the device error and the entry points of the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _boundary_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "spcl_hip.h")
LIB = os.path.join(REPO, "self-paced-contrastive-learning_amd", "lib", "libspcl_hip.so")
SYMBOLS = ("spcl_signed_distance_workspace_bytes", "spcl_signed_distance_maps", "spcl_boundary_workspace_bytes",
           "spcl_boundary_forward", "spcl_boundary_backward")
SHAPES = [(1, 1), (1, 70), (13, 1), (13, 70), (9, 130), (37, 65)]


def _fill(shape, kind, seed):
    H, W = shape
    if kind == "rect":
        m = np.zeros(shape, dtype=bool)
        m[H // 4:max(H // 4 + 1, 3 * H // 4), W // 3:max(W // 3 + 1, 2 * W // 3)] = True
        return m
    return np.random.default_rng(seed).random(shape) < kind


# ---- the oracle
@pytest.mark.parametrize("kind", [0.02, 0.5, 0.98, "rect"])
@pytest.mark.parametrize("shape", SHAPES)
def test_scipy_reference_is_the_integer_brute_force(shape, kind):
    m = _fill(shape, kind, seed=shape[0] * 1000 + shape[1])
    ref, brute = O.signed_distance_plane(m), O.signed_distance_brute(m)
    assert ref.dtype == np.float64 and np.array_equal(ref, brute), int((ref != brute).sum())
    if m.any() and not m.all():
        assert (ref[m] <= 0).all() and (ref[~m] >= 1).all()


def test_reference_rules_absent_full_and_touching_pixels():
    assert not O.signed_distance_plane(np.zeros((4, 5), bool)).any()
    assert not O.signed_distance_plane(np.ones((4, 5), bool)).any()   # (scipy alone: 1 .. 5.66, to a corner outside the image)
    m = np.zeros((5, 7), bool)
    m[1:4, 2:5] = True
    phi = O.signed_distance_plane(m)
    assert phi[2, 3] == -1.0 and phi[1, 2] == 0.0 and phi[0, 0] == np.sqrt(5.0) and phi[2, 6] == 2.0
    labels = torch.tensor([[[0, 2, 2], [7, 2, -1]]])
    out = O.signed_distance_ref(labels, (2, 3))
    assert out.dtype == torch.float32 and tuple(out.shape) == (1, 2, 2, 3)
    assert not out[0, 1].any() and out[0, 0, 1, 0] == 1.0 and out[0, 0, 0, 0] == 1.0  # (7 and -1 belong to no class)


def test_oracle_loss_is_region_plus_alpha_times_mean():
    g = torch.Generator().manual_seed(0)
    logits, labels = torch.randn(2, 4, 9, 7, generator=g), torch.randint(0, 4, (2, 9, 7), generator=g)
    loss, l_region, l_b, a = O.boundary_loss(logits, labels, alpha=0.25, classes=(1, 3), include_background=False)
    from tests import _sup_dice_oracle as R
    assert float(l_region) == float(R.dice_kl(logits, labels, include_background=False)[0])
    phi = O.signed_distance_ref(labels, (1, 3)).double()
    p = logits.double().softmax(1)
    want = (p[:, 1] * phi[:, 0] + p[:, 3] * phi[:, 1]).sum() / (2 * 2 * 9 * 7)
    assert abs(float(l_b) - float(want)) < 1e-15 and float(a) >= abs(float(l_b))
    assert abs(float(loss) - (float(l_region) + 0.25 * float(l_b))) < 1e-15
    # the gradient of the issue's closed form: p_k (a_k - sum_c a_c p_c)
    _, grad, _, _, _ = O.boundary_loss_with_grad(logits, labels, alpha=0.25, classes=(1, 3), dice_weight=0.0, kl_weight=1e-30)
    a_c = torch.zeros(2, 4, 9, 7, dtype=torch.float64)
    a_c[:, 1], a_c[:, 3] = 0.25 * phi[:, 0] / (2 * 2 * 9 * 7), 0.25 * phi[:, 1] / (2 * 2 * 9 * 7)
    closed = p * (a_c - (a_c * p).sum(1, keepdim=True))
    assert float((grad - closed).abs().max()) < 1e-15


# ---- configuration
def test_build_sup_criterion_boundary():
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses import BoundaryLoss, DiceKLLoss, build_sup_criterion
    from spcl_amd.contrastyou.losses.kl import KL_div
    c = build_sup_criterion({"SupCriterion": {"name": "boundary"}})
    assert type(c) is BoundaryLoss and type(c.region) is DiceKLLoss and c.classes is None
    assert (c.alpha, c.alpha_step, c.alpha_max) == (0.01, 0.01, 1.0)
    c = build_sup_criterion({"SupCriterion": {"name": "boundary", "alpha": 0.05, "alpha_step": 0.02, "alpha_max": 0.5,
                                              "classes": [1, 3], "dice_weight": 0.5, "kl_weight": 2.0,
                                              "class_weight": [0.2, 1.0, 1.0, 3.0], "include_background": False,
                                              "per_sample": True, "smooth": 1.0}})
    assert (c.alpha, c.alpha_step, c.alpha_max, c.classes) == (0.05, 0.02, 0.5, (1, 3))
    r = c.region
    assert (r.dice_weight, r.kl_weight, r.class_weight, r.include_background, r.per_sample, r.smooth) == \
        (0.5, 2.0, (0.2, 1.0, 1.0, 3.0), False, True, 1.0)
    assert not isinstance(c, KL_div) and hasattr(c, "from_logits")
    # the messages keep their wording
    with pytest.raises(ValueError, match="one of"):
        build_sup_criterion({"SupCriterion": {"name": "focal"}})
    with pytest.raises(ValueError, match="does not take"):
        build_sup_criterion({"SupCriterion": {"name": "boundary", "gamma": 2.0}})
    with pytest.raises(ValueError, match="does not take"):
        build_sup_criterion({"SupCriterion": {"name": "dice_kl", "alpha": 0.1}})
    assert type(build_sup_criterion({})) is KL_div


def test_constructor_refusals():
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses import BoundaryLoss, SoftDiceLoss
    from spcl_amd.contrastyou.losses.kl import KL_div
    for name in ("alpha", "alpha_step", "alpha_max"):
        for bad in (-0.1, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=name):
                BoundaryLoss(**{name: bad})
    for classes in ((1, 1), (2, 3, 2), ()):
        with pytest.raises(ValueError, match="distinct"):
            BoundaryLoss(classes=classes)
    for classes in ((-1, 2), (16,)):
        with pytest.raises(ValueError, match="classes"):
            BoundaryLoss(classes=classes)
    with pytest.raises(ValueError, match="region"):
        BoundaryLoss(region=KL_div())
    assert type(BoundaryLoss(region=SoftDiceLoss()).region) is SoftDiceLoss
    assert BoundaryLoss(alpha=0.0).alpha == 0.0 and BoundaryLoss(classes=[0, 2]).classes == (0, 2)


def test_call_refusals_come_before_the_device_check():
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses import BoundaryLoss

    def call(crit, N, C, H, W):
        return crit.from_logits(torch.zeros(N, C, H, W), torch.zeros(N, H, W, dtype=torch.long))
    with pytest.raises(ValueError, match="at most"):
        call(BoundaryLoss(), 1, 17, 2, 2)
    with pytest.raises(ValueError, match="at most"):
        call(BoundaryLoss(), 1025, 2, 1, 1)
    with pytest.raises(ValueError, match="1024 x 1024"):
        call(BoundaryLoss(), 1, 2, 1025, 1)
    with pytest.raises(ValueError, match="1024 x 1024"):
        call(BoundaryLoss(), 1, 2, 1, 1025)
    with pytest.raises(ValueError, match="not all in"):
        call(BoundaryLoss(classes=(1, 4)), 1, 4, 2, 2)
    with pytest.raises(ValueError, match="empty"):
        call(BoundaryLoss(), 1, 1, 2, 2)   # (the default 1 .. C-1 of a one-class map)
    with pytest.raises(ValueError, match="labels"):
        BoundaryLoss().from_logits(torch.zeros(1, 2, 2, 2), torch.zeros(1, 1, 2, 2, dtype=torch.long))


def test_set_epoch_is_a_pure_function_of_the_epoch():
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses import BoundaryLoss
    c = BoundaryLoss(alpha=0.01, alpha_step=0.02, alpha_max=0.1)
    assert c.alpha == 0.01
    want = {1: 0.01, 2: 0.03, 3: 0.05, 5: 0.09, 6: 0.1, 7: 0.1, 100: 0.1, 0: 0.01}
    for epoch in (3, 1, 100, 2, 6, 5, 7, 0, 3):  # (any order: no state but the epoch)
        assert c.set_epoch(epoch) == c.alpha == min(0.1, 0.01 + 0.02 * max(epoch - 1, 0))
        assert abs(c.alpha - want[epoch]) < 1e-12
    assert BoundaryLoss(alpha=2.0, alpha_max=1.0).alpha == 1.0
    assert BoundaryLoss(alpha=0.3, alpha_step=0.0).set_epoch(50) == 0.3
    assert "alpha" not in "".join(c.state_dict().keys())  # (a resumed run needs no saved state)


def test_graph_key_ignores_alpha():
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses import BoundaryLoss, DiceKLLoss
    a, b = BoundaryLoss(alpha=0.01), BoundaryLoss(alpha=0.5, alpha_step=0.1, alpha_max=3.0)
    assert a.graph_key() == b.graph_key()
    before = a.graph_key()
    a.set_epoch(40)
    assert a.graph_key() == before and hash(before) is not None
    keys = {a.graph_key(), BoundaryLoss(classes=(1, 2)).graph_key(), BoundaryLoss(classes=(2, 1)).graph_key(),
            BoundaryLoss(region=DiceKLLoss(per_sample=True)).graph_key(),
            BoundaryLoss(region=DiceKLLoss(class_weight=[1.0, 2.0])).graph_key(), DiceKLLoss().graph_key()}
    assert len(keys) == 6
    assert a._eps == a.region._eps  # (the epochers' keys read it)


def test_cpu_tensors_raise_the_device_error():
    import spcl_amd  # noqa: F401
    from spcl_amd import functional as F_hip
    from spcl_amd.contrastyou.losses import BoundaryLoss
    g = torch.Generator().manual_seed(0)
    logits, labels = torch.randn(2, 4, 9, 7, generator=g), torch.randint(0, 4, (2, 9, 7), generator=g)
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.signed_distance_maps(labels, (1, 2, 3))
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.boundary_loss(logits, torch.zeros(2, 3, 9, 7), (1, 2, 3), torch.tensor(0.1))
    crit = BoundaryLoss()
    with pytest.raises(RuntimeError, match="MI355X"):
        crit.from_logits(logits, labels)
    onehot = (labels.unsqueeze(1) == torch.arange(4).view(1, 4, 1, 1)).float()
    with pytest.raises(RuntimeError, match="MI355X"):
        crit(logits.softmax(1), onehot, disable_assert=True)
    with pytest.raises(AssertionError, match="one-hot"):
        crit(logits.softmax(1), logits.softmax(1))
    for bad in ((1, 1), (), (-1,), tuple(range(17))):
        with pytest.raises(ValueError, match="distinct"):
            F_hip.signed_distance_maps(labels, bad)


def test_begin_epoch_asks_the_class_not_the_instance():
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses import BoundaryLoss
    from spcl_amd.semi_seg.epochers.helper import begin_epoch

    class Recorder:
        def __init__(self):
            self.asked = []

        def __getattr__(self, name):
            self.asked.append(name)
            raise AttributeError(name)
    r = Recorder()
    begin_epoch(r, 3)
    assert r.asked == []
    c = BoundaryLoss(alpha=0.01, alpha_step=0.01)
    begin_epoch(c, 4)
    assert abs(c.alpha - 0.04) < 1e-12


# ---- the C ABI
def test_header_native_and_library_agree_on_the_entries():
    import spcl_amd  # noqa: F401
    from spcl_amd import native
    hdr = open(HEADER).read()
    assert int(re.search(r"#define\s+SPCL_ABI_VERSION\s+(\d+)", hdr).group(1)) == native.ABI_VERSION >= 32
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "size_t spcl_signed_distance_workspace_bytes(int N, int H, int W, int n_classes);" in flat
    for name in SYMBOLS:
        assert name in native._SIGNATURES and re.search(r"\b%s\s*\(" % name, flat)
    assert len(native._SIGNATURES["spcl_signed_distance_maps"][1]) == 10
    assert len(native._SIGNATURES["spcl_boundary_forward"][1]) == 14
    assert len(native._SIGNATURES["spcl_boundary_backward"][1]) == 12
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.spcl_abi_version() >= 32
    ws = lib.spcl_signed_distance_workspace_bytes
    ws.restype, ws.argtypes = ctypes.c_size_t, [ctypes.c_int] * 4
    assert ws(32, 224, 224, 3) >= 32 * 3 * 2 * 224 * 224 * 2 and ws(32, 224, 224, 3) % 16 == 0
    assert ws(1, 1024, 1024, 16) > 0
    for bad in ((1025, 8, 8, 1), (1, 1025, 8, 1), (1, 8, 1025, 1), (1, 8, 8, 17), (1, 8, 8, 0), (0, 8, 8, 1)):
        assert ws(*bad) == 0, bad
    wb = lib.spcl_boundary_workspace_bytes
    wb.restype, wb.argtypes = ctypes.c_size_t, [ctypes.c_int] * 3
    assert wb(32, 224, 224) > 0 and wb(1025, 8, 8) == 0
    lib.spcl_last_error.restype = ctypes.c_char_p
    rc = lib.spcl_signed_distance_maps(None, 1, 8, 8, None, 1, None, None, ctypes.c_size_t(0), None)
    assert rc == -1 and b"null" in lib.spcl_last_error()
    rc = lib.spcl_signed_distance_maps(None, 1, 2048, 8, None, 1, None, None, ctypes.c_size_t(0), None)
    assert rc == -1 and b"bad shape" in lib.spcl_last_error()
    rc = lib.spcl_boundary_forward(None, None, None, 1, 1, 4, 8, 8, None, None, None, None, ctypes.c_size_t(0), None)
    assert rc == -1 and b"null" in lib.spcl_last_error()
    # the class list is checked on the host, before any launch: duplicates and classes outside [0, C)
    one = ctypes.c_void_p(16)  # (never dereferenced: the call is refused first)
    for classes, word in (((1, 1), b"twice"), ((1, 4), b"not in"), ((-1,), b"not in")):
        arr = (ctypes.c_int * len(classes))(*classes)
        rc = lib.spcl_boundary_backward(one, one, arr, len(classes), 1, 4, 8, 8, one, None, one, None)
        assert rc == -1 and word in lib.spcl_last_error(), (classes, lib.spcl_last_error())
