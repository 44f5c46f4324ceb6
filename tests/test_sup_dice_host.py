"""CPU-only side of the soft-Dice / class-weighted supervised criteria (contrastyou/losses/dice.py, csrc/sup_dice.hip): the
float64 oracle of tests/_sup_dice_oracle.py on known answers, every refusal of the criterion, ``build_sup_criterion`` and the
three entry points of the C ABI."""
import ctypes
import os
import re

import pytest
import torch

from tests import _sup_dice_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "spcl_hip.h")
LIB = os.path.join(REPO, "self-paced-contrastive-learning_amd", "lib", "libspcl_hip.so")
SYMBOLS = ("spcl_sup_dice_workspace_bytes", "spcl_sup_dice_forward", "spcl_sup_dice_backward")


def _case(N=2, C=4, H=9, W=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, C, H, W, generator=g), torch.randint(0, C, (N, H, W), generator=g)


# ---- the oracle
@pytest.mark.parametrize("per_sample", [False, True])
def test_oracle_without_dice_and_unit_weights_is_kl_div(per_sample):
    logits, labels = _case()
    loss, l_kl, _ = O.dice_kl(logits, labels, dice_weight=0.0, kl_weight=1.0, per_sample=per_sample)
    ref = O.kl_div_onehot(logits, labels)
    assert abs(float(loss) - float(ref)) <= 1e-14 * abs(float(ref)) and float(l_kl) == float(loss)
    # and a weight vector scales the terms of its class
    w = [0.5, 2.0, 1.0, 0.0]
    lw, _, _ = O.dice_kl(logits, labels, dice_weight=0.0, class_weight=w)
    p = logits.double().softmax(1)
    per_pixel = -torch.log((p.gather(1, labels.unsqueeze(1)).squeeze(1) + 1e-16) / (1 + 1e-16))
    assert abs(float(lw) - float((torch.tensor(w, dtype=torch.float64)[labels] * per_pixel).mean())) < 1e-14


@pytest.mark.parametrize("include_background", [True, False])
@pytest.mark.parametrize("per_sample", [False, True])
def test_oracle_perfect_prediction_has_no_dice_loss(per_sample, include_background):
    _, labels = _case(seed=3)
    logits = 200.0 * O.one_hot(labels, 4).float()  # softmax = the one-hot map to within exp(-200)
    _, _, l_dice = O.dice_kl(logits, labels, per_sample=per_sample, include_background=include_background)
    assert 0.0 <= float(l_dice) < 1e-12
    _, _, worst = O.dice_kl(-logits, labels, per_sample=per_sample, include_background=include_background)
    assert float(worst) > 0.9


def test_oracle_out_of_range_label_is_an_all_zero_row():
    logits, labels = _case(seed=5)
    marked = labels.clone()
    marked[0, 2, 3], marked[1, 0, 0] = 255, -1
    keep = torch.ones_like(labels, dtype=torch.bool)
    keep[0, 2, 3] = keep[1, 0, 0] = False
    loss, l_kl, _ = O.dice_kl(logits, marked, dice_weight=0.0)
    p = logits.double().softmax(1)
    per_pixel = -torch.log((p.gather(1, labels.unsqueeze(1)).squeeze(1) + 1e-16) / (1 + 1e-16))
    assert abs(float(l_kl) - float((per_pixel * keep).sum() / labels.numel())) < 1e-14  # (M still counts every pixel)
    t = O.one_hot(marked, 4)
    assert float(t[0, :, 2, 3].sum()) == 0.0 and float(t.sum()) == labels.numel() - 2


# ---- refusals
def test_constructor_refusals():
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses import DiceKLLoss, SoftDiceLoss, WeightedKL
    for smooth in (0.0, -1e-5):
        with pytest.raises(ValueError, match="smooth"):
            DiceKLLoss(smooth=smooth)
    for w in ([1.0, -0.1, 1.0, 1.0], [1.0, float("nan"), 1.0, 1.0], [float("inf"), 1.0, 1.0, 1.0]):
        with pytest.raises(ValueError, match="weights"):
            DiceKLLoss(class_weight=w)
        with pytest.raises(ValueError, match="weights"):
            WeightedKL(class_weight=w)
    with pytest.raises(ValueError, match="both zero"):
        DiceKLLoss(dice_weight=0.0, kl_weight=0.0)
    assert SoftDiceLoss().kl_weight == 0.0 and SoftDiceLoss().dice_weight == 1.0
    assert WeightedKL([1.0, 2.0]).dice_weight == 0.0 and WeightedKL([1.0, 2.0]).class_weight == (1.0, 2.0)


def test_call_refusals_come_before_the_device_check():
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses import DiceKLLoss, SoftDiceLoss
    logits, labels = _case()
    with pytest.raises(ValueError, match="class weights for 4 classes"):
        DiceKLLoss(class_weight=[1.0, 2.0, 3.0]).from_logits(logits, labels)
    with pytest.raises(ValueError, match="no class"):
        SoftDiceLoss(include_background=False).from_logits(logits[:, :1], labels)
    with pytest.raises(ValueError, match="at most"):
        DiceKLLoss().from_logits(torch.zeros(1, 17, 2, 2), torch.zeros(1, 2, 2, dtype=torch.long))
    with pytest.raises(ValueError, match="at most"):
        DiceKLLoss().from_logits(torch.zeros(1025, 2, 1, 1), torch.zeros(1025, 1, 1, dtype=torch.long))


def test_cpu_tensor_raises_the_device_error():
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses import DiceKLLoss
    from spcl_amd.contrastyou.losses.kl import KL_div
    logits, labels = _case()
    crit = DiceKLLoss(class_weight=[1.0, 2.0, 0.5, 1.0])
    with pytest.raises(RuntimeError, match="MI355X"):
        crit.from_logits(logits, labels)
    with pytest.raises(RuntimeError, match="MI355X"):
        crit(logits.softmax(1), O.one_hot(labels, 4).float(), disable_assert=True)
    with pytest.raises(AssertionError, match="one-hot"):
        crit(logits.softmax(1), logits.softmax(1))
    assert not isinstance(crit, KL_div)  # (the epochers' isinstance tests keep their meaning)


# ---- configuration
def test_build_sup_criterion():
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses import DiceKLLoss, SoftDiceLoss, WeightedKL, build_sup_criterion
    from spcl_amd.contrastyou.losses.kl import KL_div
    for cfg in ({}, None, {"Trainer": {}}, {"SupCriterion": {"name": "kl"}}, {"SupCriterion": None}):
        assert type(build_sup_criterion(cfg)) is KL_div
    c = build_sup_criterion({"SupCriterion": {"name": "dice", "include_background": False, "per_sample": True, "smooth": 1.0}})
    assert type(c) is SoftDiceLoss and (c.include_background, c.per_sample, c.smooth, c.kl_weight) == (False, True, 1.0, 0.0)
    c = build_sup_criterion({"SupCriterion": {"name": "dice_kl", "dice_weight": 0.5, "kl_weight": 2.0,
                                              "class_weight": [0.2, 1.0, 1.0, 3.0]}})
    assert type(c) is DiceKLLoss and (c.dice_weight, c.kl_weight, c.class_weight) == (0.5, 2.0, (0.2, 1.0, 1.0, 3.0))
    c = build_sup_criterion({"SupCriterion": {"name": "weighted_kl", "class_weight": [1.0, 4.0]}})
    assert type(c) is WeightedKL and c.class_weight == (1.0, 4.0) and c.dice_weight == 0.0
    with pytest.raises(ValueError, match="one of"):
        build_sup_criterion({"SupCriterion": {"name": "focal"}})
    with pytest.raises(ValueError, match="does not take"):
        build_sup_criterion({"SupCriterion": {"name": "weighted_kl", "smooth": 1.0}})
    with pytest.raises(ValueError, match="does not take"):
        build_sup_criterion({"SupCriterion": {"name": "kl", "class_weight": [1.0, 2.0]}})


def test_graph_key_tells_two_weightings_apart():
    import spcl_amd  # noqa: F401
    from spcl_amd.contrastyou.losses import DiceKLLoss, SoftDiceLoss
    a, b = DiceKLLoss(class_weight=[1.0, 2.0, 1.0, 1.0]), DiceKLLoss(class_weight=[1.0, 2.5, 1.0, 1.0])
    assert a.graph_key() != b.graph_key() and a.graph_key() == DiceKLLoss(class_weight=[1.0, 2.0, 1.0, 1.0]).graph_key()
    keys = {DiceKLLoss().graph_key(), DiceKLLoss(dice_weight=2.0).graph_key(), DiceKLLoss(kl_weight=2.0).graph_key(),
            DiceKLLoss(include_background=False).graph_key(), DiceKLLoss(per_sample=True).graph_key(),
            DiceKLLoss(smooth=1.0).graph_key(), DiceKLLoss(eps=1e-8).graph_key(), SoftDiceLoss().graph_key()}
    assert len(keys) == 8
    hash(a.graph_key())


# ---- the C ABI
def test_header_native_and_library_agree_on_the_entries():
    import spcl_amd  # noqa: F401
    from spcl_amd import native
    hdr = open(HEADER).read()
    assert int(re.search(r"#define\s+SPCL_ABI_VERSION\s+(\d+)", hdr).group(1)) == native.ABI_VERSION >= 31
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "size_t spcl_sup_dice_workspace_bytes(int N, int C, int H, int W);" in flat
    for name in SYMBOLS:
        assert name in native._SIGNATURES and re.search(r"\b%s\s*\(" % name, flat)
    assert len(native._SIGNATURES["spcl_sup_dice_forward"][1]) == 21
    assert len(native._SIGNATURES["spcl_sup_dice_backward"][1]) == 15
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(LIB)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    ws = lib.spcl_sup_dice_workspace_bytes
    ws.restype, ws.argtypes = ctypes.c_size_t, [ctypes.c_int] * 4
    assert ws(32, 4, 224, 224) > 0 and ws(32, 4, 224, 224) % 16 == 0
    assert ws(2, 17, 8, 8) == 0 and ws(1025, 4, 8, 8) == 0 and ws(0, 4, 8, 8) == 0  # (beyond the head kernels' limits)
    lib.spcl_last_error.restype = ctypes.c_char_p
    rc = lib.spcl_sup_dice_forward(None, None, None, 1, 4, 8, 8, ctypes.c_float(1), ctypes.c_float(1), 1, 0,
                                   ctypes.c_float(1e-5), ctypes.c_float(1e-16), None, None, None, None, None, None,
                                   ctypes.c_size_t(0), None)
    assert rc == -1 and b"null" in lib.spcl_last_error()
